"""Time of the per-frame rectification (ops.rectify_u8, include/dbw_lens.h) for one chunk of a custom capture, by the protocol of
tools/bench_lens.py: 16 raw frames of 540x960 resident on the GPU, taken by four distinct cameras, -> 16 frames of one pinhole camera.
The new kernel with radial-tangential cameras and with fisheye cameras, the shared-map kernel (ops.undistort_u8: one camera for the
chunk) and the resize launch that follows on the same chunk (ops.resample_u8 to 270x480) alternate in one process, all warmed up, device
events around each call, --reps repetitions.  The first frame of both models is compared with the host build of the header before
anything is timed.  Prints one JSON line.

--once: a few launches of each, no timing (for a rocprofv3 --kernel-trace --stats run of its own)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'differentiable-blocksworld_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np                              # noqa: E402
import torch                                    # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--H', type=int, default=540)
    ap.add_argument('--W', type=int, default=960)
    ap.add_argument('--downscale', type=int, default=2)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    from bench_ingest import photo_like
    from dbw_amd import dataset, ops
    assert torch.cuda.is_available(), 'needs a GPU: there is no CPU path to time'
    import rectify_ref as RF
    dev = 'cuda:0'
    N, H, W = args.frames, args.H, args.W
    size = (round(H / args.downscale), round(W / args.downscale))
    cams = list(RF.cameras(H, W).values())[:3] + [(0.9 * W, 0.92 * W, W // 2 + 0.5, H // 2 + 0.5)]      # (D: a principal point on a pixel centre)
    intrs = [cams[n % 4] for n in range(N)]
    dist = {0: (0.12, 0.02, 0.0, 0.0, 0.003, -0.002), 1: RF.FISHEYE_COEFFS[0] + (0.0, 0.0)}
    tgt = dataset.common_pinhole(intrs)
    rng = np.random.RandomState(0)
    frames = np.stack([photo_like(rng, H, W) for _ in range(min(N, 4))])
    frames = np.concatenate([frames] * (-(-N // len(frames))))[:N]
    src = torch.from_numpy(frames).to(dev)
    tables, zooms = {}, {}
    for model in (0, 1):
        zooms[model] = dataset.rectify_zoom(H, W, intrs, [dist[model]] * N, [model] * N, tgt)
        tables[model] = (ops.lens_table(intrs, [dist[model]] * N, [model] * N), ops.lens_target(tgt, zooms[model]))
    shared_zoom = dataset.lens_zoom(H, W, cams[0], dist[0])
    calls = {'rectify_radtan': lambda: ops.rectify_u8(src, *tables[0]), 'rectify_fisheye': lambda: ops.rectify_u8(src, *tables[1]),
             'undistort_shared': lambda: ops.undistort_u8(src, cams[0], dist[0], shared_zoom), 'resample': lambda: ops.resample_u8(src, size)}
    for f in calls.values():                                            # warm-up: code objects, tables, the allocator's blocks
        f()
    torch.cuda.synchronize()
    differing = {}
    for model, name in ((0, 'rectify_radtan'), (1, 'rectify_fisheye')):
        got = calls[name]()[:1].cpu().numpy()
        differing[name] = int((got != RF.rectify_host(frames[:1], tables[model][0][:1], tables[model][1])).sum())
        assert differing[name] == 0, f'{name}: {differing[name]} bytes differ from the host build of lens_math.h'
    if args.once:
        for _ in range(3):
            for f in calls.values():
                f()
        torch.cuda.synchronize()
        return
    times = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, f in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e-3)
    chunk = N * H * W * 3
    moved = {k: 2 * chunk for k in calls}
    moved['resample'] = chunk + N * 3 * size[0] * size[1] * 4
    res = {'frames': N, 'raw': [H, W], 'img_size': list(size), 'zoom': {'radtan': round(zooms[0], 6), 'fisheye': round(zooms[1], 6), 'shared': round(shared_zoom, 6)},
           'reps': args.reps, 'bytes_differing_from_host_build': differing}
    for k in calls:
        t = float(np.median(times[k]))
        res[k] = {'median_ms': round(t * 1e3, 4), 'min_ms': round(min(times[k]) * 1e3, 4), 'max_ms': round(max(times[k]) * 1e3, 4),
                  'bytes_moved': moved[k], 'GB_per_s': round(moved[k] / t / 1e9, 1), 'share_of_hbm_peak': round(moved[k] / t / HBM_PEAK, 4)}
    shared = res['undistort_shared']['median_ms']
    res['ratio_to_shared_map'] = {k: round(res[k]['median_ms'] / shared, 3) for k in ('rectify_radtan', 'rectify_fisheye')}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
