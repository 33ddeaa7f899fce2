"""Time of the lens rectification (ops.undistort_u8, include/dbw_lens.h) for one chunk of a custom capture: 16 raw frames of 540x960
resident on the GPU -> 16 rectified frames, next to the resize launch that follows it on the same chunk (ops.resample_u8 to 270x480) and
a device-to-device copy of the bytes the rectification has to move at the least (the chunk read once and written once).  All three warmed
up, alternating in one process, device events around each call, --reps repetitions.  The output is compared with the host build of the
header on the first frame before anything is timed.  Prints one JSON line.

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
    dev = 'cuda:0'
    N, H, W = args.frames, args.H, args.W
    size = (round(H / args.downscale), round(W / args.downscale))
    intr, dist = (0.9 * W, 0.92 * W, 0.51 * W, 0.48 * H), (0.12, 0.02, 0.0, 0.0, 0.003, -0.002)
    zoom = dataset.lens_zoom(H, W, intr, dist)
    rng = np.random.RandomState(0)
    frames = np.stack([photo_like(rng, H, W) for _ in range(min(N, 4))])
    frames = np.concatenate([frames] * (-(-N // len(frames))))[:N]
    src = torch.from_numpy(frames).to(dev)
    dst = torch.empty_like(src)
    calls = {'undistort': lambda: ops.undistort_u8(src, intr, dist, zoom), 'resample': lambda: ops.resample_u8(src, size),
             'copy': lambda: dst.copy_(src)}
    for f in calls.values():                                            # warm-up: code objects, tables, the allocator's blocks
        f()
    torch.cuda.synchronize()
    import lens_ref
    got = calls['undistort']()[:1].cpu().numpy()
    differing = int((got != lens_ref.undistort_host(frames[:1], intr, dist, zoom)).sum())
    assert differing == 0, f'{differing} bytes differ from the host build of lens_math.h'
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
    moved = {'undistort': 2 * chunk, 'resample': chunk + N * 3 * size[0] * size[1] * 4, 'copy': 2 * chunk}
    res = {'frames': N, 'raw': [H, W], 'img_size': list(size), 'zoom': round(zoom, 6), 'reps': args.reps, 'bytes_differing_from_host_build': differing}
    for k in calls:
        t = float(np.median(times[k]))
        res[k] = {'median_ms': round(t * 1e3, 4), 'min_ms': round(min(times[k]) * 1e3, 4), 'max_ms': round(max(times[k]) * 1e3, 4),
                  'bytes_moved': moved[k], 'GB_per_s': round(moved[k] / t / 1e9, 1), 'share_of_hbm_peak': round(moved[k] / t / HBM_PEAK, 4)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
