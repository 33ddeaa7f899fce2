"""Time of the image ingest (ops.resample_u8, include/dbw_ingest.h) for one DTU scan: 49 raw frames of 1200x1600 resident on the GPU ->
49 targets of 300x400, both kernel forms, warmed up, alternating in one process, device events around --reps launches each.  The bytes
each form moves are counted from the shapes and set against the HBM peak of 8 TB/s.  For context, the seconds the host spends in PIL
decode and in PIL resize of the same 49 frames (written as PNG files into --tmp first), serially and on a pool of 16 threads, and the
time of the pinned upload.  Prints one JSON line.

--once: a few launches of each form, no timing (for a rocprofv3 --kernel-trace --stats run of its own)."""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'differentiable-blocksworld_amd'))

import numpy as np                              # noqa: E402
import torch                                    # noqa: E402

HBM_PEAK = 8.0e12


def photo_like(rng, H, W):
    """A frame with the statistics that matter to a PNG decoder more than white noise does: smooth shading plus mild sensor noise."""
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 100 * np.sin(x / (40.0 + 7 * c) + rng.rand() * 6) * np.cos(y / (55.0 + 5 * c) + rng.rand() * 6) for c in range(3)], -1)
    return np.clip(base + rng.randn(H, W, 3) * 4, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=49)
    ap.add_argument('--Hin', type=int, default=1200)
    ap.add_argument('--Win', type=int, default=1600)
    ap.add_argument('--H', type=int, default=300)
    ap.add_argument('--W', type=int, default=400)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--no-host', action='store_true', help='skip the PIL decode / resize context numbers')
    ap.add_argument('--tmp', default=None)
    args = ap.parse_args()
    from dbw_amd import _lib, ops
    assert torch.cuda.is_available(), 'needs a GPU: there is no CPU path to time'
    dev = 'cuda:0'
    N, Hin, Win, H, W = args.views, args.Hin, args.Win, args.H, args.W
    rng = np.random.RandomState(0)
    frames = np.stack([photo_like(rng, Hin, Win) for _ in range(min(N, 4))])
    frames = np.concatenate([frames] * (-(-N // len(frames))))[:N]
    pinned = torch.from_numpy(frames).pin_memory()
    src = pinned.to(dev)
    out = {}
    for form in ('fused', 'general'):                                   # warm-up: code objects, tables, the workspace
        out[form] = ops.resample_u8(src, (H, W), form=form)
    torch.cuda.synchronize()
    assert torch.equal(out['fused'], out['general'])
    if args.once:
        for _ in range(3):
            for form in ('fused', 'general'):
                ops.resample_u8(src, (H, W), form=form)
        torch.cuda.synchronize()
        return
    lib = _lib.load()
    ws = lib.dbw_images_resample_workspace_bytes(N, Hin, Win, H, W)
    raw_b, out_b = N * Hin * Win * 3, N * 3 * H * W * 4
    moved = {'fused': raw_b + out_b, 'general': raw_b + ws + ws + out_b}   # general: the intermediate is written once and read once
    times = {'fused': [], 'general': []}
    for _ in range(args.reps):
        for form in ('fused', 'general'):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.resample_u8(src, (H, W), form=form)
            b.record()
            b.synchronize()
            times[form].append(a.elapsed_time(b) * 1e-3)
    res = {'views': N, 'raw': [Hin, Win], 'img_size': [H, W], 'reps': args.reps}
    for form in ('fused', 'general'):
        t = float(np.median(times[form]))
        res[form] = {'median_ms': round(t * 1e3, 4), 'min_ms': round(min(times[form]) * 1e3, 4), 'max_ms': round(max(times[form]) * 1e3, 4),
                     'bytes_moved': moved[form], 'GB_per_s': round(moved[form] / t / 1e9, 1), 'share_of_hbm_peak': round(moved[form] / t / HBM_PEAK, 4)}
    ups = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pinned.to(dev, non_blocking=True)
        torch.cuda.synchronize()
        ups.append(time.perf_counter() - t0)
    res['pinned_upload_ms'] = round(float(np.median(ups)) * 1e3, 2)
    if not args.no_host:
        from PIL import Image
        with tempfile.TemporaryDirectory(dir=args.tmp) as d:
            paths = []
            for i in range(N):
                paths.append(os.path.join(d, f'{i:06d}.png'))
                Image.fromarray(frames[i], 'RGB').save(paths[-1], compress_level=1)
            res['png_bytes_per_frame'] = os.path.getsize(paths[0])
            decode = lambda p: np.array(Image.open(p).convert('RGB'))
            t0 = time.perf_counter()
            decoded = [decode(p) for p in paths]
            res['pil_decode_s_serial'] = round(time.perf_counter() - t0, 3)
            with ThreadPoolExecutor(16) as pool:
                t0 = time.perf_counter()
                list(pool.map(decode, paths))
                res['pil_decode_s_16_threads'] = round(time.perf_counter() - t0, 3)
                imgs = [Image.fromarray(a, 'RGB') for a in decoded]
                resize = lambda im: np.array(im.resize((W, H), Image.BILINEAR))
                t0 = time.perf_counter()
                small = list(pool.map(resize, imgs))
                res['pil_resize_s_16_threads'] = round(time.perf_counter() - t0, 3)
            t0 = time.perf_counter()
            small = [resize(im) for im in imgs]
            res['pil_resize_s_serial'] = round(time.perf_counter() - t0, 3)
            got = ops.resample_u8(src, (H, W), out='u8').cpu().numpy()
            res['bytes_differing_from_pillow'] = int((got != np.stack(small)).sum())
    print(json.dumps(res))


if __name__ == '__main__':
    main()
