"""Times the plane RANSAC at N points x H hypotheses on a seeded cloud (60 % on a noisy tilted ground, the rest in a blob).

Two paths on the same device tensors, alternated `--repeats` times each after one warm-up of both, wall clock between device
synchronisations around `inner` calls (so that a timed window is tens of milliseconds at every size):
  hip     eval3d.plane_ransac (dbw_eval_plane_fit: hypotheses, scoring, best, two refinement rounds, final count; one call, no host read)
  torch   eval3d.plane_ransac_torch in fp32 (hypotheses on the host, scoring in chunks of hypotheses of at most 2^24 residuals, argmax
          and refinement in torch, one host read for the best index): what a user could write without the kernel
Prints one JSON line per size.  `--path hip` / `--path torch` runs only that path (a warm-up and `inner` calls) at the first size, for a
kernel trace of it (rocprofv3 --kernel-trace --stats -- python tools/plane_bench.py --path hip --points 10000000)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'differentiable-blocksworld_amd'))
from dbw_amd import eval3d                                       # noqa: E402


def cloud(N, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    xy = torch.rand(N, 2, generator=gen, device=dev) * 2 - 1
    ground = 0.2 * xy[:, 0] - 0.1 * xy[:, 1] + 0.05 + 0.004 * torch.randn(N, generator=gen, device=dev)
    blob = torch.rand(N, generator=gen, device=dev) * 1.5 - 0.5
    z = torch.where(torch.rand(N, generator=gen, device=dev) < 0.6, ground, blob)
    cams = torch.tensor([0.0, 0.0, 1.5], device=dev) + 0.3 * torch.randn(8, 3, generator=gen, device=dev)
    return torch.cat([xy, z[:, None]], 1).contiguous(), cams


def timed(fn, inner):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(inner):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / inner, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, nargs='+', default=[100_000, 1_000_000, 10_000_000])
    ap.add_argument('--hyp', type=int, default=512)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--path', choices=['both', 'hip', 'torch'], default='both')
    args = ap.parse_args()
    dev = torch.device('cuda')
    for N in args.points if args.path == 'both' else args.points[:1]:
        pts, cams = cloud(N, dev)
        kw = dict(n_hyp=args.hyp, thresh=0.02, up=[0.0, 0.0, 1.0], cams=cams, refine=2, seed=1, return_counts=True)
        paths = {'hip': lambda: eval3d.plane_ransac(pts, **kw), 'torch': lambda: eval3d.plane_ransac_torch(pts, **kw)}
        names = list(paths) if args.path == 'both' else [args.path]
        inner = {'hip': max(2, 20_000_000 // N), 'torch': max(1, 2_000_000 // N)}
        for name in names:                                       # warm-up: library load, allocator, first launches
            timed(paths[name], 1)
        times, outs = {n: [] for n in names}, {}
        for _ in range(args.repeats if args.path == 'both' else 1):
            for name in names:
                t, outs[name] = timed(paths[name], inner[name])
                times[name].append(t)
        res = {'points': N, 'hyp': args.hyp, 'tests': N * args.hyp, 'device': torch.cuda.get_device_name(0), 'inner_calls': {n: inner[n] for n in names}}
        for name in names:
            ts = sorted(times[name])
            res[name] = {'runs_ms': [round(t * 1e3, 4) for t in times[name]], 'median_ms': ts[len(ts) // 2] * 1e3, 'min_ms': ts[0] * 1e3,
                         'max_ms': ts[-1] * 1e3, 'tests_per_s_whole_call': N * args.hyp / ts[len(ts) // 2]}
        if len(names) == 2:
            a, b = outs['hip'], outs['torch']
            res['torch_over_hip'] = res['torch']['median_ms'] / res['hip']['median_ms']
            res['same_counts'] = bool(torch.equal(a.counts, b.counts))
            res['same_best'] = int(a.best) == int(b.best)
            res['n_inliers'] = [int(a.n_inliers), int(b.n_inliers)]
            res['largest_plane_difference'] = float(torch.cat([a.normal - b.normal, (a.offset - b.offset)[None]]).abs().max())
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
