"""Times the k-means / PCA fit at N points x K centres x n_iter rounds on a seeded cloud of Gaussian blobs.

Two paths on the same device tensor, alternated `--repeats` times each after one warm-up of both, wall clock between device
synchronisations around `inner` calls (so that a timed window is tens of milliseconds at least):
  hip     eval3d.cluster_points (dbw_eval_cluster_fit: seeding, n_iter rounds, the final pass; one call, no host read)
  torch   eval3d.cluster_points_torch on the device (the same algorithm in torch ops, distances in chunks of 65536 points): what a user
          could write without the kernel
`--given-init` starts both from the same K centres (the hip path's seeding), which takes the seeding out of both.  Prints one JSON line per
size.  `--path hip` / `--path torch` runs only that path (a warm-up and `inner` calls), for a kernel trace of it
(rocprofv3 --kernel-trace --stats -- python tools/cluster_bench.py --path hip)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'differentiable-blocksworld_amd'))
from dbw_amd import eval3d                                       # noqa: E402


def cloud(N, dev, n_blobs=40):
    gen = torch.Generator(device=dev).manual_seed(0)
    centres = torch.rand(n_blobs, 3, generator=gen, device=dev) * 4 - 2
    which = torch.randint(0, n_blobs, (N,), generator=gen, device=dev)
    scale = torch.rand(n_blobs, 1, generator=gen, device=dev) * 0.3 + 0.05
    return (centres[which] + torch.randn(N, 3, generator=gen, device=dev) * scale[which]).contiguous()


def timed(fn, inner):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(inner):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / inner, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, nargs='+', default=[1_000_000])
    ap.add_argument('--k', type=int, default=64)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--given-init', action='store_true')
    ap.add_argument('--path', choices=['both', 'hip', 'torch'], default='both')
    args = ap.parse_args()
    dev = torch.device('cuda')
    for N in args.points if args.path == 'both' else args.points[:1]:
        pts = cloud(N, dev)
        init = eval3d.cluster_points(pts, args.k, n_iter=0).centres.clone() if args.given_init else None
        kw = dict(n_iter=args.iters, init=init)
        paths = {'hip': lambda: eval3d.cluster_points(pts, args.k, **kw), 'torch': lambda: eval3d.cluster_points_torch(pts, args.k, **kw)}
        names = list(paths) if args.path == 'both' else [args.path]
        inner = {'hip': max(2, 20_000_000 // N), 'torch': max(1, 2_000_000 // N)}
        for name in names:                                       # warm-up: library load, allocator, first launches
            timed(paths[name], 1)
        times, outs = {n: [] for n in names}, {}
        for _ in range(args.repeats if args.path == 'both' else 1):
            for name in names:
                t, outs[name] = timed(paths[name], inner[name])
                times[name].append(t)
        tests = N * args.k * (args.iters + 1)
        res = {'points': N, 'k': args.k, 'iters': args.iters, 'given_init': args.given_init, 'distance_tests': tests,
               'device': torch.cuda.get_device_name(0), 'inner_calls': {n: inner[n] for n in names}}
        for name in names:
            ts = sorted(times[name])
            res[name] = {'runs_ms': [round(t * 1e3, 4) for t in times[name]], 'median_ms': ts[len(ts) // 2] * 1e3, 'min_ms': ts[0] * 1e3,
                         'max_ms': ts[-1] * 1e3, 'distance_tests_per_s_whole_call': tests / ts[len(ts) // 2]}
        if len(names) == 2:
            a, b = outs['hip'], outs['torch']
            res['torch_over_hip'] = res['torch']['median_ms'] / res['hip']['median_ms']
            res['labels_that_differ'] = int((a.labels != b.labels).sum())
            res['largest_centre_difference'] = float((a.centres - b.centres).abs().max())
            res['n_nonempty'] = [int(a.n_nonempty), int(b.n_nonempty)]
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
