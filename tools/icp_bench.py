"""Times the gradient ICP at the evaluator's sizes: N = 1, 100 000 x 100 000 points, n_iter = 100, anisotropic scale.

Two paths on the same device tensors, alternated `--repeats` times each after one warm-up of both, wall clock between device
synchronisations:
  one_call     eval3d.gradient_icp (dbw_icp_run: the whole loop enqueued by one call)
  torch_loop   eval3d.gradient_icp_torch (chamfer_distance on dbw_nn_points, autograd, torch.optim.Adam, a host read per iteration):
               the best a user could write before the one-call path existed
Prints one JSON line.  `--path one_call` / `--path torch_loop` runs only that path once after a warm-up, for a kernel trace of it
(rocprofv3 --kernel-trace --stats -- python tools/icp_bench.py --path one_call)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'differentiable-blocksworld_amd'))
from dbw_amd import eval3d, mesh                                 # noqa: E402

PAIRS_PER_S = 7.2e12                                             # DESIGN.md 6c, measured at 500k x 500k


def clouds(P, dev):
    gen = torch.Generator().manual_seed(0)
    g = torch.randn(1, 2 * P, 3, generator=gen)
    g = g / g.norm(dim=2, keepdim=True) * torch.tensor([0.5, 0.35, 0.25]) + 0.01 * torch.randn(1, 2 * P, 3, generator=gen)
    R = mesh.rotation_6d_to_matrix(torch.tensor([[1., 0.15, -0.1, -0.1, 1., 0.2]]))
    return ((g[:, P:] - torch.tensor([0.03, -0.02, 0.04])) @ R.transpose(1, 2) / 1.1).to(dev).contiguous(), g[:, :P].to(dev).contiguous()


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=100_000)
    ap.add_argument('--n-iter', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--path', choices=['both', 'one_call', 'torch_loop'], default='both')
    args = ap.parse_args()
    dev = torch.device('cuda')
    pp, pg = clouds(args.points, dev)
    paths = {'one_call': lambda: eval3d.gradient_icp(pp, pg, True, True, lr=0.01, n_iter=args.n_iter),
             'torch_loop': lambda: eval3d.gradient_icp_torch(pp, pg, True, True, lr=0.01, n_iter=args.n_iter)}
    names = list(paths) if args.path == 'both' else [args.path]
    for name in names:                                           # warm-up: library load, allocator, first launches
        timed(paths[name])
    times, outs = {n: [] for n in names}, {}
    for _ in range(args.repeats if args.path == 'both' else 1):
        for name in names:
            t, outs[name] = timed(paths[name])
            times[name].append(t)
    res = {'points': args.points, 'n_iter': args.n_iter, 'device': torch.cuda.get_device_name(0),
           'expected_ms_per_iter_from_search_rate': 2.0 * args.points * args.points / PAIRS_PER_S * 1e3}
    for name in names:
        ts = sorted(times[name])
        res[name] = {'runs_s': [round(t, 5) for t in times[name]], 'median_s': ts[len(ts) // 2], 'min_s': ts[0], 'max_s': ts[-1],
                     'ms_per_iter': ts[len(ts) // 2] / max(args.n_iter, 1) * 1e3}
    if len(names) == 2:
        res['torch_loop_over_one_call'] = res['torch_loop']['median_s'] / res['one_call']['median_s']
        a, b = outs['one_call'], outs['torch_loop']
        res['largest_difference'] = {k: float((x.double() - y.double()).abs().max()) for k, x, y in
                                     (('cloud', a[0], b[0]), ('R', a[1][0], b[1][0]), ('T', a[1][1], b[1][1]), ('s', a[1][2], b[1][2]))}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
