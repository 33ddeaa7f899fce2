"""Measurement helper of the 3D evaluation (dbw_amd/eval3d.py, csrc/nn_search.hip); results go to profiles/eval3d.md.

    python tools/nn_bench.py [--points 500000] [--reps 5] [--skip-dtu]

  * exact nearest neighbours at P x P in both directions (the Chamfer-L1 of mbf_eval.py: 5e5 samples against 5e5 ground-truth points):
    pairs/s from device events, the VALU instructions per pair counted in the ISA of the search loop (hipcc --save-temps of
    csrc/nn_search.hip, the basic block with the packed fp32 arithmetic; a v_pk_*_f32 counts twice, it issues in two passes), the issue
    bound 256 CUs x 4 SIMD x 32 lanes x 2.4 GHz =
    78.6 T lane-instructions/s over that count, and the fraction of it reached;
  * wall time of eval3d.dtu_scores on a synthetic scene of DTU size (~5e6 lattice points, 2.5e6 stl points), per stage;
  * the rounds of the radius downsample.
Prints one JSON line."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time
from collections import Counter

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'differentiable-blocksworld_amd'))
from dbw_amd import eval3d  # noqa: E402

ISSUE_BOUND = 256 * 4 * 32 * 2.4e9          # lane-instructions/s
NN_Q = 8                                     # queries per lane (csrc/nn_search.hip)


def valu_per_pair():
    """VALU instructions per (query, y) pair in the unrolled search loop of nn_search_kernel, counted in the gfx950 ISA"""
    src = os.path.join(ROOT, 'differentiable-blocksworld_amd', 'csrc', 'nn_search.hip')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    with tempfile.TemporaryDirectory() as d:
        subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-fno-gpu-flush-denormals-to-zero',
                               '--cuda-device-only', '-S', src, '-o', os.path.join(d, 'nn.s')], stderr=subprocess.DEVNULL)
        asm = open(os.path.join(d, 'nn.s')).read()
    body = asm[asm.index('nn_search_kernel'):]
    body = body[:body.index('s_endpgm')]
    best = None
    for blk in re.split(r'\n\.LBB\w+:', body):
        ops = Counter(ln.split()[0] for ln in blk.split('\n') if ln.strip() and not ln.strip().startswith(('.', ';')))
        pk = sum(v for k, v in ops.items() if k.startswith('v_pk_'))
        if best is None or pk > best[0]:
            best = (pk, ops)
    ops = best[1]
    # a packed fp32 instruction (v_pk_add/mul/fma_f32) issues in two passes: 64 FLOP/clk/SIMD for v_pk_fma_f32, the same as v_fma_f32
    # (MI355X vector peak 157.3 TF), so it costs two lane-instruction slots of the bound
    valu = sum(v * (2 if k.startswith('v_pk_') and k.endswith('_f32') else 1) for k, v in ops.items() if k.startswith('v_'))
    y_per_block = sum(v for k, v in ops.items() if k.startswith('ds_read'))
    pairs = y_per_block * NN_Q
    return valu / pairs, dict(ops), pairs


def time_nn(P, reps):
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.rand(1, P, 3, device='cuda', generator=g) * 100
    y = torch.rand(1, P, 3, device='cuda', generator=g) * 100
    for _ in range(2):
        eval3d.nn_points(x, y)
        eval3d.nn_points(y, x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        eval3d.nn_points(x, y)
        eval3d.nn_points(y, x)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    return ms, 2.0 * P * P / (ms * 1e-3)


def dtu_scene(rng, n_boxes=22, side=40.0, n_stl=2_500_000):
    box_f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                      [1, 5, 7], [1, 7, 3]])
    verts, faces = [], []
    for b in range(n_boxes):
        q = rng.standard_normal(4)
        q /= np.linalg.norm(q)
        a, bq, c, d = q
        R = np.array([[a * a + bq * bq - c * c - d * d, 2 * (bq * c - a * d), 2 * (bq * d + a * c)],
                      [2 * (bq * c + a * d), a * a - bq * bq + c * c - d * d, 2 * (c * d - a * bq)],
                      [2 * (bq * d - a * c), 2 * (c * d + a * bq), a * a - bq * bq - c * c + d * d]])
        corners = np.array([[i, j, k] for i in (-.5, .5) for j in (-.5, .5) for k in (-.5, .5)]) * side * rng.uniform(0.8, 1.2, 3)
        verts.append(corners @ R.T + rng.uniform(-150, 150, 3))
        faces.append(box_f + 8 * b)
    V = np.concatenate(verts).astype(np.float32)
    F_ = np.concatenate(faces)
    k = rng.integers(0, len(F_), n_stl)
    fv = V[F_[k]].astype(np.float64)
    su, w = np.sqrt(rng.random(n_stl)), rng.random(n_stl)
    stl = (1 - su)[:, None] * fv[:, 0] + (su * (1 - w))[:, None] * fv[:, 1] + (su * w)[:, None] * fv[:, 2] + rng.normal(0, 0.5, (n_stl, 3))
    BB = np.array([[-200., -200., -200.], [200., 200., 200.]])
    obs = np.ones((101, 101, 101), np.uint8)
    plane = np.array([[0.], [0.], [1.], [180.]])
    return V, F_, obs, BB, np.array([[4.0]]), plane, stl


def time_dtu(rng):
    V, F_, obs, BB, res, plane, stl = dtu_scene(rng)
    eval3d.dtu_scores(V[:24], F_[:24], obs, BB, res, plane, stl[:1000], seed=0)          # warm-up: code objects, allocator
    torch.cuda.synchronize()
    stages = {}
    t0 = time.perf_counter()
    pcd, counts = eval3d.dense_lattice(torch.from_numpy(V).cuda(), torch.from_numpy(F_).cuda())
    torch.cuda.synchronize()
    stages['lattice_s'] = time.perf_counter() - t0
    order = torch.from_numpy(np.random.default_rng(0).permutation(pcd.shape[0])).cuda()
    t1 = time.perf_counter()
    keep, rounds = eval3d.radius_downsample(pcd[order].contiguous())
    torch.cuda.synchronize()
    stages['downsample_s'] = time.perf_counter() - t1
    t2 = time.perf_counter()
    s = eval3d.dtu_scores(V, F_, obs, BB, res, plane, stl, seed=0)
    torch.cuda.synchronize()
    total = time.perf_counter() - t2
    return dict(dtu_total_s=round(total, 3), **{k: round(v, 3) for k, v in stages.items()}, n_lattice=s['n_lattice'], n_points=s['n_points'],
                n_down=s['n_down'], n_stl=len(stl), n_in_obs=s['n_in_obs'], n_stl_above=s['n_stl_above'], rounds=s['rounds'],
                rounds_standalone=rounds, acc=s['acc'], comp=s['comp'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=500_000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip-dtu', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'nn_bench measures on the GPU'
    vpp, ops, pairs = valu_per_pair()
    ms, pps = time_nn(a.points, a.reps)
    bound = ISSUE_BOUND / vpp
    out = dict(nn_points=a.points, nn_both_directions_ms=round(ms, 3), nn_pairs_per_s=pps, valu_per_pair=vpp, isa_block_pairs=pairs,
               isa_block_ops=ops, issue_bound_pairs_per_s=bound, fraction_of_bound=round(pps / bound, 3))
    if not a.skip_dtu:
        out.update(time_dtu(np.random.default_rng(1)))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
