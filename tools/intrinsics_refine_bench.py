"""Times the intrinsics refinement (csrc/camera_grad.hip, dbw_amd/intrinsics.py) on the GPU.

  kernels  the blocks of bench.py's workload (`--blocks`, default 10 and 80: 800 / 6,400 faces, 1,600 / 12,800 clipped-face slots) seen from
           `--views` cameras (default 49: config 2), a random gradient on every slot:
             intrinsics_grad    dbw_lens_intrinsics_grad (camera_partials_kernel<KGradSink> + intrinsics_finish_kernel), workspace allocated once
             pose_grad          dbw_lens_pose_grad on the same inputs: the same per-slot work, summed per view
             project_clip_bwd   dbw_project_clip_bwd on the same inputs: the same per-slot work, summed over the views
             apply_chain        dbw_lens_intrinsics_apply + dbw_lens_intrinsics_chain
           `inner` calls between two device synchronisations per repeat, the legs alternated, the median and the spread over `--repeats`.
  step     the four-view autograd step (ShardedTrainStep(use_c_step=False, use_native=False)) of bench.py's workload with the SSIM term
           (the protocol of tools/pose_refine_bench.py), with IntrinsicsRefiner.apply before and IntrinsicsRefiner.step after it, and
           without.
One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'differentiable-blocksworld_amd'))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dbw_amd import _lib, intrinsics, metrics, ops               # noqa: E402
from masked_loss_bench import spread, timed                      # noqa: E402
from pose_refine_bench import Args                               # noqa: E402


def bench_kernels(dev, views, blocks, repeats, inner):
    import bench
    a = Args()
    a.views, a.blocks = views, blocks
    model, inp = bench.build_workload(a, dev)
    with torch.no_grad():
        model._ensure_cameras(inp)
        scene = model.build_blocks_scene(filter_transparent=False)
    verts, faces = scene.verts.contiguous(), scene.faces
    R, T = inp['R'].float().contiguous(), inp['T'].float().contiguous()
    Kmat = model.renderer.cameras.K[0].to(dev).contiguous()
    cfg = model.renderer._cfg(faces.shape[0])
    cl = ops.project_clip(verts, faces, R, T, Kmat, cfg.eps, cfg.z_clip, cfg.persp)
    B, V, F_ = R.shape[0], verts.shape[0], faces.shape[0]
    g = torch.randn(B, 2 * F_, 3, 3, generator=torch.Generator().manual_seed(0)).to(dev)
    lib = _lib.family('lens')
    ws_bytes = int(lib.dbw_lens_intrinsics_grad_workspace_bytes(B, F_))
    assert ws_bytes == int(lib.dbw_lens_pose_grad_workspace_bytes(B, F_))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    gR, gT, gv, gK = torch.empty(B, 3, 3, device=dev), torch.empty(B, 3, device=dev), torch.zeros_like(verts), torch.empty(4, 4, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    common = (p(verts), p(faces), p(R), p(T), p(Kmat), B, V, F_, float(cfg.eps), float(cfg.z_clip or 0.0), int(cfg.persp), p(cl['num_faces']), p(cl['c2o']),
              p(cl['clip_code']), p(cl['clip_w']), p(g))
    theta = torch.tensor([0.01, -0.01, 0.002, -0.003], device=dev)
    K1, gth = torch.empty_like(Kmat), torch.empty(4, device=dev)

    def apply_chain():
        _lib.call('dbw_lens_intrinsics_apply', p(Kmat), p(theta), p(K1), st)
        _lib.call('dbw_lens_intrinsics_chain', p(Kmat), p(theta), p(gK), p(gth), st)
    legs = {'intrinsics_grad': lambda: _lib.call('dbw_lens_intrinsics_grad', *common, p(ws), ws_bytes, p(gK), 0, st),
            'pose_grad': lambda: _lib.call('dbw_lens_pose_grad', *common, p(ws), ws_bytes, p(gR), p(gT), 0, st),
            'project_clip_bwd': lambda: _lib.call('dbw_project_clip_bwd', *common, p(gv), st),
            'apply_chain': apply_chain}
    ts = {k: [] for k in legs}
    for fn in legs.values():
        timed(fn, 20)
    for _ in range(repeats):
        for k, fn in legs.items():
            ts[k].append(timed(fn, inner))
    out = {'what': 'intrinsics kernels alone', 'views': B, 'faces': F_, 'slots': 2 * F_, 'clipped_faces_per_view': float(cl['num_faces'].float().mean()),
           'inner': inner, 'repeats': repeats, 'workspace_bytes': ws_bytes}
    for k in legs:
        out[k] = spread(ts[k])
    return out


def bench_step(dev, views, repeats, steps, warmup):
    import bench
    from dbw_amd.parallel import ShardedTrainStep
    a = Args()
    a.views, a.blocks = views, 10

    def make(refine):
        model, inp = bench.build_workload(a, dev)
        lw = {'rgb': model.loss_weights['rgb'], 'perceptual': 0.1}
        lw.update({k: v for k, v in model.loss_weights.items() if k != 'rgb'})
        model.loss_weights = lw
        model.set_perceptual(metrics.SSIMTerm())
        model.sync_free = True
        step = ShardedTrainStep(model, lr=5e-3, lr_texture=5e-2, seed=227391, use_c_step=False, use_native=False)
        ref = intrinsics.IntrinsicsRefiner(inp['K'][0], dev, lr=1e-4) if refine else None
        return step, inp, ref
    legs = {'refined': make(True), 'plain': make(False)}
    vals = {}

    def one(k):
        step, inp, ref = legs[k]
        losses = step(ref.apply(inp) if ref is not None else inp)
        if ref is not None:
            ref.step()
        vals[k] = {n: float(v) for n, v in losses.items()}          # (the loss values read every step, as the reference's trainer does)
    for k in legs:
        for _ in range(warmup):
            one(k)
    ts = {k: [] for k in legs}
    for _ in range(repeats):
        for k in legs:
            ts[k].append(timed(lambda: one(k), steps))
    diff = [x - y for x, y in zip(ts['refined'], ts['plain'])]
    out = {'what': f'{views}-view autograd step (use_c_step=False, use_native=False), 300x400, 10 blocks, faces_per_pixel=10, 256^2 textures, SSIM term, '
                   'loss values read every step', 'steps_per_repeat': steps, 'repeats': repeats}
    for k in legs:
        s = spread(ts[k])
        out[k] = {'median_ms': s['median_us'] / 1e3, 'min_ms': s['min_us'] / 1e3, 'max_ms': s['max_us'] / 1e3,
                  'losses': {n: round(v, 6) for n, v in vals[k].items()}}
    out['refined_minus_plain_ms'] = {'median': statistics.median(diff) * 1e3, 'min': min(diff) * 1e3, 'max': max(diff) * 1e3}
    out['theta'] = [float(v) for v in legs['refined'][2].flat.cpu().tolist()]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=['kernels', 'step'], default=None)
    ap.add_argument('--views', type=int, default=49)
    ap.add_argument('--blocks', type=int, nargs='+', default=[10, 80])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--inner', type=int, default=300)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    dev = torch.device('cuda:0')
    if args.only != 'step':
        for blocks in args.blocks:
            print(json.dumps(bench_kernels(dev, args.views, blocks, args.repeats, args.inner)), flush=True)
    if args.only != 'kernels':
        print(json.dumps(bench_step(dev, 4, args.repeats, args.steps, args.warmup)), flush=True)


if __name__ == '__main__':
    main()
