"""Times the masked image terms (csrc/masked_loss.hip, csrc/ssim_term.hip) on the GPU beside what they replace, and a masked training step beside an unmasked one.

  kernels  at 4 x 3 x 300 x 400 (`--batch`), seeded inputs, a mask with a lens-like border and 30 % holes:
             masked_composite_fwd_bwd   dbw_monitor_masked_composite forward (rec + value) and its one-launch backward fed by an upstream
                                        scalar and a gradient for rec
             replaced_fwd_bwd           what the unmasked path runs for the same: dbw_composite_mse forward (value) and backward,
                                        ops.composite forward (rec) and its elementwise torch backward, and the sum of the two gradients
             masked_ssim_term           dbw_monitor_masked_ssim_term, value + gradient, with that mask and with a mask of ones
             plain_ssim_term            dbw_monitor_ssim_term, value + gradient
           `inner` calls between two device synchronisations per repeat, the legs alternated, the median and the spread over `--repeats`.
           Bytes: the planes each leg must move, computed from the shapes, over the median time.
  step     the four-view autograd step (ShardedTrainStep(use_c_step=False, use_native=False)) of bench.py's workload with the SSIM term,
           with a batch that carries masks (and its mask_sum) and without, alternated.
One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'differentiable-blocksworld_amd'))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
from dbw_amd import _lib, metrics, ops                           # noqa: E402


def timed(fn, inner):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / inner


def spread(ts):
    return {'median_us': statistics.median(ts) * 1e6, 'min_us': min(ts) * 1e6, 'max_us': max(ts) * 1e6}


def make_mask(N, H, W, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    y = (torch.arange(H).float() + 0.5) / H * 2 - 1
    x = (torch.arange(W).float() + 0.5) / W * 2 - 1
    ring = ((y[:, None] / 0.95) ** 2 + (x[None, :] / 0.9) ** 2 <= 1).float()
    return (ring * (torch.rand(N, 1, H, W, generator=g) >= 0.3).float()).contiguous().to(dev)


def bench_kernels(dev, N, H, W, repeats, inner):
    g = torch.Generator().manual_seed(N)
    fg, env = torch.rand(N, 4, H, W, generator=g).to(dev), torch.rand(N, 4, H, W, generator=g).to(dev)
    imgs = torch.rand(N, 3, H, W, generator=g).to(dev)
    x = (1e-3 * torch.randn(N, 3, H, W, generator=g)).to(dev)
    up = torch.ones(1, device=dev)
    m, ones = make_mask(N, H, W, dev), torch.ones(N, 1, H, W, device=dev)
    count, full = ops.mask_count(m), float(imgs.numel())
    a = imgs
    b = (a + 0.1 * torch.randn(N, 3, H, W, generator=g).to(dev)).clamp(0, 1).contiguous()
    p = lambda t: t.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def masked_composite():
        ops.masked_composite_fwd(fg, env, imgs, m, 1.0 / count)
        return ops.masked_composite_bwd(fg, env, imgs, m, 1.0 / count, up, x)

    def replaced():
        loss = torch.zeros(1, device=dev)
        _lib.call('dbw_composite_mse', p(fg), p(env), p(imgs), N, H, W, 1.0 / full, 0, 0, p(loss), 0, 0, stream)
        rec = torch.empty(N, 3, H, W, device=dev)
        _lib.call('dbw_composite_mse', p(fg), p(env), 0, N, H, W, 0.0, 0, p(rec), 0, 0, 0, stream)
        g_fg, g_env = torch.empty_like(fg), torch.empty_like(env)
        _lib.call('dbw_composite_mse', p(fg), p(env), p(imgs), N, H, W, 1.0 / full, p(up), 0, 0, p(g_fg), p(g_env), stream)
        mask = fg[:, 3:4]                                        # ops._Composite.backward, and autograd's sum of the two gradients
        g_fg2 = torch.cat([x * mask, (x * (fg[:, :3] - env[:, :3])).sum(1, keepdim=True)], 1)
        g_env2 = torch.cat([x * (1 - mask), torch.zeros_like(mask)], 1)
        return g_fg + g_fg2, g_env + g_env2

    legs = {'masked_composite_fwd_bwd': masked_composite, 'replaced_fwd_bwd': replaced,
            'masked_ssim_term': lambda: ops.masked_ssim_term_value_grad(a, b, m, count),
            'masked_ssim_term_ones': lambda: ops.masked_ssim_term_value_grad(a, b, ones, full),
            'plain_ssim_term': lambda: ops.ssim_term_value_grad(a, b)}
    for fn in legs.values():
        for _ in range(5):
            fn()
    ts = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            ts[k].append(timed(fn, inner))
    plane = N * H * W * 4
    # planes: forward fg 4, env rgb 3, imgs 3, masks 1 in, rec 3 out; backward the same 11 and grad_rec 3 in, 8 out
    moved = {'masked_composite_fwd_bwd': (11 + 3) * plane + (11 + 3 + 8) * plane,
             'masked_ssim_term': (3 + 3 + 1 + 3) * plane, 'masked_ssim_term_ones': (3 + 3 + 1 + 3) * plane, 'plain_ssim_term': 9 * plane}
    out = {'what': 'masked image terms alone', 'shape': [N, 3, H, W], 'valid_share': count / full, 'inner': inner, 'repeats': repeats}
    for k in legs:
        out[k] = spread(ts[k])
        if k in moved:
            out[k]['bytes_moved'] = moved[k]
            out[k]['GB_per_s'] = moved[k] / statistics.median(ts[k]) / 1e9
    # the same results: a mask of ones is the plain term, the masked composite with ones is the unmasked pair
    v1, g1 = ops.masked_ssim_term_value_grad(a, b, ones, full)
    v0, g0 = ops.ssim_term_value_grad(a, b)
    out['ones_equals_plain_bits'] = bool(torch.equal(g1, g0) and torch.equal(v1, v0))
    ops.masked_composite_fwd(fg, env, imgs, ones, 1.0 / full)
    gm, em = ops.masked_composite_bwd(fg, env, imgs, ones, 1.0 / full, up, x)
    gr, er = replaced()
    out['composite_ones_max_rel_diff_to_replaced'] = max(((gm - gr).abs().max() / gr.abs().max()).item(), ((em - er).abs().max() / er.abs().max()).item())
    return out


def bench_step(dev, views, repeats, steps, warmup):
    import bench
    from dbw_amd.parallel import ShardedTrainStep

    class A:
        pass
    a = A()
    a.views, a.H, a.W, a.blocks, a.fpp, a.txt = views, 300, 400, 10, 10, 256

    def make(masked):
        model, inp = bench.build_workload(a, dev)
        lw = {'rgb': model.loss_weights['rgb'], 'perceptual': 0.1}
        lw.update({k: v for k, v in model.loss_weights.items() if k != 'rgb'})
        model.loss_weights = lw
        model.set_perceptual(metrics.SSIMTerm())
        model.sync_free = True
        step = ShardedTrainStep(model, lr=5e-3, lr_texture=5e-2, seed=227391, use_c_step=False, use_native=False)
        if masked:
            inp = dict(inp, masks=make_mask(views, a.H, a.W, dev))
            inp['mask_sum'] = float(inp['masks'].sum(dtype=torch.float64))
        return step, inp
    legs = {'masked': make(True), 'unmasked': make(False)}
    vals = {}

    def one(k):
        step, inp = legs[k]
        vals[k] = {n: float(v) for n, v in step(inp).items()}        # (the loss values read every step, as the reference's trainer does)
    for k in legs:
        for _ in range(warmup):
            one(k)
    ts = {k: [] for k in legs}
    for _ in range(repeats):
        for k in legs:
            ts[k].append(timed(lambda: one(k), steps))
    diff = [x - y for x, y in zip(ts['masked'], ts['unmasked'])]
    out = {'what': f'{views}-view autograd step (use_c_step=False, use_native=False), 300x400, 10 blocks, faces_per_pixel=10, 256^2 textures, SSIM term, '
                   'loss values read every step', 'steps_per_repeat': steps, 'repeats': repeats,
           'valid_share': legs['masked'][1]['mask_sum'] / (views * 300 * 400)}
    for k in legs:
        s = spread(ts[k])
        out[k] = {'median_ms': s['median_us'] / 1e3, 'min_ms': s['min_us'] / 1e3, 'max_ms': s['max_us'] / 1e3,
                  'losses': {n: round(v, 6) for n, v in vals[k].items()}}
    out['masked_minus_unmasked_ms'] = {'median': statistics.median(diff) * 1e3, 'min': min(diff) * 1e3, 'max': max(diff) * 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=['kernels', 'step'], default=None)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--inner', type=int, default=300)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    dev = torch.device('cuda:0')
    if args.only != 'step':
        print(json.dumps(bench_kernels(dev, args.batch, 300, 400, args.repeats, args.inner)), flush=True)
    if args.only != 'kernels':
        print(json.dumps(bench_step(dev, 4, args.repeats, args.steps, args.warmup)), flush=True)


if __name__ == '__main__':
    main()
