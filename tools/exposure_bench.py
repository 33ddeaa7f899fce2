"""Times the exposure compensation (csrc/exposure_loss.hip) on the GPU beside the masked composite it is modelled on, and a training step
with the option on beside the same step under all-ones masks (the same layers path without theta).

  kernels  at 4 x 3 x 300 x 400 (`--batch`), seeded inputs, all-ones masks, theta random in +-0.3:
             exposure_bwd / masked_bwd           the backward alone: dbw_monitor_exposure_composite (image launch + finishing launch) and
                                                 dbw_monitor_masked_composite (one launch), upstream scalar and a gradient for rec
             exposure_fwd_bwd / masked_fwd_bwd   forward (rec + value) and backward
           `inner` calls between two device synchronisations per repeat, the legs alternated, the median and the spread over `--repeats`.
           Bytes: the planes each leg must move, computed from the shapes, over the median time.
  step     the four-view autograd step of configs/custom_exposure.yml's model (10 blocks, 10 faces per pixel, 64^2 textures, SSIM term;
           300 x 400) with a batch that carries `exposure` -- the refiner's Adam step and centring included -- and with a batch that
           carries all-ones masks instead, alternated.
  ones_masks  (`--only ones_masks`) the all-ones-masks leg alone.  With DBW_BENCH_ROOT=<a checkout of another commit, built> the package,
           bench.py and the library are taken from that tree: a process per tree, so that this tree and its parent can be alternated.
One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.environ.get('DBW_BENCH_ROOT') or os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'differentiable-blocksworld_amd'))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
from dbw_amd import metrics, ops                                 # noqa: E402


def timed(fn, inner):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / inner


def spread(ts):
    return {'median_us': statistics.median(ts) * 1e6, 'min_us': min(ts) * 1e6, 'max_us': max(ts) * 1e6}


def bench_kernels(dev, N, H, W, repeats, inner):
    g = torch.Generator().manual_seed(N)
    fg, env = torch.rand(N, 4, H, W, generator=g).to(dev), torch.rand(N, 4, H, W, generator=g).to(dev)
    imgs = torch.rand(N, 3, H, W, generator=g).to(dev)
    x = (1e-3 * torch.randn(N, 3, H, W, generator=g)).to(dev)
    theta = ((torch.rand(N + 3, 6, generator=g) - 0.5) * 0.6).to(dev)
    ids = torch.randperm(N + 3, generator=g)[:N].to(torch.int32).to(dev)
    up, ones = torch.ones(1, device=dev), torch.ones(N, 1, H, W, device=dev)
    scale = 1.0 / imgs.numel()
    table = torch.zeros_like(theta)

    def exposure_bwd():
        return ops.exposure_composite_bwd(fg, env, imgs, ones, theta, ids, scale, up, x, grad_theta=table)

    def masked_bwd():
        return ops.masked_composite_bwd(fg, env, imgs, ones, scale, up, x)

    def exposure_pair():
        ops.exposure_composite_fwd(fg, env, imgs, ones, theta, ids, scale)
        return exposure_bwd()

    def masked_pair():
        ops.masked_composite_fwd(fg, env, imgs, ones, scale)
        return masked_bwd()

    legs = {'exposure_bwd': exposure_bwd, 'masked_bwd': masked_bwd, 'exposure_fwd_bwd': exposure_pair, 'masked_fwd_bwd': masked_pair}
    for fn in legs.values():
        for _ in range(5):
            fn()
    ts = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            ts[k].append(timed(fn, inner))
    plane = N * H * W * 4
    # planes: forward fg 4, env rgb 3, imgs 3, masks 1 in, rec 3 out; backward the same 11 and grad_rec 3 in, 8 out
    moved = {'exposure_bwd': (11 + 3 + 8) * plane, 'masked_bwd': (11 + 3 + 8) * plane, 'exposure_fwd_bwd': (14 + 22) * plane,
             'masked_fwd_bwd': (14 + 22) * plane}
    out = {'what': 'exposure composite beside the masked composite', 'shape': [N, 3, H, W], 'inner': inner, 'repeats': repeats}
    for k in legs:
        out[k] = spread(ts[k])
        out[k]['bytes_moved'] = moved[k]
        out[k]['GB_per_s'] = moved[k] / statistics.median(ts[k]) / 1e9
    diff = [a - b for a, b in zip(ts['exposure_bwd'], ts['masked_bwd'])]
    out['exposure_bwd_minus_masked_bwd_us'] = {'median': statistics.median(diff) * 1e6, 'min': min(diff) * 1e6, 'max': max(diff) * 1e6}
    # the same results: theta = 0 is the masked composite bit for bit
    zero = torch.zeros_like(theta)
    g0, e0, _ = ops.exposure_composite_bwd(fg, env, imgs, ones, zero, ids, scale, up, x)
    gm, em = masked_bwd()
    out['zero_theta_equals_masked_bits'] = bool(torch.equal(g0, gm) and torch.equal(e0, em))
    return out


def bench_step(dev, views, repeats, steps, warmup, legs=('exposure', 'ones_masks')):
    import bench
    from dbw_amd.parallel import ShardedTrainStep

    class A:
        pass
    a = A()
    a.views, a.H, a.W, a.blocks, a.fpp, a.txt = views, 300, 400, 10, 10, 64

    def make(exposed):
        model, inp = bench.build_workload(a, dev)
        lw = {'rgb': model.loss_weights['rgb'], 'perceptual': 0.1}
        lw.update({k: v for k, v in model.loss_weights.items() if k != 'rgb'})
        model.loss_weights = lw
        model.set_perceptual(metrics.SSIMTerm())
        model.sync_free = True
        step = ShardedTrainStep(model, lr=5e-3, lr_texture=5e-2, seed=227391, use_c_step=False, use_native=False)
        refiner = None
        if exposed:
            from dbw_amd.exposure import ExposureRefiner
            refiner = ExposureRefiner(views, dev, lr=1e-3)
            ids = torch.arange(views, device=dev)
            inp = refiner.attach(dict(inp, view_ids=ids, view_ids_host=list(range(views))))
        else:
            inp = dict(inp, masks=torch.ones(views, 1, a.H, a.W, device=dev), mask_sum=float(views * a.H * a.W))
        return step, inp, refiner
    legs = {k: make(k == 'exposure') for k in legs}
    vals = {}

    def one(k):
        step, inp, refiner = legs[k]
        vals[k] = {n: float(v) for n, v in step(inp).items()}        # (the loss values read every step, as the reference's trainer does)
        if refiner is not None:
            refiner.step()
    for k in legs:
        for _ in range(warmup):
            one(k)
    ts = {k: [] for k in legs}
    for _ in range(repeats):
        for k in legs:
            ts[k].append(timed(lambda: one(k), steps))
    out = {'tree': os.path.abspath(ROOT), 'what': f'{views}-view autograd step (use_c_step=False, use_native=False), 300x400, 10 blocks, faces_per_pixel=10, 64^2 textures, SSIM term, '
                   'loss values read every step', 'steps_per_repeat': steps, 'repeats': repeats}
    for k in legs:
        s = spread(ts[k])
        out[k] = {'median_ms': s['median_us'] / 1e3, 'min_ms': s['min_us'] / 1e3, 'max_ms': s['max_us'] / 1e3,
                  'losses': {n: round(v, 6) for n, v in vals[k].items()}}
    if len(legs) == 2:
        diff = [x - y for x, y in zip(ts['exposure'], ts['ones_masks'])]
        out['exposure_minus_ones_masks_ms'] = {'median': statistics.median(diff) * 1e3, 'min': min(diff) * 1e3, 'max': max(diff) * 1e3}
        out['theta_abs_max'] = float(legs['exposure'][2].flat.abs().max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=['kernels', 'step', 'ones_masks'], default=None)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--inner', type=int, default=300)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    dev = torch.device('cuda:0')
    if args.only == 'ones_masks':
        print(json.dumps(bench_step(dev, 4, args.repeats, args.steps, args.warmup, legs=('ones_masks',))), flush=True)
        return
    if args.only != 'step':
        print(json.dumps(bench_kernels(dev, args.batch, 300, 400, args.repeats, args.inner)), flush=True)
    if args.only != 'kernels':
        print(json.dumps(bench_step(dev, 4, args.repeats, args.steps, args.warmup)), flush=True)


if __name__ == '__main__':
    main()
