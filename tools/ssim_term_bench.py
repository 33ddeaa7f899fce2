"""Times the SSIM term (ops.ssim_term, csrc/ssim_term.hip) on the GPU and what it adds to a training step.

  term    value + gradient of the term alone on seeded images, at 4 x 3 x 300 x 400 and 49 x 3 x 300 x 400: `inner` calls between two device
          synchronisations per repeat (a timed window of tens of milliseconds), the median and the spread over `--repeats`; beside it the
          value alone (a null gradient) and the torch formula (metrics.ssim_map under autograd, fp32 on the same device) for context.
          Bytes: the 3 image planes the algorithm must move (read target and rec, write the gradient), over the time.
  step    the four-view one-call C step of BASELINE config 2's geometry (300 x 400, 10 blocks, 10 faces per pixel, 256^2 textures; bench.py's
          workload, the loss values read every step as the reference's trainer does) three ways, alternated `--repeats` times after a
          warm-up of all three: with the built-in SSIM term, with no perceptual term, and with LPIPSVGG(allow_random_init=True) (seeded
          weights: the cost is real, the values are not).  `added_ms` = with the term - without, median of the per-repeat differences.
One JSON line per measurement.  `--only term` / `--only step` runs one half (a kernel trace wants the first:
rocprofv3 --kernel-trace --stats -- python tools/ssim_term_bench.py --only term)."""
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


def bench_term(dev, N, H, W, repeats, inner):
    g = torch.Generator().manual_seed(N)
    a = torch.rand(N, 3, H, W, generator=g).to(dev)
    b = (a + 0.1 * torch.randn(N, 3, H, W, generator=g).to(dev)).clamp(0, 1).contiguous()
    rec = b.clone().requires_grad_(True)

    def torch_formula():
        return torch.autograd.grad((1 - metrics.ssim_map(a, rec, padding=True)).mean(), rec)
    paths = {'value_and_gradient': lambda: ops.ssim_term_value_grad(a, b), 'value_only': lambda: ops.ssim_term_value_grad(a, b, with_grad=False),
             'function_fwd_bwd': lambda: torch.autograd.grad(ops.ssim_term(a, rec), rec), 'torch_formula_fwd_bwd': torch_formula}
    for fn in paths.values():
        for _ in range(3):
            fn()
    ts = {k: [] for k in paths}
    for _ in range(repeats):
        for k, fn in paths.items():
            ts[k].append(timed(fn, inner if k != 'torch_formula_fwd_bwd' else max(inner // 10, 3)))
    out = {'what': 'ssim term alone', 'shape': [N, 3, H, W], 'inner': inner, 'repeats': repeats}
    out.update({k: spread(v) for k, v in ts.items()})
    moved = 3 * N * 3 * H * W * 4
    out['bytes_moved'] = moved
    out['GB_per_s_value_and_gradient'] = moved / statistics.median(ts['value_and_gradient']) / 1e9
    v, gr = ops.ssim_term_value_grad(a, b)
    gt, = torch_formula()
    out['value'] = v.item()
    out['max_abs_diff_to_torch_formula_over_max_abs'] = ((gr - gt).abs().max() / gt.abs().max()).item()
    return out


def bench_step(dev, views, repeats, steps, warmup):
    import bench
    from dbw_amd.lpips_vgg import LPIPSVGG
    from dbw_amd.parallel import ShardedTrainStep

    class A:
        pass
    a = A()
    a.views, a.H, a.W, a.blocks, a.fpp, a.txt = views, 300, 400, 10, 10, 256

    def make(kind):
        model, inp = bench.build_workload(a, dev)
        if kind != 'none':
            lw = {'rgb': model.loss_weights['rgb'], 'perceptual': 0.1}
            lw.update({k: v for k, v in model.loss_weights.items() if k != 'rgb'})
            model.loss_weights = lw
            if kind == 'ssim':
                model.set_perceptual(metrics.SSIMTerm())
            else:
                torch.manual_seed(5)
                model.set_perceptual(LPIPSVGG(allow_random_init=True).to(dev))
        model.sync_free = True
        step = ShardedTrainStep(model, lr=5e-3, lr_texture=5e-2, seed=227391)
        assert step.cstep is not None and step.cstep.supported(), 'the one-call C step refused the model'
        step.cstep.read_losses = True
        return step, inp
    legs = {k: make(k) for k in ('ssim', 'none', 'lpips')}
    vals = {}
    for k, (step, inp) in legs.items():
        for _ in range(warmup):
            vals[k] = step(inp).host()
    ts = {k: [] for k in legs}
    for _ in range(repeats):
        for k, (step, inp) in legs.items():
            ts[k].append(timed(lambda: step(inp).host(), steps if k != 'lpips' else max(steps // 5, 3)))
    added = [x - y for x, y in zip(ts['ssim'], ts['none'])]
    out = {'what': f'{views}-view C step, 300x400, 10 blocks, faces_per_pixel=10, 256^2 textures, loss values read every step',
           'steps_per_repeat': steps, 'repeats': repeats}
    for k in legs:
        s = spread(ts[k])
        out[k] = {'median_ms': s['median_us'] / 1e3, 'min_ms': s['min_us'] / 1e3, 'max_ms': s['max_us'] / 1e3,
                  'losses': {n: round(float(v), 6) for n, v in vals[k].items()}}
    out['added_ms'] = {'median': statistics.median(added) * 1e3, 'min': min(added) * 1e3, 'max': max(added) * 1e3}
    out['condition'] = 'added_ms.median < none.median_ms'
    out['condition_holds'] = bool(statistics.median(added) < statistics.median(ts['none']))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=['term', 'step'], default=None)
    ap.add_argument('--batches', type=int, nargs='+', default=[4, 49])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--inner', type=int, default=300)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    dev = torch.device('cuda:0')
    if args.only != 'step':
        for N in args.batches:
            print(json.dumps(bench_term(dev, N, 300, 400, args.repeats, args.inner)), flush=True)
    if args.only != 'term':
        print(json.dumps(bench_step(dev, 4, args.repeats, args.steps, args.warmup)), flush=True)


if __name__ == '__main__':
    main()
