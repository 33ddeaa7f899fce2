"""Times the surface term on a synthetic capture: a cloud of N points on and around n_blocks ellipsoids over a ground
plane, M points drawn per step.  Run by no test; the figures go into profiles/surface_term.md.

  --what term   forward + backward of ops.surface_term (the HIP kernels) against eval3d.surface_term_torch on the same device tensors
                (fp32, the chunked torch formulation: what a user could write without the kernels), alternated `--repeats` times each after
                a warm-up of both; every timed window is `inner` calls between two device events (torch.cuda.Event, elapsed_time), sized so
                that a window is tens of milliseconds at least.  Also the forward call alone with the box test on and off, and with
                back = 0 (no nearest-neighbour search of the vertices in the cloud, no back launch): the difference is their share.
  --what step   a general-path training step (autograd, launch by launch) of a model of n_blocks blocks with perceptual_name: ssim, with
                surface_weight 1 and with surface_weight 0, alternated, device events around `inner` steps.  Both legs are built with
                use_c_step=False: with the SSIM term and no surface term the default step would be the one-call C step (NativeStep refuses a
                perceptual term, so without the C step both legs take the general path).  A third leg, `c_step`, is the default step
                without the term -- the one-call C step --: what a user leaves behind by switching the term on.  --no-term times the legs
                without the term only (the parent commit has no surface_weight): the general-path step the term is compared with.
One JSON line per shape.  A run without a GPU fails: there is no CPU timing."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'differentiable-blocksworld_amd'))
sys.path.insert(0, os.path.join(HERE, '..', 'oracle'))


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner, out


def scene(n_blocks, N, dev, seed=0):
    """Ellipsoids on the model's own block mesh (42 vertices, 80 faces) over a ground of 128 faces; the cloud: points on random faces, 2 cm of
    noise."""
    from dbw_amd import mesh as M
    g = torch.Generator().manual_seed(seed)
    sv, sf = M.get_icosphere(level=1)
    gv, gf = M.get_plane()
    for _ in range(3):
        gv, gf = M.subdivide_mesh(gv, gf)
    gv = gv * torch.tensor([3.0, 1.0, 3.0]) + torch.tensor([0.0, -0.6, 0.0])
    verts, faces, fg, vg = [gv], [gf], [0, len(gf)], [torch.full((len(gv),), -1)]
    off = len(gv)
    for k in range(n_blocks):
        radii, centre = torch.rand(3, generator=g) * 0.15 + 0.1, (torch.rand(3, generator=g) * 2 - 1) * torch.tensor([1.5, 0.3, 1.5])
        verts.append(sv * radii + centre); faces.append(sf + off); fg.append(fg[-1] + len(sf)); vg.append(torch.full((len(sv),), k))
        off += len(sv)
    verts, faces = torch.cat(verts).float(), torch.cat(faces).to(torch.int32)
    w = torch.distributions.Dirichlet(torch.ones(3)).sample((N,))
    tri = verts[faces[torch.randint(0, len(faces), (N,), generator=g)].long()]
    cloud = (w[:, :, None] * tri).sum(1) + torch.randn(N, 3, generator=g) * 0.02
    return dict(points=cloud.float().contiguous().to(dev), verts=verts.contiguous().to(dev), faces=faces.contiguous().to(dev),
                face_group=torch.tensor(fg, dtype=torch.int32, device=dev), group_keep=None,
                vert_alpha=torch.rand(n_blocks, generator=g).to(dev), vert_group=torch.cat(vg).to(torch.int32).to(dev)), float(n_blocks * len(sv))


def bench_term(args, dev):
    from dbw_amd import eval3d, ops
    for nb in args.blocks:
        d, bc = scene(nb, args.cloud, dev)
        kw = dict(n_points=args.points, tau=0.1, back=0.5, seed=3, weight=1.0, back_count=bc)
        state = {'step': 0}

        def run(fn):
            def once():
                state['step'] += 1
                v, a = d['verts'].clone().requires_grad_(), d['vert_alpha'].clone().requires_grad_()
                out = fn(**dict(d, verts=v, vert_alpha=a), step=state['step'], **kw)
                out.backward()
                return out.detach(), v.grad, a.grad
            return once
        paths = {'hip': run(ops.surface_term), 'torch': run(eval3d.surface_term_torch)}
        inner = {'hip': 50, 'torch': 2}
        for n in paths:
            event_ms(paths[n], 1)
        times = {n: [] for n in paths}
        for _ in range(args.repeats):
            for n in paths:
                times[n].append(event_ms(paths[n], inner[n])[0])
        fwd = {}
        for cull in (1, 0):
            f = lambda: ops.surface_records(**d, n_points=args.points, tau=0.1, back=0.5, seed=3, step=7, back_count=bc, cull=cull)      # noqa: E731
            event_ms(f, 1)
            fwd[cull] = sorted(event_ms(f, 50)[0] for _ in range(args.repeats))
        f0 = lambda: ops.surface_records(**d, n_points=args.points, tau=0.1, back=0.0, seed=3, step=7, back_count=bc, cull=1)      # noqa: E731
        event_ms(f0, 1)
        fwd['no_back'] = sorted(event_ms(f0, 50)[0] for _ in range(args.repeats))
        state['step'] = 100
        a = paths['hip']()
        state['step'] = 100
        b = paths['torch']()
        med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
        print(json.dumps({'what': 'term', 'blocks': nb, 'faces': int(d['faces'].shape[0]), 'verts': int(d['verts'].shape[0]), 'cloud': args.cloud,
                          'points': args.points, 'device': torch.cuda.get_device_name(0), 'inner_calls': inner,
                          'hip_fwd_bwd_ms': [round(t, 4) for t in times['hip']], 'torch_fwd_bwd_ms': [round(t, 4) for t in times['torch']],
                          'median_ms': med, 'torch_over_hip': med['torch'] / med['hip'],
                          'hip_forward_call_ms': {'cull': [round(t, 4) for t in fwd[1]], 'no_cull': [round(t, 4) for t in fwd[0]],
                                                  'cull_back_0': [round(t, 4) for t in fwd['no_back']]},
                          'value': [float(a[0]), float(b[0])], 'largest_vertex_gradient_difference': float((a[1] - b[1]).abs().max()),
                          'largest_vertex_gradient': float(b[1].abs().max())}), flush=True)


def bench_step(args, dev):
    import oracle as O
    from dbw_amd import create_model
    from dbw_amd.parallel import ShardedTrainStep
    H, W = 128, 192
    for nb in args.blocks:
        steps = {}
        for name, weight, c_step in (('without', 0.0, False), ('c_step', 0.0, True)) + (() if args.no_term else (('with', 1.0, False),)):
            loss = {'rgb_weight': 1, 'perceptual_weight': 0.1, 'perceptual_name': 'ssim', 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}
            if weight:
                loss.update(surface_weight=weight, surface={'points': args.points})
            cfg = {'model': {'name': 'dbw', 'mesh': {'n_blocks': nb, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': 64},
                             'renderer': {'faces_per_pixel': 10, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                             'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True,
                                            'opacity_noise': False}, 'loss': loss}}
            torch.manual_seed(3)
            model = create_model(cfg, (H, W)).to(dev).train()
            model.sync_free = True
            if weight:
                with torch.no_grad():
                    v = model.blocks_mesh(filter_transparent=False)[0]
                g = torch.Generator(device=dev).manual_seed(1)
                model.set_surface_points(v[torch.randint(0, len(v), (args.cloud,), generator=g, device=dev)] +
                                         0.02 * torch.randn(args.cloud, 3, generator=g, device=dev))
            R, T, K = O.synthetic_cameras(4, R_world=model.R_world[0].cpu())
            inp = {'imgs': torch.rand(4, 3, H, W, generator=torch.Generator().manual_seed(0)).to(dev), 'R': R.to(dev), 'T': T.to(dev), 'K': K.to(dev)}
            step = ShardedTrainStep(model, lr=1e-3, lr_texture=1e-2, seed=1, use_c_step=c_step)
            took_c = step.cstep is not None and step.cstep.supported()
            if took_c != c_step or (step.native is not None and step.native.supported()):
                raise SystemExit(f'surface_bench: the {name} leg would not take the path it is named for')
            steps[name] = lambda step=step, inp=inp: step(inp)
        for n in steps:
            event_ms(steps[n], 3)
        times = {n: [] for n in steps}
        for _ in range(args.repeats):
            for n in steps:
                times[n].append(event_ms(steps[n], 20)[0])
        med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
        print(json.dumps({'what': 'step', 'blocks': nb, 'image': [H, W], 'views': 4, 'cloud': args.cloud, 'points': args.points,
                          'device': torch.cuda.get_device_name(0), 'step_ms': {n: [round(t, 4) for t in ts] for n, ts in times.items()},
                          'median_ms': med, 'paths': {'without': 'general', 'with': 'general', 'c_step': 'one-call C step'},
                          'term_ms_general_vs_general': (med['with'] - med['without']) if 'with' in med else None}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', choices=['term', 'step'], default='term')
    ap.add_argument('--blocks', type=int, nargs='+', default=[10, 50])
    ap.add_argument('--cloud', type=int, default=262144)
    ap.add_argument('--points', type=int, default=16384)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-term', action='store_true', help='time the step without the term only (the parent commit has no surface_weight)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('surface_bench needs a GPU: there is no CPU timing')
    dev = torch.device('cuda:0')
    (bench_term if args.what == 'term' else bench_step)(args, dev)


if __name__ == '__main__':
    main()
