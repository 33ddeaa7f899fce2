"""Times the free-space term on a synthetic capture: N depth rays from 8 camera centres to points on a ground plane and on
n_blocks ellipsoids standing over it, M rays drawn per step.  Run by no test; the figures go into profiles/freespace_term.md.

  --what term   forward + backward of ops.freespace_term (the HIP kernels) against ops.freespace_term_torch on the same device tensors
                (fp32, the chunked torch formulation: what a user could write without the kernels), alternated `--repeats` times each after
                a warm-up of both; every timed window is `inner` calls between two device events (torch.cuda.Event, elapsed_time), sized so
                that a window is tens of milliseconds at least.  Also the forward call alone in its two layouts (1: a workgroup per 256 rays walks
                every face; 2: ray tiles x face chunks with an integer atomic minimum), each with the slab test on and off.
  --what step   a general-path training step (autograd, launch by launch) of a model of n_blocks blocks with perceptual_name: ssim, with
                freespace_weight 1 and with freespace_weight 0, alternated, device events around `inner` steps.  Both legs are built with
                use_c_step=False, as tools/surface_bench.py builds its own (whose --no-term legs are the same step on a commit without the
                term).
One JSON line per shape.  A run without a GPU fails: there is no CPU timing."""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'differentiable-blocksworld_amd'))
sys.path.insert(0, os.path.join(HERE, '..', 'oracle'))
sys.path.insert(0, HERE)

from surface_bench import event_ms, scene as surface_scene        # noqa: E402


def scene(n_blocks, N, dev, seed=0):
    """tools/surface_bench.py's meshes; the rays: 8 origins on a ring above the scene, ends on random faces (the ground's among them) with
    2 cm of noise -- a ray to the ground behind a block passes through the block: those are the hits."""
    d, _ = surface_scene(n_blocks, N, dev, seed)
    g = torch.Generator().manual_seed(seed + 1)
    ang = torch.arange(8) * (2 * torch.pi / 8) + 0.3
    origins = torch.stack([2.5 * torch.cos(ang), torch.full((8,), 1.2) + 0.2 * torch.sin(3 * ang), 2.5 * torch.sin(ang)], 1).float()
    frame = torch.randint(0, 8, (N,), generator=g).to(torch.int32)
    G = d['face_group'].numel() - 1
    return dict(ends=d['points'], frame=frame.to(dev), origins=origins.contiguous().to(dev), verts=d['verts'], faces=d['faces'],
                face_group=d['face_group'], group_keep=None, group_alpha=torch.tensor([-1] + list(range(G - 1)), dtype=torch.int32, device=dev),
                vert_alpha=d['vert_alpha'])


def bench_term(args, dev):
    from dbw_amd import ops
    for nb in args.blocks:
        d = scene(nb, args.total, dev)
        kw = dict(n_rays=args.rays, tau=0.1, margin=0.02, seed=3, weight=1.0)
        state = {'step': 0}

        def run(fn):
            def once():
                state['step'] += 1
                v, a = d['verts'].clone().requires_grad_(), d['vert_alpha'].clone().requires_grad_()
                out = fn(**dict(d, verts=v, vert_alpha=a), step=state['step'], **kw)
                out.backward()
                return out.detach(), v.grad, a.grad
            return once
        paths = {'hip': run(ops.freespace_term), 'torch': run(ops.freespace_term_torch)}
        inner = {'hip': 50, 'torch': 2}
        for n in paths:
            event_ms(paths[n], 1)
        times = {n: [] for n in paths}
        for _ in range(args.repeats):
            for n in paths:
                times[n].append(event_ms(paths[n], inner[n])[0])
        fwd = {}
        legs = [(layout, cull) for layout in (1, 2) for cull in (1, 0)]
        calls = {leg: (lambda leg=leg: ops.freespace_records(**d, n_rays=args.rays, tau=0.1, margin=0.02, seed=3, step=7, layout=leg[0], cull=leg[1]))
                 for leg in legs}
        for leg in legs:
            event_ms(calls[leg], 1)
            fwd[leg] = []
        for _ in range(args.repeats):                               # (alternated, as the two paths above)
            for leg in legs:
                fwd[leg].append(event_ms(calls[leg], 50)[0])
        same = len({ops.freespace_records(**d, n_rays=args.rays, tau=0.1, margin=0.02, seed=3, step=7, layout=layout)[0].cpu().numpy().tobytes()
                    for layout in (1, 2)}) == 1
        rec = ops.freespace_records(**d, n_rays=args.rays, tau=0.1, margin=0.02, seed=3, step=7)[0]
        state['step'] = 100
        a = paths['hip']()
        state['step'] = 100
        b = paths['torch']()
        med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
        print(json.dumps({'what': 'term', 'blocks': nb, 'faces': int(d['faces'].shape[0]), 'verts': int(d['verts'].shape[0]), 'total_rays': args.total,
                          'rays': args.rays, 'device': torch.cuda.get_device_name(0), 'inner_calls': inner,
                          'hip_fwd_bwd_ms': [round(t, 4) for t in times['hip']], 'torch_fwd_bwd_ms': [round(t, 4) for t in times['torch']],
                          'median_ms': med, 'torch_over_hip': med['torch'] / med['hip'],
                          'hip_forward_call_ms': {f'layout_{layout}_{"cull" if cull else "no_cull"}': sorted(round(t, 4) for t in fwd[(layout, cull)])
                                                  for layout, cull in legs},
                          'layouts_give_the_same_records': same,
                          'share_of_rays_with_a_hit': float((rec[:, 1] >= 0).float().mean()),
                          'value': [float(a[0]), float(b[0])], 'largest_vertex_gradient_difference': float((a[1] - b[1]).abs().max()),
                          'largest_vertex_gradient': float(b[1].abs().max())}), flush=True)


def bench_step(args, dev):
    import oracle as O
    from dbw_amd import create_model
    from dbw_amd.parallel import ShardedTrainStep
    H, W = 128, 192
    for nb in args.blocks:
        steps = {}
        for name, weight in (('without', 0.0), ('with', 1.0)):
            loss = {'rgb_weight': 1, 'perceptual_weight': 0.1, 'perceptual_name': 'ssim', 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1,
                    'freespace_weight': weight, 'freespace': {'rays': args.rays}}
            cfg = {'model': {'name': 'dbw', 'mesh': {'n_blocks': nb, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': 64},
                             'renderer': {'faces_per_pixel': 10, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                             'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True,
                                            'opacity_noise': False}, 'loss': loss}}
            torch.manual_seed(3)
            model = create_model(cfg, (H, W)).to(dev).train()
            model.sync_free = True
            R, T, K = O.synthetic_cameras(4, R_world=model.R_world[0].cpu())
            if weight:
                with torch.no_grad():
                    v = model.blocks_mesh(filter_transparent=False)[0].reshape(-1, 3)
                g = torch.Generator(device=dev).manual_seed(1)
                ends = v[torch.randint(0, len(v), (args.total,), generator=g, device=dev)] + 0.3 * torch.randn(args.total, 3, generator=g, device=dev)
                centres = -torch.einsum('nij,nj->ni', R, T)                      # the cameras' centres: x_cam = x R + T
                model.set_freespace_rays(ends, torch.randint(0, 4, (args.total,), generator=g, device=dev), centres.to(dev))
            inp = {'imgs': torch.rand(4, 3, H, W, generator=torch.Generator().manual_seed(0)).to(dev), 'R': R.to(dev), 'T': T.to(dev), 'K': K.to(dev)}
            step = ShardedTrainStep(model, lr=1e-3, lr_texture=1e-2, seed=1, use_c_step=False)
            if (step.cstep is not None and step.cstep.supported()) or (step.native is not None and step.native.supported()):
                raise SystemExit(f'freespace_bench: the {name} leg would not take the general path')
            steps[name] = lambda step=step, inp=inp: step(inp)
        for n in steps:
            event_ms(steps[n], 3)
        times = {n: [] for n in steps}
        for _ in range(args.repeats):
            for n in steps:
                times[n].append(event_ms(steps[n], 20)[0])
        med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
        print(json.dumps({'what': 'step', 'blocks': nb, 'image': [H, W], 'views': 4, 'total_rays': args.total, 'rays': args.rays,
                          'device': torch.cuda.get_device_name(0), 'step_ms': {n: [round(t, 4) for t in ts] for n, ts in times.items()},
                          'median_ms': med, 'paths': {'without': 'general', 'with': 'general'},
                          'term_ms': med['with'] - med['without']}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', choices=['term', 'step'], default='term')
    ap.add_argument('--blocks', type=int, nargs='+', default=[10, 50])
    ap.add_argument('--total', type=int, default=1 << 20, help='rays of the capture')
    ap.add_argument('--rays', type=int, default=16384, help='rays drawn per step')
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('freespace_bench needs a GPU: there is no CPU timing')
    dev = torch.device('cuda:0')
    (bench_term if args.what == 'term' else bench_step)(args, dev)


if __name__ == '__main__':
    main()
