#!/usr/bin/env python
"""bench.py -- BASELINE.json metric: rendered views/sec (fwd+bwd) per node, DTU-like 400x300, K=10 blocks.

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A "step" = one full optimisation iteration of the hot path over this rank's batch of synthetic views (config 2 of
BASELINE.json: V=49 views per GPU, 300x400 (HxW), 10 superquadric blocks + ground + sky dome, faces_per_pixel=10, 256^2
textures, coarse phase at epoch 0: sigma=1e-4, opacity noise, decimated textures): param -> mesh, env pass + fg pass
(project/clip, raster, shade+blend), composite + MSE, parsimony/TV/overlap regularisers, backward to all 10 parameter
tensors, [RCCL all-reduce of the flat gradient buffer when N > 1], fused Adam on both lr groups.  LPIPS is excluded
(SURVEY.md 8a A10).  Inputs are resident in HBM before the timed region.  Weak scaling (default): every rank renders V views per
step; value = N * V * steps / max-over-ranks time.  `--scaling strong` is BASELINE config 3 as written: the SAME 49 views split over
the ranks (7,6,...,6), value = V * steps / time.  A plain run does only that: set-up, warm-up, the timed steps, one JSON line from
rank 0 (the measurements below are null in it).  `--dump-outputs DIR` then writes what one more call of the timed path, from the seeded
state the warm-up started from, hands its caller (loss values, parameters after Adam, their gradient, Adam's moments) as DIR/<name>.npy, to
compare two builds output for output.

`--full` adds, measured in the same run after the timed region: the two other training phases of the config (`phases`), the per-step
all-reduce time (`allreduce_ms`) and the other scaling form (N > 1), `roofline` for the dominant kernel (HIP-event timed on the launch
stream), and at N = 1 the extra legs and `cpu_baseline` (the CPU oracle -- a port: the reference's own path needs PyTorch3D -- on a
bounded sample)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, 'differentiable-blocksworld_amd'))

import torch                                                            # noqa: E402
import torch.distributed as dist                                        # noqa: E402

PMC_FILE = 'r06_pmc_counters.json'


def csrc_sha16():
    """Hash of the kernel sources + build flags of the library: committed counter files are keyed on it (a later kernel change must not ship
    the counters of the old kernels)."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, 'differentiable-blocksworld_amd', 'csrc')
    for f in sorted(os.listdir(d)):
        h.update(f.encode())
        h.update(open(os.path.join(d, f), 'rb').read())
    h.update(open(os.path.join(ROOT, 'differentiable-blocksworld_amd', 'build.py'), 'rb').read())
    return h.hexdigest()[:16]


HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured float4 copy)


def live_traffic(dom_label, calib, steps=5, limit_s=240):
    """HBM bytes per launch of the dominant kernel, measured IN THIS RUN: two child processes of this bench run -- `rocprofv3 --kernel-trace
    --pmc FETCH_SIZE` and `... --pmc WRITE_SIZE`, one counter per pass as MI355X_MICROARCH.md prescribes, no other trace domain -- each over
    `steps` training steps of the headline workload (tools/pmc_target.py: the same build_workload, the same one-call step; its streams wait
    through events there, a counter pass runs one kernel at a time).  Median over the kernel's dispatches of the sum over the counter's
    instances, x the byte-counter factors `calib` ({fetch, write}: known bytes / reported bytes for 4 B-per-lane plane traffic, measured with
    tools/ubench/plane_rw.hip next to the committed counters; 2.0 / 1.0 = the guide's gfx950 correction).  Returns (bytes or None, note)."""
    import csv, glob, shutil, signal, subprocess, tempfile
    rp = shutil.which('rocprofv3') or next((p for p in ('/opt/rocm/bin/rocprofv3',) if os.path.exists(p)), None)
    if rp is None:
        return None, 'rocprofv3 not found'
    want = next((v for k, v in (('render_fwd_fused K=1 ', 'render_fwd_kernel<1,'), ('render_fwd_fused', 'render_fwd_kernel<'), ('render_bwd_fused K=1 ', 'render_bwd_hard_kernel'),
                                ('render_bwd_fused', 'render_bwd_uv_kernel')) if dom_label.startswith(k)), None)
    if want is None:
        return None, f'no kernel name known for {dom_label}'
    kb = {}
    for ctr in ('FETCH_SIZE', 'WRITE_SIZE'):
        d = tempfile.mkdtemp(prefix='dbw_pmc_', dir='/tmp')
        env = dict(os.environ, DBW_STEP_EVENTS='1', DBW_EPOCH='0', DBW_STEPS=str(steps), TMPDIR='/tmp')
        for k in ('DBW_DEBUG_FLAGS', 'DBW_RENDER_VARIANT', 'DBW_PMC_EMPTY', 'RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
            env.pop(k, None)
        try:
            proc = subprocess.Popen([rp, '--kernel-trace', '--pmc', ctr, '-d', d, '-o', 'p', '--output-format', 'csv', '--', sys.executable,
                                     os.path.join(ROOT, 'tools', 'pmc_target.py')], env=env, cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                                    start_new_session=True)
            try:
                rc = proc.wait(timeout=limit_s)
            except subprocess.TimeoutExpired:
                os.killpg(proc.pid, signal.SIGKILL)          # (the process group this call started, nothing else)
                proc.wait()
                return None, f'the {ctr} pass did not finish within {limit_s} s'
            if rc != 0:
                return None, f'the {ctr} pass exited with {rc}'
            per = {}
            for f in glob.glob(os.path.join(d, '**', '*counter_collection.csv'), recursive=True):
                for r in csv.DictReader(open(f, encoding='utf-8', errors='replace')):
                    if want in r['Kernel_Name'] and r['Counter_Name'] == ctr:
                        per[r['Dispatch_Id']] = per.get(r['Dispatch_Id'], 0.0) + float(r['Counter_Value'])
            if not per:
                return None, f'the {ctr} pass reported no dispatch of {want}'
            kb[ctr] = sorted(per.values())[len(per) // 2]
        except (OSError, ValueError, KeyError) as e:
            return None, f'the {ctr} pass failed: {e!r}'
        finally:
            shutil.rmtree(d, ignore_errors=True)
    nbytes = int((calib['fetch'] * kb['FETCH_SIZE'] + calib['write'] * kb['WRITE_SIZE']) * 1024)          # (the counters are in KB)
    return nbytes, (f'measured in this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE (one pass each) over {steps} steps of this workload in child '
                    f'processes, median per launch of {want}...; FETCH_SIZE {kb["FETCH_SIZE"] / 1024:.1f} MB x {calib["fetch"]:.3f} + WRITE_SIZE '
                    f'{kb["WRITE_SIZE"] / 1024:.1f} MB x {calib["write"]:.3f}')


def make_cfg(n_blocks, fpp, ts):
    return {'model': {'name': 'dbw',
                      'mesh': {'n_blocks': n_blocks, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': ts},
                      'renderer': {'faces_per_pixel': fpp, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                      'rend_optim': {'coarse_learning': 1500, 'decimate_txt': 750, 'decimate_factor': 8, 'kill_blocks': True,
                                     'decouple_rendering': True, 'opacity_noise': True},
                      'loss': {'rgb_weight': 1, 'perceptual_weight': 0, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}}}


def build_workload(args, dev):
    import dbw_amd
    from dbw_amd import mesh as M
    torch.manual_seed(227391)                                           # configs/dtu/default.yml:42
    model = dbw_amd.create_model(make_cfg(args.blocks, args.fpp, args.txt), (args.H, args.W)).to(dev)
    R, T, K = M.synthetic_cameras(args.views, R_world=model.R_world[0])
    # targets: a self-render of a perturbed scene (realistic coverage), fp32 (B,3,H,W) in [0,1]
    target = dbw_amd.create_model(make_cfg(args.blocks, args.fpp, args.txt), (args.H, args.W)).to(dev)
    with torch.no_grad():
        g = torch.Generator().manual_seed(99)
        target.T.add_(torch.randn(target.T.shape, generator=g).to(dev) * 0.2)
        target.alpha_logit.add_(2.0)
        target.textures.add_(torch.randn(target.textures.shape, generator=g).to(dev))
        target.texture_bkg.add_(torch.randn(target.texture_bkg.shape, generator=g).to(dev))
        target.eval()
        inp = {'imgs': torch.zeros(args.views, 3, args.H, args.W, device=dev), 'R': R.to(dev), 'T': T.to(dev), 'K': K.to(dev)}
        inp['imgs'] = target.predict(inp, None).clamp(0, 1).contiguous()
    del target
    model.train()
    return model, inp


DUMP_LIMIT_BYTES = 64_000_000


def write_outputs(d, arrays, limit=DUMP_LIMIT_BYTES):
    """{name: tensor} -> d/<name>.npy, float64 kept, everything else as float32, `limit` bytes in all.  Smallest first, an array is
    written whole when it fits an equal share of the bytes still free, else as a sample of that many elements drawn with seed 0, in
    flat-index order: the same elements on every run with the same arguments, so that two runs compare element for element."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    arrays = {k: v.detach().cpu() for k, v in arrays.items()}
    arrays = {k: v.double() if v.dtype == torch.float64 else v.float() for k, v in arrays.items()}
    free = limit - 256 * len(arrays)                    # (256 B: room for each file's header)
    order = sorted(arrays, key=lambda k: arrays[k].numel() * arrays[k].element_size())
    for i, k in enumerate(order):
        v = arrays[k]
        m = min(v.numel(), int(free / (len(order) - i)) // v.element_size())
        if m < v.numel():
            idx = torch.randperm(v.numel(), generator=torch.Generator().manual_seed(0))[:m].sort().values
            v = v.reshape(-1)[idx]
        free -= v.numel() * v.element_size()
        np.save(os.path.join(d, f'{k}.npy'), v.numpy())


def dump_outputs(d, model, step, losses):
    """What one call of the timed path handed its caller: the loss values `losses`, the parameters Adam moved, the gradient it moved them
    by and Adam's two moments (the flat buffers of parallel.FlatParams and ShardedTrainStep, in the parameters' shapes).  main() makes that
    call the first step from the seeded state, where the bias-corrected moments are g and g^2 whatever the betas: the moments themselves,
    (1 - beta1) g and (1 - beta2) g^2, are what show the betas.  What the optimiser does past its first step (the bias correction at
    n_steps > 1, moments carried from step to step) is not in the dump."""
    torch.cuda.synchronize()
    shapes = {n: p.shape for n, p in model.named_parameters()}
    arrays = {f'loss_{k}': v for k, v in losses.items() if v is not None}
    for name, off, k in step.params.names:
        arrays[f'param_{name}'] = step.params.flat[off:off + k].view(shapes[name])
        arrays[f'grad_{name}'] = step.params.grad[off:off + k].view(shapes[name])
        arrays[f'exp_avg_{name}'] = step.exp_avg[off:off + k].view(shapes[name])
        arrays[f'exp_avg_sq_{name}'] = step.exp_avg_sq[off:off + k].view(shapes[name])
    write_outputs(d, arrays)


BIN_STATS = {}


def measure_other(views, H, W, blocks, fpp, txt, dev, steps, warmup, read_losses=False, lr_scale=1.0, min_seconds=0.0, epoch=0, c_step=True):
    """One more workload measured like the headline (same step, same launch path, inputs resident), outside its timed region:
    -> ms per step, views / s and the share of the HBM roofline the WHOLE-PATH algorithmic bytes (64 P K + 140 P per view)
    reach.  read_losses: every loss value is read on the host after every step, as the reference's trainer does
    (src/trainer.py:143); lr_scale = 0: frozen parameters (Adam runs, nothing moves); min_seconds: keep stepping that long."""
    from dbw_amd.parallel import ShardedTrainStep

    class A:
        pass
    a = A()
    a.views, a.H, a.W, a.blocks, a.fpp, a.txt = views, H, W, blocks, fpp, txt
    model, inp = build_workload(a, dev)
    model.set_cur_epoch(epoch)
    model.sync_free = True
    step = ShardedTrainStep(model, lr=5e-3 * lr_scale, lr_texture=5e-2 * lr_scale, seed=227391, use_c_step=c_step)
    if step.cstep is not None:
        step.cstep.read_losses = bool(read_losses)        # the step copies its five loss values to host memory itself

    def read(out):
        # every loss value on the host after every step (trainer.py:143): one wait for the step's own copy (C step), or six scalar reads
        return out.host() if hasattr(out, 'host') else {k: float(v) for k, v in out.items()}
    for _ in range(warmup):
        out = step(inp)
        if read_losses:
            read(out)
    torch.cuda.synchronize()
    st0 = torch.cuda.memory_stats(dev)
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(steps):
            out = step(inp)
            if read_losses:
                vals = read(out)
        n += steps
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            break
    total = float(out['total'])
    assert total == total, 'loss is NaN'
    P = H * W
    vps = views * n / dt
    st1 = torch.cuda.memory_stats(dev)
    res = {'workload': f'{views} views/step, {W}x{H}, {blocks} blocks, faces_per_pixel={fpp}, {txt}^2 textures', 'steps': n,
           'ms_per_step': dt / n * 1e3, 'views_per_s': vps, 'whole_path_frac': vps * (64 * P * fpp + 140 * P) / 1e9 / HBM_PEAK_GBS,
           # device allocations (hipMalloc) inside the timed region: must be 0 -- every buffer of a step comes out of torch's cache
           'device_allocs_in_timed_region': int(st1.get('num_device_alloc', 0) - st0.get('num_device_alloc', 0)),
           'step': 'one C-ABI call per iteration (dbw_train_step_run)' if step.cstep is not None else 'launch by launch from Python'}
    del step, model, inp
    torch.cuda.empty_cache()
    return res


def measure_perceptual(dev, views=4, steps=30, warmup=5):
    """The iteration with the loss every shipped config uses (configs/dtu/default.yml:23: perceptual_weight 0.1; src/model/dbw.py:369-371):
    LPIPS-VGG16 on the composite, here with seeded weights (none exist offline: the architecture and its cost are real, the values are
    not), at the reference's batch size.  The network is torch / MIOpen outside the library; the step runs in two phases around it
    (c_step.py).  -> ms per step, and the network's forward + backward alone on the same images."""
    from dbw_amd.lpips_vgg import LPIPSVGG
    from dbw_amd.parallel import ShardedTrainStep

    class A:
        pass
    a = A()
    a.views, a.H, a.W, a.blocks, a.fpp, a.txt = views, 300, 400, 10, 10, 256
    model, inp = build_workload(a, dev)
    model.loss_weights = dict(model.loss_weights)
    model.loss_weights = {k: model.loss_weights[k] for k in model.loss_weights}
    lw = {'rgb': model.loss_weights['rgb'], 'perceptual': 0.1}
    lw.update({k: v for k, v in model.loss_weights.items() if k != 'rgb'})
    model.loss_weights = lw
    torch.manual_seed(5)
    net = LPIPSVGG(allow_random_init=True).to(dev)
    model.set_perceptual(net)
    model.sync_free = True
    step = ShardedTrainStep(model, lr=5e-3, lr_texture=5e-2, seed=227391)
    assert step.cstep is not None and step.cstep.supported()
    step.cstep.read_losses = True
    for _ in range(warmup):
        step(inp).host()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        vals = step(inp).host()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    rec = torch.rand_like(inp['imgs']).requires_grad_(True)
    for _ in range(3):
        torch.autograd.grad(net(inp['imgs'], rec), rec)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        torch.autograd.grad(net(inp['imgs'], rec), rec)
    torch.cuda.synchronize()
    net_ms = (time.perf_counter() - t0) / 10 * 1e3
    # ... and as dbw_amd.trainer.Trainer runs it: the targets' features are constants of the training views (frozen network, fixed images) --
    # computed once, gathered by view id (lpips_vgg.LPIPSVGG.cache_targets).  Same values.
    net.cache_targets(inp['imgs'])
    inp_ids = dict(inp, view_ids=torch.arange(views, device=dev))
    for _ in range(warmup):
        step(inp_ids).host()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        vals_c = step(inp_ids).host()
    torch.cuda.synchronize()
    ms_c = (time.perf_counter() - t0) / steps * 1e3
    return {'what': f'batch_size {views} with perceptual_weight 0.1: LPIPS-VGG16 (seeded weights, torch / MIOpen, outside the library) between the two '
                    'phases of the C step; loss values read every step', 'ms_per_step': ms, 'lpips_fwd_bwd_alone_ms': net_ms,
            'render_path_ms': ms - net_ms, 'losses': {k: round(v, 6) for k, v in vals.items()},
            'ms_per_step_cached_targets': ms_c, 'cached_targets': 'the Trainer\'s default: target features computed once per training view and gathered by view id '
                                                                  '(lpips_vgg.py); losses after the same number of steps: '
                                                                  + str({k: round(v, 6) for k, v in vals_c.items()})}


def kernel_breakdown(model, inp, reps=5):
    """HIP-event timing (events recorded on the stream the kernels are launched on = torch's current stream) of the four
    kernels that dominate an iteration -- the fused forward and fused backward of the fg (soft, K faces per pixel) and env
    (hard, 1 face per pixel) passes -- each launched alone on the real step geometry.
    -> {name: (avg_ms, algorithmic_bytes_per_launch)}; bytes per view: forward writes 20*P*K of fragments + 16*P of image,
    backward reads them back plus the 16*P image gradient (zbuf not materialised)."""
    from dbw_amd import _lib, ops
    B, H, W = inp['R'].shape[0], model.img_size[0], model.img_size[1]
    P = H * W
    res = {}
    with torch.no_grad():
        fine = not model.is_live('coarse_learning')                        # same choices as DifferentiableBlocksWorld.render_layers
        blocks = model.build_blocks_scene(filter_transparent=fine)
        alpha = None if fine else model._alpha.detach().repeat_interleave(model.BNF).contiguous()
        passes = [('env', model.renderer_env, model.build_env_scene(), None, True),
                  ('fg', model.renderer_fine if fine else model.renderer, blocks, alpha, bool(model._blocks_decimated))]
    img_env = None
    for tag, r, scene, alpha, agg in passes:
        cfg = r._cfg(scene.faces.shape[0], lds_aggregate=agg, const_faces=getattr(scene, 'const_faces', 0))
        K = cfg.K
        Kmat = r.cameras.K[0].contiguous()
        verts, maps = scene.verts.detach(), scene.maps.detach()
        cl = ops.project_clip(verts, scene.faces, inp['R'], inp['T'], Kmat, cfg.eps, cfg.z_clip, cfg.persp)
        fvc = cl['face_verts'].view(-1, 3, 3)
        # fragment layout the training step uses for this pass
        mode = 2 if (cfg.detach_bary and ops.UV_FRAGMENTS) else ops.hard_layout(cfg, alpha, scene.map_desc)
        # the render kernel alone, as the training step launches it: the per-face set-up of the pass (stage 1: records, bins, tile
        # lists, launch order -- a few small kernels that run ahead of the pass on the other stream) is done once, outside the timed region
        if tag == 'fg' and mode == 2:
            # the training step's form of the soft pass: composite over the env image + MSE against the targets in the epilogue, the
            # two gradient images instead of an image (dbw_render_fwd_fused_mse); one opacity per block as in native_step
            fa_blk = None if fine else model._alpha.detach().contiguous()
            scale = 1.0 / inp['imgs'].numel()
            target = ops.tile_image(inp['imgs'])                          # (the step tiles the targets once)
            state = ops.render_fwd_fused_mse(cl, B, cfg, scene.face_uvs, scene.face_map, scene.map_desc, maps, fa_blk, r._bg, None, None, 0.0, stage=1,
                                             img_tiled=True)
            fwd = lambda: ops.render_fwd_fused_mse(cl, B, cfg, scene.face_uvs, scene.face_map, scene.map_desc, maps, fa_blk, r._bg, img_env,
                                                   target, scale, stage=2, state=state, img_tiled=True)
            p2f, bary, dists, _part, g_img, _g_env = fwd()
            g_img = g_img.clone()
            alpha = fa_blk
        else:
            state = ops._render_fwd_fused(fvc, cl, B, cfg, scene.face_uvs, scene.face_map, scene.map_desc, maps, alpha, r._bg, mode, stage=1,
                                          img_tiled=True)
            fwd = lambda: ops._render_fwd_fused(fvc, cl, B, cfg, scene.face_uvs, scene.face_map, scene.map_desc, maps, alpha, r._bg, mode, stage=2,
                                                state=state, img_tiled=True)
            p2f, bary, dists, img = fwd()
            g_img = torch.rand_like(img)
            if tag == 'env':
                img_env = img
        g_maps, g_fvc = torch.zeros_like(maps), torch.zeros_like(fvc)
        g_alpha = torch.zeros_like(alpha) if alpha is not None else None
        if alpha is not None and ops._alpha_len(alpha, scene.map_desc, cfg.F) < 0:     # one opacity per map: 64 partial sums each
            g_alpha = torch.zeros(alpha.numel() * ops.ALPHA_SPREAD, device=alpha.device)
        bins = scene.texbins if (ops.TEXTURE_BINS and not agg and scene.texbins is not None and scene.texbins[2] > 0) else None
        bin_base = cursor = records = layout = 0
        cap = 0
        if bins is not None:                                               # same sizing as ops._RenderScene.backward
            nbins = bins[2]
            cap = ops.texbin_capacity(B, H, W, K, nbins)
            cursor_t = torch.zeros(nbins * ops.BIN_SUBCURSORS, dtype=torch.int32, device=fvc.device)   # one cursor per record sub-range
            records_t = torch.empty(nbins * cap * 8, dtype=torch.int32, device=fvc.device)
            bin_base, cursor, records = bins[0].data_ptr(), cursor_t.data_ptr(), records_t.data_ptr()
            layout = ops.uniform_bin_layout(nbins, cap, fvc.device).data_ptr()            # equal shares (the step sizes them by demand)

        def bwd():
            if bins is not None:
                cursor_t.zero_()
            _lib.call('dbw_render_bwd_fused', *ops._shade_args(p2f, bary, dists, cl, scene.face_uvs, scene.face_map, scene.map_desc, maps,
                                                               alpha, cfg.F, cfg.sigma, r._bg, (B, H, W, K)),
                      g_img.data_ptr(), fvc.data_ptr(), int(cfg.persp), int(cfg.detach_bary), g_maps.data_ptr(),
                      0 if g_alpha is None else g_alpha.data_ptr(), g_fvc.data_ptr(), int(agg), mode, bin_base, cursor, records, cap, layout,
                      int(getattr(scene, 'const_faces', 0)), 0, 1, ops._stream(fvc))          # image_layout 1: the step's tiled images

        def reduce():
            _lib.call('dbw_texbin_reduce', bins[1].data_ptr(), cursor, records, cap, layout, bins[2], g_maps.data_ptr(), ops._stream(fvc))

        def t(fn):
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps

        res[f'render_fwd_fused K={K} ({tag} pass)'] = (t(fwd), (20 * P * K + 16 * P) * B)
        res[f'render_bwd_fused K={K} ({tag} pass)'] = (t(bwd), (20 * P * K + 16 * P) * B)
        if bins is not None:
            sub_cap = cap // ops.BIN_SUBCURSORS
            res[f'texbin_reduce_kernel ({tag} pass)'] = (t(reduce), 64 * int(cursor_t.clamp(max=sub_cap).sum()))  # record write + read
            BIN_STATS[tag] = {'records_per_fragment_slot': round(float(cursor_t.float().sum() / (B * P * K)), 4), 'bins': bins[2],
                              'subranges_overflowed': int((cursor_t > sub_cap).sum()), 'capacity': cap, 'subranges_per_bin': ops.BIN_SUBCURSORS}
    return res


def cpu_baseline(args):
    """The CPU oracle (oracle/: C rasteriser + torch-CPU for the rest) timed on this box's host cores on a bounded sample
    of the SAME workload.  kind = 'port': the reference's own path needs PyTorch3D, which cannot be installed here."""
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import oracle as O
    cores = min(os.cpu_count() or 1, 64)
    torch.set_num_threads(cores)
    nv = 4
    m = O.OracleDBW((args.H, args.W), n_blocks=args.blocks, txt_size=args.txt, faces_per_pixel=args.fpp, seed=227391)
    R, T, K = O.synthetic_cameras(args.views, R_world=m.R_world[0])
    g = torch.Generator().manual_seed(0)
    inp = dict(imgs=torch.rand(nv, 3, args.H, args.W, generator=g), R=R[:nv], T=T[:nv], K=K[:nv])

    def it():
        for v in m.p.values():
            v.grad = None
        loss = m.forward(inp, training=True, coarse=True, decimate=True, opacity_noise=torch.randn(args.blocks, generator=g),
                         overlap_points=torch.rand(args.blocks, 1000, 3, generator=g), n_threads=cores)
        loss['total'].backward()
    # (`inp`, `cores`, `nv` are rebound below for the single-thread variant: `it` reads them at call time)
    it()
    t0, n = time.time(), 0
    while n < 3 or (time.time() - t0 < 10 and n < 20):
        it()
        n += 1
    dt = (time.time() - t0) / n
    out = {'value': nv / dt, 'unit': 'views/s', 'cores': cores, 'kind': 'port',
           'sample': f'{n} fwd+bwd iterations of {nv} views of the same config (oracle/: OpenMP C rasteriser on {cores} threads + '
                     f'torch-CPU sampling/blend/losses/autograd), {dt:.2f} s/iter'}
    # the "PyTorch3D-faithful" variant -- the naive CPU rasteriser is single-threaded per image in PyTorch3D, so
    # the same iteration on ONE thread, one view (bounded: one warm-up + one timed iteration)
    torch.set_num_threads(1)
    inp = {k: v[:1] for k, v in inp.items()}
    cores, nv = 1, 1
    it()
    t0 = time.time()
    it()
    dt1 = time.time() - t0
    torch.set_num_threads(min(os.cpu_count() or 1, 64))
    out['single_thread'] = {'value': 1 / dt1, 'unit': 'views/s', 'cores': 1,
                            'sample': f'1 fwd+bwd iteration of 1 view, 1 thread (naive rasteriser as PyTorch3D runs it on CPU), {dt1:.2f} s'}
    return out


def roofline_report(args, step, model, inp, global_count, restore, world, views_per_s, bytes_per_view):
    """`roofline` of the result line (--full): the dominant kernel of the step, HIP-event timed, against the HBM roofline."""
    P = args.H * args.W
    # the kernels of an iteration in exactly the form the step launches them (the fg forward WITH the env layer folded into it, the
    # composite + MSE epilogue, tiled images): the step's own HIP events around its four big kernels, once with everything in order on ONE
    # stream (every kernel alone on the GPU: `frac`), once as the step really runs (side streams next to them: `frac_in_step`)
    K_ = args.fpp
    B_ = inp['R'].shape[0]
    fg_bytes, env_bytes = (20 * P * K_ + 16 * P) * B_, (20 * P + 16 * P) * B_
    if step.cstep is not None and world == 1:
        restore()
        alone = step.cstep.kernel_times(inp, global_count, alone=True)
        folded = alone['env_fwd'] < 0.03 and (step.cstep.fuse & 18) == 18          # no env pass of its own between its two events (an empty pair reads ~5 us)
        name_of = {'env_fwd': 'render_fwd_fused K=1 (env pass)',
                   'fg_fwd': f'render_fwd_fused K={K_} (fg pass' + (' + folded env layer)' if folded else ')'),
                   'fg_bwd': f'render_bwd_fused K={K_} (fg pass)', 'env_bwd': 'render_bwd_fused K=1 (env pass)'}
        # algorithmic bytes per launch (zbuf not materialised): a pass writes 20 P K of fragments + 16 P of image and its
        # backward reads them back; the folded forward does the env pass's writes (K = 1) too
        nbytes_of = {'env_fwd': env_bytes, 'fg_fwd': fg_bytes + (env_bytes if folded else 0), 'fg_bwd': fg_bytes, 'env_bwd': env_bytes}
        kb = {name_of[k]: (v, nbytes_of[k]) for k, v in alone.items() if not (k == 'env_fwd' and folded)}
        restore()
        kt = step.cstep.kernel_times(inp, global_count)
        in_step = {name_of[k]: round(v, 4) for k, v in kt.items() if not (k == 'env_fwd' and folded)}
        restore()
    else:
        kb, in_step = kernel_breakdown(model, inp), None
    order = sorted(kb, key=lambda k: -kb[k][0])
    dom = order[0]
    ms, nbytes = kb[dom]
    achieved = nbytes / (ms * 1e-3) / 1e9

    def kernel_line(k):
        t, nb_ = kb[k]
        return {'kernel': k, 'avg_ms_per_launch': t, 'algorithmic_bytes_per_launch': nb_, 'achieved': nb_ / (t * 1e-3) / 1e9,
                'frac': nb_ / (t * 1e-3) / 1e9 / HBM_PEAK_GBS,
                'avg_ms_in_step': None if not in_step else in_step.get(k),
                'frac_in_step': None if not in_step or not in_step.get(k) else nb_ / (in_step[k] * 1e-3) / 1e9 / HBM_PEAK_GBS}
    # counter evidence for the dominant kernel from the rocprofv3 PMC passes of this same workload (profiles/, see its _how):
    # HBM bytes per launch (FETCH_SIZE / WRITE_SIZE with the gfx950 correction) and the SQ issue counters
    traffic, counters, counters_note = None, None, None
    sha = csrc_sha16()
    try:
        pmc = json.load(open(os.path.join(ROOT, 'profiles', PMC_FILE)))
        pmc_key = next((k for k in pmc if not k.startswith('_') and k.split(' (')[0] == dom.split(' (')[0] and ('fg' in k) == ('fg' in dom)), None)
        if inp['R'].shape[0] == 49 and (args.H, args.W, args.fpp, args.blocks, args.txt, args.epoch) == (300, 400, 10, 10, 256, 0) and pmc_key:
            if pmc.get('_csrc_sha16') == sha:
                traffic, counters = pmc[pmc_key].get('hbm_bytes'), {k: v for k, v in pmc[pmc_key].items() if k != 'hbm_bytes'}
            else:       # counters of another build of the kernels say nothing about this one
                counters_note = f'profiles/{PMC_FILE} was collected on csrc {pmc.get("_csrc_sha16")}, this library is built from {sha}: not reported'
    except (OSError, ValueError, KeyError):
        pmc = {}
    # ... and the HBM bytes measured live, in child processes of this run (N = 1, headline workload; --no-live-counters: the committed value only)
    traffic_source = None if traffic is None else f'profiles/{PMC_FILE} (committed; keyed on csrc_sha16)'
    default_workload = inp['R'].shape[0] == 49 and (args.H, args.W, args.fpp, args.blocks, args.txt, args.epoch) == (300, 400, 10, 10, 256, 0)
    profiled = 'rocprof' in os.environ.get('LD_PRELOAD', '') or any(k.startswith(('ROCPROF', 'ROCP_')) for k in os.environ)       # (no profiler inside a profiler)
    if world == 1 and default_workload and not (args.no_live_counters or args.no_extras or profiled) and step.cstep is not None:
        cal = pmc.get('_calibration') if isinstance(pmc, dict) else None
        cal = {'fetch': float(cal['fetch']), 'write': float(cal['write'])} if cal and 'fetch' in cal and 'write' in cal else {'fetch': 2.0, 'write': 1.0}
        torch.cuda.synchronize()
        live, note = live_traffic(dom, cal)
        if live is not None:
            committed = traffic
            traffic, traffic_source = live, note + ('' if committed is None else f'; the committed passes (profiles/{PMC_FILE}) read {committed} B')
        else:
            traffic_source = (traffic_source or 'none') + f' (live collection: {note})'
    return {'bound': 'hbm', 'kernel': dom, 'achieved': achieved, 'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': achieved / HBM_PEAK_GBS,
            'traffic': traffic, 'traffic_frac': None if traffic is None else traffic / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
            'traffic_source': traffic_source,
            'avg_ms_per_launch': ms, 'algorithmic_bytes_per_launch': nbytes,
            # frac: the kernel alone on the GPU, launched by the step itself in order on one stream (HIP events recorded by the
            # step); frac_in_step: the same launch where it really runs, sharing the GPU with the env backward chain and the
            # regularisers on their side streams
            'frac_in_step': None if not in_step or not in_step.get(dom) else nbytes / (in_step[dom] * 1e-3) / 1e9 / HBM_PEAK_GBS,
            'top_kernels': [kernel_line(k) for k in order[:2]],
            'measured_as': 'dbw_train_step_profile: the kernels the training step launches, in the form it launches them' if in_step is not None
                           else 'operator-level launches from Python (tools form: fg forward without the folded env layer)',
            'all_kernels_ms_in_step': in_step,
            'all_kernels_ms': {k: round(v[0], 4) for k, v in kb.items()}, 'texbins': BIN_STATS or None,
            'whole_path_frac': views_per_s / world * bytes_per_view / 1e9 / HBM_PEAK_GBS,
            'counters': counters, 'csrc_sha16': sha,
            'counters_source': counters_note if counters is None else f'profiles/{PMC_FILE}: separate rocprofv3 --pmc passes of this '
                               'workload on this build (tools/pmc_sq.sh), committed -- NOT measured in this run (a counter pass '
                               'serialises the kernels); avg_ms_per_launch, achieved and frac ARE measured in this run (HIP events)',
            'limiter': 'instruction issue and latency, not HBM: see `counters` (share of the SIMD time the VALU is busy, lane '
                       f'utilisation, HBM traffic per launch; profiles/{PMC_FILE}) and DESIGN.md section 4; frac is the '
                       'share of the HBM roofline the ALGORITHMIC bytes reach, traffic_frac the share the measured bytes reach'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    # 20 steps from the freshly initialised scene: the synthetic targets are noise, so the optimiser fades and shrinks the blocks and
    # the workload gets lighter step by step (tools/diag/window_times.py: 1.21 -> 1.00 ms/step over 300 steps, flat with frozen
    # parameters) -- a long window would measure that drift, not the configuration
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--views', type=int, default=49, help='views per GPU per step (weak scaling)')
    ap.add_argument('--H', type=int, default=300)
    ap.add_argument('--W', type=int, default=400)
    ap.add_argument('--blocks', type=int, default=10)
    ap.add_argument('--fpp', type=int, default=10)
    ap.add_argument('--txt', type=int, default=256)
    ap.add_argument('--epoch', type=int, default=0, help='training phase to measure: 0 = coarse+decimated textures (default, the '
                    'configuration at the start of training), 800 = coarse, 1600 = fine (dbw.py:210-219, default.yml:15-16)')
    ap.add_argument('--scaling', choices=['auto', 'weak', 'strong'], default='auto', help='strong (default when --gpus > 1): --views in total, sharded '
                    'over the ranks = BASELINE config 3 as written (49 views -> 7,6,...,6), the weak form measured next to it in the same run; '
                    'weak: --views per GPU')
    ap.add_argument('--dump-outputs', metavar='DIR', help='after the timed steps, write what one more step from the seeded starting state '
                    'computes (loss values, parameters, gradient, Adam\'s moments) as DIR/<name>.npy')
    ap.add_argument('--full', action='store_true', help='after the timed steps, measure everything reported next to the headline: the other '
                    'training phases, roofline, the all-reduce and the other scaling form (N > 1), the extra legs and the CPU baselines (N = 1)')
    ap.add_argument('--no-phases', action='store_true', help='with --full: skip the measurement of the two other training phases')
    ap.add_argument('--no-extras', action='store_true', help='with --full: skip the measurements reported next to the headline at N = 1: the reference\'s own '
                    'operating point (batch 4, loss values read every step), BASELINE configs 4 and 5 (per-GPU share) and the sustained run')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baselines')
    ap.add_argument('--no-live-counters', action='store_true', help='with --full: do not collect roofline.traffic in this run (two rocprofv3 --pmc '
                    'child processes, ~1 min at N = 1 on the headline workload): report the committed counters only')
    ap.add_argument('--backward-order', choices=['auto', 'sequential', 'concurrent'], default='auto', help='debug: the two backward kernels')
    ap.add_argument('--no-side-priority', action='store_true', help='debug: the side stream of the native step at normal priority')
    ap.add_argument('--no-overlap', action='store_true', help='everything in order on ONE stream: every kernel alone on the GPU (per-kernel averages of a '
                    'trace are then exact)')
    ap.add_argument('--launch-by-launch', action='store_true', help='the round-3 form of the step: ~33 launches issued one by one from Python '
                    '(dbw_amd/native_step.py) instead of one C-ABI call per iteration (dbw_train_step_run)')
    args = ap.parse_args()

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if not torch.cuda.is_available():
        raise RuntimeError('bench.py needs MI355X GPUs: the render path has no CPU implementation')
    if world != args.gpus:
        raise RuntimeError(f'--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}')
    # DBW_BENCH_BACKEND=gloo + DBW_BENCH_SHARE_GPU=1 let the N>1 code path be exercised on a single-GPU box (ranks share cuda:0,
    # gloo all-reduce); the measured configuration is always one rank per GPU over RCCL
    backend = os.environ.get('DBW_BENCH_BACKEND', 'nccl')
    dev_index = local_rank % torch.cuda.device_count() if os.environ.get('DBW_BENCH_SHARE_GPU') else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device('cuda', dev_index)
    if world > 1:
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=dev)
        else:
            dist.init_process_group(backend)
        # the communicator itself has to agree with the launch: --gpus ranks, one per process
        assert dist.get_world_size() == args.gpus and dist.get_rank() == rank, (dist.get_world_size(), args.gpus, dist.get_rank(), rank)

    from dbw_amd.parallel import ShardedTrainStep, shard_views
    if args.scaling == 'auto':
        args.scaling = 'strong' if world > 1 else 'weak'
    model, inp = build_workload(args, dev)
    model.set_cur_epoch(args.epoch)
    model.sync_free = True
    model.overlap_passes = not args.no_overlap
    inp_all = inp
    if args.scaling == 'strong':            # BASELINE config 3: the SAME views, split 7,6,...,6 over the ranks
        a, b = shard_views(args.views, world, rank)
        global_count = inp['imgs'].numel()
        inp = {k: v[a:b].contiguous() for k, v in inp.items()}
        views_total = args.views
    else:
        global_count = inp['imgs'].numel() * world
        views_total = args.views * world
    step = ShardedTrainStep(model, lr=5e-3, lr_texture=5e-2, seed=227391, use_c_step=not args.launch_by_launch)
    # every phase below is measured from the SAME state (freshly initialised parameters + its own warm-up), not from whatever the
    # previously measured phase left behind (opacities drift, blocks get filtered: the workload would change)
    if step.native is not None and args.backward_order != 'auto':
        step.native.sequential_backward = args.backward_order == 'sequential'
    if step.native is not None and args.no_side_priority:
        step.native.side_priority = False
    if step.native is not None and args.no_overlap:
        step.native.overlap_regularisers = False      # every kernel alone on one stream: per-kernel averages of a trace are then exact
    if step.cstep is not None:
        if args.no_overlap:
            step.cstep.use_side_stream = False
        if args.backward_order != 'auto':
            step.cstep.backward_order = int(args.backward_order == 'sequential')
    snapshot = (step.params.flat.clone(), step.exp_avg.clone(), step.exp_avg_sq.clone(), step.n_steps)

    def restore():
        step.params.flat.copy_(snapshot[0]); step.exp_avg.copy_(snapshot[1]); step.exp_avg_sq.copy_(snapshot[2])
        step.n_steps = snapshot[3]

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(n, inp=inp, global_count=global_count):
        """n steps bracketed by barrier + synchronize on both sides; MAX over ranks."""
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            out = step(inp, global_count=global_count)
        sync()
        dt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = t.item()
        return dt, out

    for _ in range(args.warmup):
        step(inp, global_count=global_count)
    dt, losses = timed(args.steps)
    total_loss = losses['total'].item()
    assert total_loss == total_loss, 'loss is NaN'
    if args.dump_outputs:
        # the dumped step is one more call of the timed path, from the seeded state the warm-up started from: the state the last timed step
        # started from is not the same from run to run (every step sums with unordered fp32 atomics, and the chained optimiser steps grow the
        # last-bit differences: tools/diag/dump_drift.py, profiles/dump_drift.txt), the state before the first one is.  The state after the
        # timed steps is put back for --full.
        after = (step.params.flat.clone(), step.exp_avg.clone(), step.exp_avg_sq.clone(), step.n_steps)
        restore()
        replay = step(inp, global_count=global_count)
        if rank == 0:
            dump_outputs(args.dump_outputs, model, step, replay)
        sync()
        step.params.flat.copy_(after[0]); step.exp_avg.copy_(after[1]); step.exp_avg_sq.copy_(after[2])
        step.n_steps = after[3]
        del replay, after

    # ---- outside the timed region (--full): the other two training phases of the same config, the all-reduce alone ----
    PHASES = (('epoch0', 0, 'coarse, decimated textures', 750), ('epoch800', 800, 'coarse, full-resolution textures', 750),
              ('epoch1600', 1600, 'fine', 300))          # default.yml:15-16,39: decimation until 750, coarse until 1500, 1800 epochs
    phases = None
    if args.full and not args.no_phases:
        phases = {}
        for name, epoch, what, n_ep in PHASES:
            if epoch == args.epoch:
                d, k = dt, args.steps
            else:
                restore()
                model.set_cur_epoch(epoch)
                for _ in range(max(args.warmup, 3)):
                    step(inp, global_count=global_count)
                k = max(5, min(args.steps, 10))
                d, _ = timed(k)
            phases[name] = {'what': what, 'epochs': n_ep, 'ms_per_step': d / k * 1e3, 'views_per_s': views_total * k / d}
        model.set_cur_epoch(args.epoch)
        step(inp, global_count=global_count)
        mean_ms = sum(p['ms_per_step'] * p['epochs'] for p in phases.values()) / sum(p['epochs'] for p in phases.values())
        phases['schedule_weighted'] = {'ms_per_step': mean_ms, 'views_per_s': views_total / mean_ms * 1e3,
                                       'what': 'mean over the 1800-epoch schedule (750 / 750 / 300 epochs)'}
    allreduce_ms, allreduce_bytes = None, None
    deferred = step.cstep is not None and step.defer_textures       # the ranks sum the prepared maps' gradient + the small gradients (parallel.py)
    if world > 1:
        bufs = [step.cstep.map_grads(), step.params.grad[:step.params.bounds[0][1]]] if deferred else None
        allreduce_bytes = sum(t.numel() * 4 for t in bufs) if deferred else step.params.flat.numel() * 4
    if args.full and world > 1:
        sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            if deferred:
                step._allreduce_all(bufs)
            else:
                step.allreduce_gradients()
        e1.record()
        torch.cuda.synchronize()
        allreduce_ms = e0.elapsed_time(e1) / 5
        step.params.zero_grad()
        if deferred:
            step.cstep.arena().zero_()

    # ---- N > 1: the other scaling form in the same run, and what the early slice of the all-reduce buys ----
    other_scaling, overlap_off_ms, flat_ms = None, None, None
    if args.full and world > 1:
        restore()
        model.set_cur_epoch(args.epoch)
        if args.scaling == 'strong':
            o_inp, o_count, o_views, o_name = inp_all, inp_all['imgs'].numel() * world, args.views * world, 'weak'
        else:
            a, b = shard_views(args.views, world, rank)
            o_inp, o_count, o_views, o_name = {k: v[a:b].contiguous() for k, v in inp_all.items()}, inp_all['imgs'].numel(), args.views, 'strong'
        for _ in range(max(args.warmup, 3)):
            step(o_inp, global_count=o_count)
        k = max(5, min(args.steps, 10))
        d, _ = timed(k, o_inp, o_count)
        other_scaling = {'scaling': o_name, 'value': o_views * k / d, 'unit': 'views/s', 'ms_per_step': d / k * 1e3, 'views_per_step': o_views,
                         'views_on_rank0': int(o_inp['R'].shape[0])}
        # the other data-parallel flow: the whole flat gradient buffer all-reduced, with and without its early slice overlapped
        was = step.defer_textures
        step.defer_textures = False
        if deferred:
            restore()
            for _ in range(max(args.warmup, 3)):
                step(inp, global_count=global_count)
            d, _ = timed(k)
            flat_ms = d / k * 1e3
        if step.overlap_allreduce:
            restore()
            step.overlap_allreduce = False
            for _ in range(max(args.warmup, 3)):
                step(inp, global_count=global_count)
            d, _ = timed(k)
            overlap_off_ms = d / k * 1e3
            step.overlap_allreduce = True
        step.defer_textures = was
        restore()
        step(inp, global_count=global_count)

    if rank == 0:
        phase = ('coarse phase (sigma=1e-4, opacity noise, decimated textures)' if model.is_live('decimate_txt') else
                 'coarse phase (sigma=1e-4, opacity noise, full-resolution textures)' if model.is_live('coarse_learning') else
                 'fine phase (sigma=5e-6, transparent blocks filtered, full-resolution textures)')
        views_per_s = views_total * args.steps / dt
        P = args.H * args.W
        bytes_per_view = 64 * P * args.fpp + 140 * P                      # whole-path algorithmic bytes
        roofline = None
        if args.full:
            roofline = roofline_report(args, step, model, inp, global_count, restore, world, views_per_s, bytes_per_view)
        local_views = inp['R'].shape[0]
        out = {
            'metric': 'rendered views/sec (fwd+bwd) per node, DTU 400x300 K=10 blocks', 'value': views_per_s, 'unit': 'views/s',
            'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': dt / args.steps * 1e3,
            'higher_is_better': True, 'scaling': args.scaling, 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
            'config': {'workload': f'DTU-scan24-like synthetic: ' + (f'{args.views} views/GPU/step' if args.scaling == 'weak' else
                                   f'{args.views} views/step sharded over {world} ranks ({local_views} on rank 0)') +
                                   f', {args.W}x{args.H}, {args.blocks} superquadric '
                                   f'blocks + ground + sky dome, faces_per_pixel={args.fpp}, {args.txt}^2 textures, {phase}, '
                                   f'MSE+parsimony+TV+overlap, Adam; LPIPS excluded',
                       'views_per_gpu': local_views, 'views_per_step': views_total, 'image_hw': [args.H, args.W], 'n_blocks': args.blocks,
                       'faces_per_pixel': args.fpp, 'txt_size': args.txt,
                       'launch': ('one C-ABI call per iteration (dbw_train_step_run: ~18 launches enqueued from C)' if step.cstep is not None else
                                  'launch by launch from Python, no host sync in the iteration') +
                                 ('' if args.no_overlap else ', env backward chain and regularisers on side streams' +
                                  ((' that wait through HIP events' if step.cstep.sync_events else ' that wait through polled words in device memory') if step.cstep is not None else '')) +
                                 ('' if step.native is None else ', native step (no autograd)'),
                       'parallelism': 'one GPU: all views on it, no collective' if world == 1 else f'view-sharded dp{world}, ' + (
                           f'{(allreduce_bytes or 0) / 1e6:.2f} MB all-reduced per step over RCCL: the gradient of the prepared texture maps (sigmoid + '
                           f'decimation are linear behind it) + the small gradients, instead of the {step.params.flat.numel() * 4 / 1e6:.1f} MB gradient buffer'
                           if deferred else
                           f'{step.params.flat.numel() * 4 / 1e6:.1f} MB of gradients all-reduced per step over RCCL'
                           + (' (blocks\' textures overlapped with the env backward, the rest after it)' if step.overlap_allreduce else '')),
                       'nranks': dist.get_world_size() if world > 1 else 1},
            'roofline': roofline,
            'phases': phases, 'allreduce_ms': allreduce_ms, 'allreduce_path': getattr(step, 'allreduce_path', None), 'other_scaling': other_scaling, 'ms_per_step_overlap_allreduce_off': overlap_off_ms, 'ms_per_step_flat_allreduce': flat_ms, 'allreduce_bytes': allreduce_bytes,
            'final_loss': total_loss,
            # polls between the step's streams that gave up (dbw_train_step_sync_timeouts): anything but 0 voids the run
            'sync_timeouts': step.cstep.sync_timeouts() if step.cstep is not None and step.cstep._cur is not None else None,
        }
        if args.full and world == 1 and not args.no_extras:
            default = (args.views, args.H, args.W, args.blocks, args.fpp, args.txt, args.epoch) == (49, 300, 400, 10, 10, 256, 0)
            if default:
                del step, model, inp
                torch.cuda.empty_cache()
                # the reference's operating point: configs/dtu/default.yml:28 trains with batch_size 4 and src/trainer.py:143 reads every
                # loss value on the host each iteration
                def best_of(n, *a, **k):
                    # (the small-batch numbers are 0.3 ms windows on a shared box: a run that catches another tenant's burst or a clock ramp
                    # reads 2x; the lowest of n runs, all kept, the median next to it)
                    runs = [measure_other(*a, **k) for _ in range(n)]
                    best = min(runs, key=lambda r: r['ms_per_step'])
                    best['runs_ms_per_step'] = [round(r['ms_per_step'], 4) for r in runs]
                    best['median_ms_per_step'] = sorted(best['runs_ms_per_step'])[len(runs) // 2]
                    return best
                out['batch4'] = best_of(3, 4, 300, 400, 10, 10, 256, dev, steps=200, warmup=20, read_losses=True)
                out['batch4']['what'] = ('batch_size 4 (configs/dtu/default.yml:28), the loss values on the host after every step '
                                         '(src/trainer.py:143): one C-ABI call per iteration, the step copies its loss values itself')
                out['batch4_no_reads'] = best_of(3, 4, 300, 400, 10, 10, 256, dev, steps=200, warmup=20, read_losses=False)
                out['batch7'] = best_of(3, 7, 300, 400, 10, 10, 256, dev, steps=200, warmup=20, read_losses=True)
                out['batch7']['what'] = 'the largest per-rank batch of BASELINE config 3 (49 views over 8 ranks: 7,6,...,6), loss values read every step'
                # the round-3 form of the same step for comparison: ~33 launches issued one by one from Python, six scalar reads
                out['batch4_launch_by_launch'] = measure_other(4, 300, 400, 10, 10, 256, dev, steps=100, warmup=10, read_losses=True, c_step=False)
                out['perceptual'] = measure_perceptual(dev)
                # >= 2 s of steps from the initial scene with frozen parameters (learning rates 0: Adam runs, the workload does not drift)
                out['sustained'] = measure_other(49, 300, 400, 10, 10, 256, dev, steps=200, warmup=10, lr_scale=0.0, min_seconds=2.0)
                out['sustained']['what'] = '>= 2 s of steps of the headline workload with both learning rates 0 (the scene does not drift)'
                # BASELINE configs 4 and 5, the share of ONE GPU (31 views on 4 GPUs -> 8; 200 views on 8 GPUs -> 25)
                out['configs'] = {
                    'c4': measure_other(8, 576, 768, 20, 16, 256, dev, steps=20, warmup=3),
                    'c5': measure_other(25, 1080, 1920, 50, 16, 512, dev, steps=5, warmup=2),
                }
                out['configs']['c4']['what'] = 'BASELINE config 4 (BlendedMVS-like, 31 views, 768x576, K=20, fpp 16, 4 GPUs): the 8 views of one GPU'
                out['configs']['c5']['what'] = 'BASELINE config 5 (Nerfstudio-like, 200 views, 1080x1920, K=50, 512^2 textures, fpp 16, 8 GPUs): the 25 views of one GPU'
                # ... and their full-resolution phase (epoch 800: texel gradients through the texture bins, sub-ranges sized by demand)
                for name, cfg_, st_ in (('c4', (8, 576, 768, 20, 16, 256), 20), ('c5', (25, 1080, 1920, 50, 16, 512), 5)):
                    r = measure_other(*cfg_, dev, steps=st_, warmup=3, epoch=800)
                    out['configs'][name]['full_resolution_phase'] = {k: r[k] for k in ('ms_per_step', 'views_per_s', 'whole_path_frac', 'steps')}
        if args.full and world == 1 and not args.no_cpu_baseline:
            out['cpu_baseline'] = cpu_baseline(args)
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
