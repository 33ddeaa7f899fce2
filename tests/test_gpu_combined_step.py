"""GPU tests of ONE step with every optional training term on (DESIGN.md "The combined step against float64"), `-m gpu`: validity masks, the
SSIM term, per-view exposure, pose refinement, intrinsics refinement, the surface term and the free-space term in one forward and one
backward, held to the float64 reference of tests/combined_ref.py -- whose preconditions tests/test_combined_step_host.py checks on the CPU.

Bars.  No new tolerance: loss values 1e-5 relative (tests/test_gpu_exposure.py), total against the sum of its entries 1e-5
(tests/test_gpu_surface.py), gradients REL = 1e-4 of the reference's largest element (tests/test_gpu_model.py), the 3D terms' values one
element-wise bar of surface_ref.bars, and ORDER_ULPS = 8 units in the last place of a tensor's largest element wherever the same work is
summed in another order (tests/test_gpu_pose.py); two runs of one optimisation are held to tests/trajectory.py."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import combined_ref as CR                                       # noqa: E402
import oracle as O                                              # noqa: E402
import surface_ref as SR                                        # noqa: E402
import dbw_amd                                                  # noqa: E402
from dbw_amd import _lib, intrinsics, ops, parallel, phase, pose  # noqa: E402
from dbw_amd.trainer import Trainer                             # noqa: E402
from trajectory import assert_same_trajectory                   # noqa: E402

DEV = 'cuda:0'
H, W, NB = CR.H, CR.W, CR.NB
REL, ORDER_ULPS, PARAMS = CR.REL, CR.ORDER_ULPS, CR.PARAMS
ULP = 2.0 ** -23
KEYS = ['rgb', 'perceptual', 'parsimony', 'tv', 'overlap', 'surface', 'freespace', 'total']
POSE_GRAD, K_GRAD = 'dbw_lens_pose_grad', 'dbw_lens_intrinsics_grad'
CHAINS = ('dbw_lens_pose_chain', 'dbw_lens_intrinsics_chain')
TERM_CALLS = ('dbw_eval_surface_fwd', 'dbw_eval_surface_bwd', 'dbw_eval_freespace_fwd', 'dbw_eval_freespace_bwd')


def rel_err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max() / b.detach().abs().max().clamp(min=1e-12))


def _model(terms3d=True, size=(H, W), rig='smoke'):
    torch.manual_seed(CR.SEED)
    model = dbw_amd.create_model(CR.model_cfg(True, terms3d), size).to(DEV).train()
    c = CR.case(rig)
    model._overlap_u_override = c['u'].to(DEV)
    if terms3d:
        assert model.set_surface_points(c['cloud'].to(DEV)) == len(c['cloud'])
        assert model.set_freespace_rays(c['ends'].to(DEV), c['frame'].to(DEV), c['origins'].to(DEV)) == len(c['ends'])
        assert model.surface_cfg['back'] == CR.BACK and model.freespace_cfg['margin'] == CR.MARGIN and model.surface_cfg['ground']
    model._rng_step = CR.STEP                                    # (what the trainer's step sets: parallel.py)
    return model


class Setup:
    """The all-on case on the device: the three refiners at their non-trivial values and the batch builder."""

    def __init__(self, identity=False, rig='smoke'):
        c = self.c = CR.case(rig)
        self.pose = pose.PoseRefiner(CR.N_ROWS, DEV)
        self.intr = intrinsics.IntrinsicsRefiner(c['K0'], DEV, focal='separate', principal=True)
        self.theta = (torch.zeros(CR.N_ROWS, 6) if identity else c['exposure']).to(DEV).requires_grad_(True)
        if not identity:
            with torch.no_grad():
                self.pose.flat.copy_(c['delta'].reshape(-1).to(DEV))
                self.intr.flat.copy_(c['ktheta'].to(DEV))
        self.masks = torch.ones_like(c['masks']) if identity else c['masks']
        self.base = {k: c[k].to(DEV) for k in ('imgs', 'R', 'T', 'K')}
        self.base.update(masks=self.masks.to(DEV), mask_sum=float(self.masks.double().sum()), view_ids=torch.tensor(c['rows'], device=DEV),
                         view_ids_host=torch.tensor(c['rows']))

    def batch(self):
        """A fresh all-on batch (a backward frees the graph of the last one): R, T through the pose refiner, K_live through the intrinsics
        refiner, the exposure table; R', T', K' keep their gradients."""
        b = self.intr.apply(self.pose.apply(self.base))
        b['exposure'] = self.theta
        for k in ('R', 'T', 'K_live'):
            b[k].retain_grad()
        return b

    def zero(self, model):
        model.zero_grad(set_to_none=True)
        self.pose.grad.zero_()
        self.intr.grad.zero_()
        self.theta.grad = None


def _recorder():
    argtypes = dict(_lib.SIGNATURES)
    for f in _lib.FAMILIES.values():
        argtypes.update(f.signatures)
    calls, call = [], _lib.call

    def recording(name, *args):
        calls.append((name,) + tuple(a for a, t in zip(args, argtypes[name]) if t is not _lib.c_p))
        return call(name, *args)
    return calls, call, recording


def _run(model, s, what, batch=None):
    """One forward and one backward of what(losses) on a fresh batch -> (losses, gradients: the ten parameters and, as R1, T1, K1, delta,
    exposure, ktheta, those of R', T', K' and of the three tables -- a tensor no gradient reached reads as zeros --, the library calls of
    the forward and the backward, the batch)."""
    s.zero(model)
    b = s.batch() if batch is None else batch
    calls, call, recording = _recorder()
    _lib.call = recording
    try:
        out = model(b)
        what(out).backward()
        torch.cuda.synchronize()
    finally:
        _lib.call = call
    z = lambda g, like: torch.zeros_like(like) if g is None else g.detach().clone()        # noqa: E731
    grads = {k: z(getattr(model, k).grad, getattr(model, k)) for k in PARAMS}
    if batch is None:
        grads.update(R1=z(b['R'].grad, b['R']), T1=z(b['T'].grad, b['T']), K1=z(b['K_live'].grad, b['K_live']),
                     delta=s.pose.grad.view(CR.N_ROWS, 6).clone(), exposure=z(s.theta.grad, s.theta), ktheta=s.intr.grad.clone())
    return {k: v.detach().clone() for k, v in out.items()}, grads, calls, b


# ---------------------------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize('rig', sorted(CR.RIGS, reverse=True))
def test_every_term_on_equals_the_float64_sum_of_the_terms(rig, record_property):
    """Measured on an MI355X: the table of DESIGN.md "The combined step against float64" (printed below, and recorded as properties).
    `smoke`: the cameras of smoke(), which look down on the blocks and the ground.  `horizon`: the rig of tests/test_gpu_env_backward.py with
    the horizon across the view -- half of every image is the sky dome, whose vertices are constants but which moves in the image with the
    camera: its part of the camera and K gradients is in the oracle's, and has to be in the step's."""
    c = CR.case(rig)
    model, s = _model(rig=rig), Setup(rig=rig)
    everything = lambda o: o['total']                                                       # noqa: E731
    _run(model, s, everything)                                  # (a first call differs from later ones: the texture bins have no demand yet)
    # the plain masked + exposure step at the same cameras: no refiner in the graph, no 3D term in the model
    b = s.batch()
    plain = dict(s.base, R=b['R'].detach(), T=b['T'].detach(), K_live=b['K_live'].detach(), exposure=s.theta)
    weights = model.loss_weights
    model.loss_weights = {k: v for k, v in weights.items() if k not in ('surface', 'freespace')}
    try:
        out_p, _, calls_p, _ = _run(model, s, everything, batch=plain)
    finally:
        model.loss_weights = weights
    out, g_tot, calls, b = _run(model, s, everything)
    # ---- the reference: the device's cameras, vertices and opacities on the CPU
    R1, T1, K1 = (b[k].detach().cpu() for k in ('R', 'T', 'K_live'))
    sc = CR.term_scene(model._surface_ground_v, model._surface_block_v, *[model._surface_tables(NB, True, DEV)[i] for i in (0, 1, 2, 4)])
    alpha = model._alpha.detach().cpu().double().numpy()
    with torch.no_grad():
        verts_at = {'env': model.build_env_scene().verts.cpu(), 'blocks': model.build_blocks_scene(filter_transparent=False).verts.cpu()}
    orc = CR.oracle()
    ref = CR.reference(orc, c['imgs'], R1, T1, K1, c['masks'], c['exposure'], c['rows'], c['u'], verts_at=verts_at,
                       factor=phase.phase_of(model, True).perceptual_factor)
    ref['delta'] = CR.delta_grad64(c['R'], c['T'], c['delta'], c['rows'], ref['R'], ref['T'])
    ref['ktheta'] = CR.ktheta_grad64(c['K0'], c['ktheta'], ref['K'])
    ref.update(R1=ref['R'], T1=ref['T'], K1=ref['K'], exposure=ref['theta'])
    surf64 = CR.surface_value64(sc, c['cloud'], alpha)
    free64 = CR.freespace_value64(sc, c['ends'], c['frame'], c['origins'], alpha)
    total64 = ref['total_img'] + surf64 + free64
    # ---- the loss dict
    assert list(out) == KEYS and list(out_p) == [k for k in KEYS if k not in ('surface', 'freespace')]
    v = {k: float(x) for k, x in out.items()}
    print('losses: ' + ', '.join(f'{k} {x:.9f}' for k, x in v.items()))
    print(f"float64: rgb {ref['rgb']:.9f}, perceptual {ref['perceptual']:.9f}, regs {ref['regs']}, surface {surf64:.9f}, freespace {free64:.9f}, total {total64:.9f}")
    assert abs(v['total'] - sum(x for k, x in v.items() if k != 'total')) < 1e-5
    for k, r in (('rgb', ref['rgb']), ('perceptual', ref['perceptual']), ('total', total64)):
        e = abs(v[k] - r) / abs(r)
        record_property(f'value_{k}', f'{e:.2e}')
        print(f'   {k}: rel err {e:.2e}')
        assert e <= 1e-5, (k, v[k], r)
    for k, r in ref['regs'].items():                            # (the regularisers: implied by the total's bar, asserted at it one by one)
        assert abs(v[k] - r) <= 1e-5 * abs(total64), (k, v[k], r)
    for k, r in (('surface', surf64), ('freespace', free64)):
        e = SR.bars(v[k], r)
        record_property(f'value_{k}_bars', round(e, 4))
        print(f'   {k}: {e:.4f} bars')
        assert r > 0 and e <= 1.0, (k, v[k], r)
    # ---- the camera-side gradients of the one backward of `total`
    cams = ('R1', 'T1', 'K1', 'delta', 'exposure', 'ktheta')
    for k in cams:
        e = rel_err(g_tot[k], ref[k])
        record_property(f'grad_{k}', f'{e:.2e}')
        print(f'   {k}.grad: rel err {e:.2e} (max {float(ref[k].abs().max()):.3e})')
        assert e < REL, (k, e)
    outside = [i for i in range(CR.N_ROWS) if i not in c['rows']]
    assert not g_tot['K1'][2].any()
    assert not g_tot['delta'][outside].any() and not g_tot['exposure'][outside].any()
    assert bool(g_tot['delta'][c['rows']].all()) and bool(g_tot['exposure'][c['rows']].all())
    # ---- the ten parameter gradients: image terms and regularisers against the oracle, the 3D terms by additivity
    out_i, g_img, _, _ = _run(model, s, lambda o: o['total'] - o['surface'] - o['freespace'])
    for k in PARAMS + cams:
        e = rel_err(g_img[k], ref['params'][k] if k in PARAMS else ref[k])
        if k in PARAMS:
            record_property(f'grad_{k}', f'{e:.2e}')
        print(f'   {k}.grad without the 3D terms: rel err {e:.2e}')
        assert e < REL, (k, e)
    _, g_s, _, _ = _run(model, s, lambda o: o['surface'])
    _, g_f, _, _ = _run(model, s, lambda o: o['freespace'])
    for k in cams:                                              # the 3D terms see neither a camera nor an exposure
        assert not g_s[k].any() and not g_f[k].any(), k
    assert any(bool(g_s[k].any()) for k in PARAMS) and any(bool(g_f[k].any()) for k in PARAMS)
    for k in PARAMS:
        parts = [g_img[k], g_s[k], g_f[k]]
        room = ORDER_ULPS * ULP * sum(float(p.abs().max()) for p in parts)
        e = float((g_tot[k].double() - sum(p.double() for p in parts)).abs().max())
        record_property(f'additivity_{k}', f'{e / max(room, 1e-300):.3f}')
        print(f'   {k}: total against the sum of its three parts {e:.2e} (room {room:.2e})')
        assert e <= room, (k, e, room)
    # ---- the work enqueued: the plain masked + exposure step, plus the camera gradients, the chains and the 3D terms
    added = (POSE_GRAD, K_GRAD) + CHAINS + TERM_CALLS
    assert not any(x[0] in added for x in calls_p) and calls_p
    # (one argument differs: the env pass's backward skips the geometry gradient of the sky dome's faces -- constant vertices -- unless a camera or K
    # gradient sums over them: const_faces 0 in place of the dome's face count)
    BWD = 'dbw_render_bwd_fused'
    domeless = lambda cs: [x[:-2] + (0,) + x[-1:] if x[0] == BWD else x for x in cs]        # noqa: E731
    assert domeless([x for x in calls if x[0] not in added]) == domeless(calls_p)
    assert {x[-2] for x in calls if x[0] == BWD} == {0} and {x[-2] for x in calls_p if x[0] == BWD} == {0, model._n_bkg_faces}
    assert [x[-1] for x in calls if x[0] == POSE_GRAD] == [0, 0] and [x[-1] for x in calls if x[0] == K_GRAD] == [0, 0]
    names = [x[0] for x in calls if x[0] in CHAINS + TERM_CALLS]
    assert sorted(names) == sorted(CHAINS + TERM_CALLS), names
    for x in calls:                                             # both 3D terms are numbered by the step the trainer set: (.., seed, step, ..)
        if x[0] in TERM_CALLS:
            assert (CR.SEED, CR.STEP) in list(zip(x[1:], x[2:])), x


# ---------------------------------------------------------------------------------------------------------------- b
def test_identity_refiners_and_unit_masks_change_nothing():
    c = CR.case()
    s = Setup(identity=True)
    # zero refinements return their inputs bit for bit
    b = s.batch()
    assert torch.equal(b['R'], s.base['R']) and torch.equal(b['T'], s.base['T']) and torch.equal(b['K_live'], s.base['K'][0])
    model = _model(terms3d=False)
    seen, node = [], ops.composite_mse_exposure
    ops.composite_mse_exposure = lambda *a, **k: (seen.append(1), node(*a, **k))[1]
    try:
        _run(model, s, lambda o: o['total'])                    # (the first call: the texture bins have no demand yet)
        out1, g1, calls1, _ = _run(model, s, lambda o: o['total'])
        n_exposed = len(seen)
        bare = dict(s.base)
        for k in ('view_ids', 'view_ids_host'):
            bare.pop(k)
        out0, g0, calls0, _ = _run(model, s, lambda o: o['total'], batch=bare)
    finally:
        ops.composite_mse_exposure = node
    assert n_exposed == 2 and len(seen) == 2                    # the `exposure` branch of _forward, and only for the all-on batch
    assert any(x[0] == 'dbw_monitor_exposure_composite' for x in calls1) and not any(x[0] == 'dbw_monitor_exposure_composite' for x in calls0)
    assert list(out1) == list(out0) == [k for k in KEYS if k not in ('surface', 'freespace')]
    for k in out0:
        e = abs(float(out1[k]) - float(out0[k])) / abs(float(out0[k])) if float(out0[k]) != 0 else abs(float(out1[k]))
        print(f'{k}: {float(out1[k]):.9e} with identity refiners, {float(out0[k]):.9e} bare ({e:.1e})')
        assert e <= 1e-6, k
    for k in PARAMS:
        e = rel_err(g1[k], g0[k])
        print(f'   {k}: {e:.1e}{" (same bits)" if torch.equal(g1[k], g0[k]) else ""}')
        assert e <= ORDER_ULPS * ULP, k
    assert float(g1['delta'].abs().max()) > 0 and float(g1['ktheta'].abs().max()) > 0      # (the refiners were in the graph)


# ---------------------------------------------------------------------------------------------------------------- c
def test_each_camera_gradient_is_the_same_alone_and_in_company():
    """project_clip_bwd, project_clip_bwd_cam and project_clip_bwd_k walk the same g_fvc and the same clipped slots one after the other.  On
    the saved inputs of the env pass and of the fg pass of one all-on backward: the camera and K gradients (no float atomics,
    csrc/camera_grad.hip) are the same bits whether a walk runs alone, first or last, the vertex gradient (atomics) agrees within
    ORDER_ULPS, and no walk writes to g_fvc or to the clip tables."""
    model, s = _model(), Setup()
    _run(model, s, lambda o: o['total'])
    saved, orig = [], ops.project_clip_bwd

    def spy(verts, faces, R, T, Kmat, cl, g_fvc, *rest):
        saved.append((verts, faces, R, T, Kmat, cl, g_fvc.clone(), rest))
        return orig(verts, faces, R, T, Kmat, cl, g_fvc, *rest)
    ops.project_clip_bwd = spy
    try:
        _run(model, s, lambda o: o['total'])
    finally:
        ops.project_clip_bwd = orig
    assert len(saved) == 2 and {a[1].shape[0] for a in saved} == {NB * SR.BNF, model.env_n_faces}      # the fg pass and the env pass
    for verts, faces, R, T, Kmat, cl, g, rest in saved:
        name = 'fg' if faces.shape[0] == NB * SR.BNF else 'env'
        assert bool(g.any()) and R.shape[0] == 2
        tables = {k: cl[k].clone() for k in ('num_faces', 'c2o', 'clip_code', 'clip_w', 'face_verts')}
        g_in = g.clone()
        args = (verts, faces, R, T, Kmat, cl, g) + rest
        cam = lambda: tuple(t.clone() for t in ops.project_clip_bwd_cam(*args))            # noqa: E731
        kk = lambda: ops.project_clip_bwd_k(*args).clone()                                 # noqa: E731
        vv = lambda: ops.project_clip_bwd(*args).clone()                                   # noqa: E731
        alone = dict(cam=cam(), k=kk(), v=vv())
        first = {}
        first['cam'], first['k'], first['v'] = cam(), kk(), vv()                           # cam -> K -> verts
        last = {}
        last['v'], last['k'], last['cam'] = vv(), kk(), cam()                              # verts -> K -> cam
        torch.cuda.synchronize()
        for other in (first, last):
            assert torch.equal(other['cam'][0], alone['cam'][0]) and torch.equal(other['cam'][1], alone['cam'][1]), name
            assert torch.equal(other['k'], alone['k']), name
            assert rel_err(other['v'], alone['v']) <= ORDER_ULPS * ULP, name
        bits = lambda t: t.contiguous().view(torch.int32)                                  # noqa: E731  (slots behind num_faces are never written: any bytes, NaN patterns too)
        assert torch.equal(bits(g), bits(g_in)) and all(torch.equal(bits(cl[k]), bits(t)) for k, t in tables.items()), name
        assert bool(alone['cam'][0].any()) and bool(alone['cam'][1].any()) and bool(alone['k'].any()) and not alone['k'][2].any(), name
        print(f"{name}: g_R, g_T, g_K the same bits alone, first and last; g_verts within {max(rel_err(first['v'], alone['v']), rel_err(last['v'], alone['v'])) / ULP:.2f} ulp")


# ---------------------------------------------------------------------------------------------------------------- d
def test_both_render_passes_see_the_live_K():
    model, s = _model(), Setup()
    b = s.batch()
    K_live = b['K_live'].detach()
    b = dict(b, R=b['R'].detach(), T=b['T'].detach(), K_live=K_live)

    def layers():
        with torch.no_grad():
            fg, env = model.render_layers(b)
        return fg.clone(), env.clone()

    def without_K(renderer):
        orig = renderer.render_packed
        renderer.render_packed = lambda *a, **k: orig(*a, **dict(k, Kmat=None))
        try:
            return layers()
        finally:
            del renderer.render_packed                          # (the instance attribute: the class's method is back)
    fg, env = layers()
    fg2, env2 = layers()
    assert torch.equal(fg, fg2) and torch.equal(env, env2)       # the forward render has no atomics
    assert model.renderer is not model.renderer_env and not torch.equal(K_live, model.renderer.cameras.K[0].to(DEV))
    fg_e, env_e = without_K(model.renderer_env)
    assert torch.equal(fg_e, fg) and not torch.equal(env_e, env)
    fg_f, env_f = without_K(model.renderer)
    assert torch.equal(env_f, env) and not torch.equal(fg_f, fg)
    # ... and each is the renderer's own output at the live matrix
    with torch.no_grad():
        env_d = model.renderer_env.render_packed(model.build_env_scene(), b['R'], b['T'], lds_aggregate=True, Kmat=K_live)
        blocks = model.build_blocks_scene(filter_transparent=False)
        fg_d = model.renderer.render_packed(blocks, b['R'], b['T'], faces_alpha=model._alpha.repeat_interleave(model.BNF), Kmat=K_live)
        env_0 = model.renderer_env.render_packed(model.build_env_scene(), b['R'], b['T'], lds_aggregate=True)
    assert torch.equal(env_d, env) and torch.equal(fg_d, fg) and torch.equal(env_0, env_e)
    print(f'env differs in {int((env_e != env).sum())} values without the live K, fg in {int((fg_f != fg).sum())}')


# ---------------------------------------------------------------------------------------------------------------- e
TH, TW, TV = 24, 32, 6


def _capture(root):
    """tests/depth_fixture.py's capture of 6 frames of 24 x 32 with depth maps, and mask files written the way
    tests/test_gpu_masked_scene.py writes them: an 8-bit PNG per frame under masks/, named by the frame's mask_path."""
    import depth_fixture as DF
    from PIL import Image
    DF.write_depth_capture(root, 'cap', H=TH, W=TW, n=TV)
    folder = os.path.join(str(root), 'custom', 'cap')
    os.makedirs(os.path.join(folder, 'masks'))
    with open(os.path.join(folder, 'transforms.json')) as f:
        meta = json.load(f)
    for i, frame in enumerate(meta['frames']):
        a = np.full((TH, TW), 255, np.uint8)
        a[6 + i:15 + i, 3 * i:3 * i + 9] = 0                    # a shadow that moves with the frame
        frame['mask_path'] = f'masks/mask_{i + 1:05d}.png'
        Image.fromarray(a, 'L').save(os.path.join(folder, frame['mask_path']))
    with open(os.path.join(folder, 'transforms.json'), 'w') as f:
        json.dump(meta, f)


def _full_cfg():
    model = CR.model_cfg(True, True)['model']
    model['mesh']['n_blocks'] = 2
    model['loss'].update(surface={'points': 64, 'tau': 0.5, 'start_epoch': 1}, freespace={'rays': 64, 'tau': 0.5, 'start_epoch': 2})
    return {'dataset': {'name': 'custom', 'tag': 'cap', 'cloud': 'depth', 'masks': True}, 'model': model,
            'training': {'batch_size': 2, 'n_epoches': 3, 'seed': 3, 'optimizer': {'name': 'adam', 'lr': 1e-3}, 'scheduler': {'name': 'multi_step'},
                         'pose_refine': {'lr': 1e-4, 'start_epoch': 1}, 'exposure': {'lr': 1e-3, 'start_epoch': 2},
                         'intrinsics_refine': {'lr': 1e-4, 'start_epoch': 2, 'focal': 'separate', 'principal': True}}}


def _full_trainer(root):
    """What dbw_amd.train.main builds for the config, in this process: the scene with masks and the depth cloud, the model with the cloud and
    the rays, the Trainer with the three refiners."""
    from dbw_amd import dataset as DS
    from dbw_amd import train
    cfg = _full_cfg()
    torch.manual_seed(cfg['training']['seed'])
    scene, _, _ = DS.create_train_val_test(cfg, str(root), DEV)
    train.resolve_depth_cloud(scene, DEV)
    model = dbw_amd.create_model(cfg, scene.img_size).to(DEV).train()
    assert train.resolve_surface(scene, model, DEV) > 0 and train.resolve_freespace(scene, model, DEV) > 0
    model._overlap_u_override = torch.rand(2, 1000, 3, generator=torch.Generator().manual_seed(1)).to(DEV)      # (a resumed run: the same samples)
    tr = Trainer(cfg, model, scene.views(DEV))
    tr.scene = scene
    return tr


def test_the_trainer_runs_every_option_at_once_and_resumes(tmp_path, monkeypatch):
    _capture(tmp_path)
    full = _full_trainer(tmp_path)
    assert len(full.scene) == TV and 'masks' in full.views and full.mask_sums is not None and full.n_batches == 3
    assert float(full.views['masks'].min()) == 0.0 and full.pose is not None and full.exposure is not None and full.intrinsics is not None
    seen, step = [], parallel.ShardedTrainStep.__call__
    monkeypatch.setattr(parallel.ShardedTrainStep, '__call__', lambda self, batch, **k: seen.append((self, batch)) or step(self, batch, **k))
    c_steps, c_iter = [], parallel.ShardedTrainStep._c_iteration
    monkeypatch.setattr(parallel.ShardedTrainStep, '_c_iteration', lambda self, inp: c_steps.append(self) or c_iter(self, inp))
    lasts = [{k: float(v) for k, v in full.run_epoch(shuffle=False).items()} for _ in range(3)]
    torch.cuda.synchronize()
    mine = [b for st, b in seen if st is full.step_fn]
    assert len(mine) == 9 and not c_steps                        # masks and the 3D terms: the general path, every step
    for e, last in enumerate(lasts, 1):
        print(f'epoch {e}: ' + ', '.join(f'{k} {v:.6f}' for k, v in last.items()))
        assert list(last) == KEYS and all(np.isfinite(v) for v in last.values())
        assert last['surface'] > 0 and (last['freespace'] == 0.0 if e < 2 else last['freespace'] > 0)
    for i, b in enumerate(mine):
        epoch = i // 3 + 1
        assert 'masks' in b and 'mask_sum' in b and 'view_ids' in b and b['R'].requires_grad                      # pose_refine from epoch 1
        assert ('exposure' in b) == (epoch >= 2) and ('K_live' in b) == (epoch >= 2)
    # each refiner stepped once per batch since its start_epoch
    assert full.pose.n_steps == 9 and full.exposure.n_steps == 6 and full.intrinsics.n_steps == 6 and full.step_fn.n_steps == 9
    assert bool(full.pose.flat.any()) and bool(full.exposure.flat.any()) and bool(full.intrinsics.flat.any())
    sd = full.state_dict()
    assert sd['pose_refine']['n_steps'] == 9 and sd['exposure']['n_steps'] == 6 and sd['intrinsics_refine']['n_steps'] == 6
    assert sd['epoch'] == 3
    # the refined-camera files (the two evaluation walks stubbed: they are not what is tested here)
    monkeypatch.setattr(full.model, 'qualitative_eval', lambda loader, device, path=None, **kw: None)
    monkeypatch.setattr(full.model, 'quantitative_eval', lambda loader, device, hard_inference=True: {'PSNR': 1.0})
    full.evaluate([], tmp_path / 'run')
    for name in ('transforms_refined.json', 'intrinsics_refined.yml', 'exposures.tsv'):
        assert (tmp_path / 'run' / name).exists(), name
    with open(tmp_path / 'run' / 'transforms_refined.json') as f:
        refined = json.load(f)
    with open(tmp_path / 'custom' / 'cap' / 'transforms.json') as f:
        src = json.load(f)
    assert refined['fl_x'] != src['fl_x'] and refined['cx'] != src['cx']
    moved = [float(np.abs(np.asarray(r['transform_matrix']) - np.asarray(q['transform_matrix'])).max()) for r, q in zip(refined['frames'], src['frames'])]
    print('largest change of a transform_matrix entry per frame:', ['%.2e' % x for x in moved])
    print('delta:', full.pose.flat.view(TV, 6).tolist())
    assert len(moved) == TV and all(np.isfinite(x) and 0 < x < 0.1 for x in moved)      # every training view's pose moved a little
    # 2 epochs, a checkpoint into a fresh Trainer, 1 epoch: the straight run
    first = _full_trainer(tmp_path)
    for _ in range(2):
        first.run_epoch(shuffle=False)
    ckpt = first.state_dict()
    resumed = _full_trainer(tmp_path)
    resumed.load_state_dict(ckpt)
    assert resumed.epoch == 3 and resumed.step_fn.n_steps == 6 and resumed.pose.n_steps == 6 and resumed.exposure.n_steps == 3 and resumed.intrinsics.n_steps == 3
    for a, b in ((resumed.pose, first.pose), (resumed.exposure, first.exposure), (resumed.intrinsics, first.intrinsics)):
        assert torch.equal(a.flat, b.flat) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    last = resumed.run_epoch(shuffle=False)
    torch.cuda.synchronize()
    assert list(last) == KEYS and float(last['freespace']) > 0
    assert_same_trajectory(resumed.step_fn.params.flat, full.step_fn.params.flat, lr_max=1e-3)
    for a, b in ((resumed.pose, full.pose), (resumed.exposure, full.exposure), (resumed.intrinsics, full.intrinsics)):
        print(f'{type(a).__name__}: largest difference to the straight run {float((a.flat - b.flat).abs().max()):.2e} at lr {a.lr:g}')
        assert_same_trajectory(a.flat, b.flat, lr_max=a.lr)
        assert a.n_steps == b.n_steps
    assert resumed.step_fn.n_steps == full.step_fn.n_steps == 9


# ---------------------------------------------------------------------------------------------------------------- f
LH, LW = 12, 16


def _late_trainer(general_path):
    """The SSIM-term model without masks and without 3D terms -- the one-call C step is eligible -- on 6 synthetic views of 12 x 16, with the
    three refiners starting in epoch 2.  general_path: the C step and the native step taken away from the start."""
    model = _model(terms3d=False, size=(LH, LW))
    R, T, Km = O.synthetic_cameras(TV, R_world=O.world_rotation(115, 0, 0))
    g = torch.Generator().manual_seed(4)
    views = {k: v.to(DEV) for k, v in dict(imgs=torch.rand(TV, 3, LH, LW, generator=g), R=R, T=T, K=Km).items()}
    cfg = {'training': {'batch_size': 2, 'n_epoches': 2, 'seed': 3, 'optimizer': {'name': 'adam', 'lr': 5e-3, 'texture': {'lr': 5e-2}},
                        'scheduler': {'name': 'multi_step'}, 'pose_refine': {'lr': 1e-4, 'start_epoch': 2},
                        'exposure': {'lr': 1e-2, 'start_epoch': 2},
                        'intrinsics_refine': {'lr': 1e-4, 'start_epoch': 2, 'focal': 'separate', 'principal': True}}}
    tr = Trainer(cfg, model, views)
    if general_path:
        tr.step_fn.cstep = tr.step_fn.native = None
    return tr


def test_a_refiner_that_starts_later_takes_over_from_the_c_step(monkeypatch):
    c_steps, c_iter = [], parallel.ShardedTrainStep._c_iteration
    monkeypatch.setattr(parallel.ShardedTrainStep, '_c_iteration', lambda self, inp: c_steps.append(self) or c_iter(self, inp))
    arena_checks, begin = [], ops.ARENA.begin_step

    def checked_begin(device):
        begin(device)
        buf = ops.ARENA.buf.get(torch.device(device) if not isinstance(device, torch.device) else device)
        if ops.ARENA.enabled and buf is not None:
            arena_checks.append(bool((buf == 0).all()))          # what the step carves its zero-initialised scratch from
    monkeypatch.setattr(ops.ARENA, 'begin_step', checked_begin)
    mixed = _late_trainer(False)
    assert mixed.step_fn.cstep is not None and mixed.step_fn.cstep.supported()
    mixed.run_epoch(shuffle=False)
    assert len(c_steps) == 3 and all(st is mixed.step_fn for st in c_steps) and not arena_checks      # epoch 1: the one-call C step
    assert mixed.step_fn.n_steps == 3 and mixed.pose.n_steps == mixed.exposure.n_steps == mixed.intrinsics.n_steps == 0
    mixed.run_epoch(shuffle=False)
    torch.cuda.synchronize()
    assert len(c_steps) == 3 and len(arena_checks) == 3 and all(arena_checks)      # epoch 2: the autograd iteration, on a clean zero arena from its first step
    assert mixed.step_fn.n_steps == 6 and mixed.pose.n_steps == mixed.exposure.n_steps == mixed.intrinsics.n_steps == 3
    del arena_checks[:]
    general = _late_trainer(True)
    for _ in range(2):
        general.run_epoch(shuffle=False)
    torch.cuda.synchronize()
    assert len(c_steps) == 3 and len(arena_checks) == 6 and all(arena_checks) and general.step_fn.n_steps == 6
    a, b = mixed.step_fn, general.step_fn
    for t in (a.params.flat, a.exp_avg, a.exp_avg_sq, b.params.flat, b.exp_avg, b.exp_avg_sq):
        assert bool(torch.isfinite(t).all())
    assert_same_trajectory(a.params.flat, b.params.flat, lr_max=5e-2)
    # the moments are of the gradients' size, not of a step's: each tensor scaled by its largest element, then the same rule
    for name in ('exp_avg', 'exp_avg_sq'):
        x, y = getattr(a, name), getattr(b, name)
        assert float(y.abs().max()) > 0
        print(f'{name}: largest difference {float((x - y).abs().max() / y.abs().max()):.2e} of the largest element')
        assert_same_trajectory(x / y.abs().max(), y / y.abs().max(), lr_max=5e-2)
    for ra, rb in ((mixed.pose, general.pose), (mixed.exposure, general.exposure), (mixed.intrinsics, general.intrinsics)):
        assert ra.n_steps == rb.n_steps == 3 and bool(torch.isfinite(ra.flat).all()) and bool(ra.flat.any()) and bool(rb.flat.any())
        for m in (ra.exp_avg, ra.exp_avg_sq, rb.exp_avg, rb.exp_avg_sq):
            assert bool(torch.isfinite(m).all())
