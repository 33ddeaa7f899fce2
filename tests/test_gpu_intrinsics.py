"""GPU tests of the intrinsics refinement, `-m gpu`: dbw_lens_intrinsics_grad against the host build of the same header
(tests/intrinsics_ref.py, itself held to autograd of the oracle on the CPU by tests/test_host_intrinsics_math.py) and against the oracle's
autograd, dbw_lens_intrinsics_apply / dbw_lens_intrinsics_chain at the values of the host tests, K.grad of the model's two render nodes against
the oracle model, an intrinsics-only refinement that has to reduce a known error, and one run of the command line with --intrinsics-refine.

Bars (tests/intrinsics_ref.py says where each comes from): kernel against host build n * 2^-23 * sum|terms| (two fp32 sums of the same terms in
different orders); against the oracle's autograd 1e-4 * max|g_K|; apply / chain 4 x torch's own fp32 error, floor 1e-6 relative, against
float64; the model's K.grad rel_err < 1e-4 like the parameter gradients of tests/test_gpu_model.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle as O                                              # noqa: E402
import intrinsics_ref as IR                                     # noqa: E402
import pose_ref as PR                                           # noqa: E402
import dbw_amd                                                  # noqa: E402
from custom_fixture import write_capture                        # noqa: E402
from dbw_amd import _lib, intrinsics, ops, train                # noqa: E402
from dbw_amd.parallel import ShardedTrainStep                   # noqa: E402

DEV = 'cuda:0'
GUARD, PAD = 0xA5, 64
REL = 1e-4                                                      # tests/test_gpu_model.py


def rel_err(a, b):
    return float((a.cpu() - b.cpu()).abs().max() / b.abs().max().clamp(min=1e-12))


class Guarded:
    """`nbytes` of device memory between PAD bytes of GUARD on each side (4-byte aligned); check() after the kernels ran."""

    def __init__(self, nbytes, fill=None):
        self.n = nbytes
        self.buf = torch.full((nbytes + 2 * PAD,), GUARD, dtype=torch.uint8, device=DEV)
        self.mem = self.buf[PAD:PAD + nbytes]
        assert self.mem.data_ptr() % 4 == 0
        if fill is not None:
            self.mem.view(torch.float32).copy_(fill.reshape(-1))

    def floats(self, *shape):
        return self.mem.view(torch.float32).view(*shape)

    def check(self):
        host = self.buf.cpu()
        assert bool((host[:PAD] == GUARD).all()) and bool((host[PAD + self.n:] == GUARD).all()), 'a byte outside the buffer was written'


def _k_grad(dv, cl, g, B, V, F_, persp, accumulate=0, into=None):
    """dbw_lens_intrinsics_grad on device tensors with grad_K and the workspace between guard bytes -> g_K (4,4) on the CPU."""
    ws_bytes = int(_lib.family('lens').dbw_lens_intrinsics_grad_workspace_bytes(B, F_))
    assert ws_bytes == B * ((2 * F_ + 255) // 256) * 12 * 4
    ws = Guarded(ws_bytes)
    gK = Guarded(64, fill=into)
    _lib.call('dbw_lens_intrinsics_grad', dv['verts'].data_ptr(), dv['faces'].data_ptr(), dv['R'].data_ptr(), dv['T'].data_ptr(), dv['K'].data_ptr(), B, V,
              F_, 1e-8, IR.ZC, int(persp), cl['num_faces'].data_ptr(), cl['c2o'].data_ptr(), cl['clip_code'].data_ptr(), cl['clip_w'].data_ptr(),
              g.data_ptr(), ws.mem.data_ptr(), ws_bytes, gK.mem.data_ptr(), int(accumulate), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for x in (ws, gK):
        x.check()
    return gK.floats(4, 4).cpu().clone()


def _case(B, F_, seed=4):
    """The icosphere scene of the host tests seen by B cameras, its first F_ faces; with B > 1 the last view looks away from everything (every
    face behind the near plane).  F_ = 1, 2: the faces are chosen so that the first one is clipped in view 0."""
    verts, faces, R, T, Kmat = PR.scene(seed, B=B)
    if B > 1:
        R[B - 1], T[B - 1] = torch.eye(3), torch.tensor([0.0, 0.0, -10.0])
    if F_ < faces.shape[0]:
        cl = PR.host_project_clip(verts, faces, R[:1].contiguous(), T[:1].contiguous(), Kmat, IR.ZC, True)
        j = int((cl['clip_code'][0, :int(cl['num_faces'][0])] >= 0).nonzero()[0])
        f = int(cl['c2o'][0, j])
        faces = torch.cat([faces[f:f + 1], faces[:f], faces[f + 1:]])[:F_].contiguous()
    return verts, faces, R.contiguous(), T.contiguous(), Kmat


@pytest.mark.parametrize('persp', [True, False])
@pytest.mark.parametrize('B,F_', [(1, 320), (3, 320), (65, 320), (3, 1), (3, 2), (65, 2), (1, 1), (65, 1), (1, 2)])
def test_k_grad_against_the_host_build_and_the_oracle(B, F_, persp):
    verts, faces, R, T, Kmat = _case(B, F_)
    V = verts.shape[0]
    dv = {k: v.to(DEV) for k, v in dict(verts=verts, faces=faces, R=R, T=T, K=Kmat).items()}
    cl = ops.project_clip(dv['verts'], dv['faces'], dv['R'], dv['T'], dv['K'], 1e-8, IR.ZC, persp)
    clh = {k: v.cpu() for k, v in cl.items()}
    num = clh['num_faces']
    if B > 1:
        assert int(num[B - 1]) == 0                                        # the view that looks away
    if F_ == 320:
        kinds = {int(k) for b in range(B) for k in (clh['clip_code'][b, :int(num[b])] >> 2).unique()}
        assert kinds == {-1, 0, 1, 2}
    gen = torch.Generator().manual_seed(1)
    g = torch.randn(B, 2 * F_, 3, 3, generator=gen)
    g[:, 3::5] = 0.0                                                       # slots whose nine components are all zero skip the projection
    gpu_g = g.clone()
    for b in range(B):
        gpu_g[b, int(num[b]):] = 1e30                                      # what lies behind num_faces must not reach the result
    gd = gpu_g.to(DEV)
    gK = _k_grad(dv, cl, gd, B, V, F_, persp)
    # the host build of the same header: the derived bound of two fp32 sums of the same terms, added over the views
    hK, hKv, abs_terms, n_terms, _ = IR.host_intrinsics_grad(verts, faces, R, T, Kmat, clh, g, IR.ZC, persp)
    bound = IR.k_bound(n_terms, abs_terms)
    err = (gK.double() - hK.double()).abs().reshape(-1)
    print(f'B={B} F={F_} persp={persp}: vs host g_K {float(err.max()):.3e} (smallest nonzero bound '
          f'{float(bound[bound > 0].min()) if bool((bound > 0).any()) else 0.0:.3e})')
    assert bool((err <= bound + 2.0 ** -24 * hK.double().abs().reshape(-1)).all())          # (+ the one rounding of the fp64 total to fp32)
    assert not gK[2].any()                                                 # row 2: exactly 0
    if B > 1:
        assert not hKv[B - 1].any() and int(n_terms[B - 1]) == 0           # the view without faces contributes exactly 0 ...
        if B == 3 and F_ == 320:                                           # ... on the device too: without it, the same bits
            sub = {k: (v[:B - 1].contiguous() if k in ('R', 'T') else v) for k, v in dv.items()}
            cl_sub = {k: v[:B - 1].contiguous() for k, v in cl.items()}
            assert torch.equal(_k_grad(sub, cl_sub, gd[:B - 1].contiguous(), B - 1, V, F_, persp), gK)
    # the oracle's autograd
    rK, _ = IR.oracle_k_grad(verts, faces, R, T, Kmat, g, IR.ZC, persp)
    print(f'   vs oracle g_K {float((gK - rK).abs().max()):.3e} (max {float(rK.abs().max()):.3e})')
    assert float((gK - rK).abs().max()) <= 1e-4 * float(rK.abs().max())
    # two identical calls: the same bits
    assert torch.equal(gK, _k_grad(dv, cl, gd, B, V, F_, persp))
    # accumulate: a second pass with other gradients is added to the first (one fp64 add, one rounding: |acc - (r1 + r2)| <= 2^-23 (|r1| + |r2|))
    g2d = torch.randn(B, 2 * F_, 3, 3, generator=gen).to(DEV)
    sK = _k_grad(dv, cl, g2d, B, V, F_, persp)
    aK = _k_grad(dv, cl, g2d, B, V, F_, persp, accumulate=1, into=gK)
    assert bool(((aK.double() - (gK.double() + sK.double())).abs() <= 2.0 ** -23 * (gK.double().abs() + sK.double().abs())).all())
    # ... and through ops: the one buffer of the env and fg passes
    oK = ops.project_clip_bwd_k(dv['verts'], dv['faces'], dv['R'], dv['T'], dv['K'], cl, gd, 1e-8, IR.ZC, persp)
    assert torch.equal(oK.cpu(), gK)
    pK = ops.project_clip_bwd_k(dv['verts'], dv['faces'], dv['R'], dv['T'], dv['K'], cl, g2d, 1e-8, IR.ZC, persp, out=oK)
    assert pK is oK and torch.equal(pK.cpu(), aK)


def test_k_grad_validates_its_arguments():
    verts, faces, R, T, Kmat = _case(3, 2)
    dv = {k: v.to(DEV) for k, v in dict(verts=verts, faces=faces, R=R, T=T, K=Kmat).items()}
    cl = ops.project_clip(dv['verts'], dv['faces'], dv['R'], dv['T'], dv['K'], 1e-8, IR.ZC, True)
    g = torch.zeros(3, 4, 3, 3, device=DEV)
    out, ws = torch.zeros(16, device=DEV), torch.zeros(64, device=DEV)
    lib = _lib.family('lens')
    assert lib.dbw_lens_intrinsics_grad_workspace_bytes(0, 5) == 0 and lib.dbw_lens_intrinsics_grad_workspace_bytes(3, 2) == 3 * 12 * 4

    def call(B=3, F_=2, ws_ptr=ws.data_ptr(), ws_bytes=144, gK=out.data_ptr()):
        _lib.call('dbw_lens_intrinsics_grad', dv['verts'].data_ptr(), dv['faces'].data_ptr(), dv['R'].data_ptr(), dv['T'].data_ptr(), dv['K'].data_ptr(), B,
                  verts.shape[0], F_, 1e-8, IR.ZC, 1, cl['num_faces'].data_ptr(), cl['c2o'].data_ptr(), cl['clip_code'].data_ptr(),
                  cl['clip_w'].data_ptr(), g.data_ptr(), ws_ptr, ws_bytes, gK, 0, None)
    call()
    call(B=0, ws_ptr=None, ws_bytes=0)                                     # no views: OK, nothing launched
    with pytest.raises(RuntimeError, match='workspace'):
        call(ws_bytes=143)
    with pytest.raises(RuntimeError, match='workspace'):
        call(ws_ptr=None)
    with pytest.raises(RuntimeError, match='aligned'):
        call(ws_ptr=ws.data_ptr() + 2)
    with pytest.raises(RuntimeError, match='null'):
        call(gK=None)
    with pytest.raises(RuntimeError, match='bad size'):
        call(B=-1)
    with pytest.raises(RuntimeError, match='overflows'):
        call(B=65535, F_=1 << 20)                                          # B*2F past int32: refused before the workspace is looked at
    for name, args in (('dbw_lens_intrinsics_apply', (None, out.data_ptr(), out.data_ptr(), None)),
                       ('dbw_lens_intrinsics_chain', (dv['K'].data_ptr(), out.data_ptr(), None, out.data_ptr(), None))):
        with pytest.raises(RuntimeError, match='null'):
            _lib.call(name, *args)
    torch.cuda.synchronize()


# ---- apply / chain ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('value', IR.THETAS, ids=[f'{v:g}' for v in IR.THETAS])
def test_apply_and_chain_at_the_values_of_the_host_tests(value):
    theta, gK = IR.theta_case(value, 11)
    ref = IR.intrinsics_reference(IR.K0, theta, gK)
    th = theta.to(DEV).requires_grad_(True)
    K1 = ops.intrinsics_apply(IR.K0.to(DEV), th)
    (K1 * gK.to(DEV)).sum().backward()
    K1, gt = K1.detach().cpu(), th.grad.cpu()
    hK, hg = IR.host_intrinsics_apply(IR.K0, theta), IR.host_intrinsics_chain(IR.K0, theta, gK)
    eK, eg = float((K1.double() - ref['K']).abs().max()), float((gt.double() - ref['g']).abs().max())
    same = torch.equal(K1, hK) and torch.equal(gt, hg)
    print(f'theta={value:g}: K err {eK:.2e} (bar {ref["tol_K"]:.2e}), g_theta err {eg:.2e} (bar {ref["tol_g"]:.2e}); host build: '
          f'{"same bits" if same else "max diff %.2e" % max(float((K1 - hK).abs().max()), float((gt - hg).abs().max()))}')
    assert eK <= ref['tol_K'] and eg <= ref['tol_g']
    # against the host build: expf comes from two libraries, so the bar each build is held to against float64 -- except at theta = 0, where
    # no library function is called and K0 comes back bit for bit
    assert float((K1.double() - hK.double()).abs().max()) <= ref['tol_K'] and float((gt.double() - hg.double()).abs().max()) <= ref['tol_g']
    if value == 0.0:
        assert torch.equal(K1, IR.K0) and same


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
H, W, NB, TS, FPP = 32, 48, 3, 16, 4                             # the geometry of __graft_entry__.smoke()
PARAMS = ('sq_eps', 'S', 'R_6d', 'T', 'alpha_logit', 'R_6d_ground', 'T_ground', 'texture_bkg', 'texture_ground', 'textures')
ORDER_ULPS = 8                                                   # tests/test_gpu_pose.py: the room of reordered float atomic sums
GRAD = 'dbw_lens_intrinsics_grad'


def _smoke_cfg():
    return {'model': {'name': 'dbw', 'mesh': {'n_blocks': NB, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': TS},
                      'renderer': {'faces_per_pixel': FPP, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                      'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True,
                                     'opacity_noise': False},
                      'loss': {'rgb_weight': 1, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}}}


def _smoke_model():
    torch.manual_seed(227391)
    model = dbw_amd.create_model(_smoke_cfg(), (H, W)).to(DEV).train()
    orc = O.OracleDBW((H, W), n_blocks=NB, txt_size=TS, faces_per_pixel=FPP, seed=227391)
    R, T, Km = O.synthetic_cameras(2, R_world=orc.R_world[0])
    g = torch.Generator().manual_seed(0)
    imgs, u = torch.rand(2, 3, H, W, generator=g), torch.rand(NB, 1000, 3, generator=g)
    model._overlap_u_override = u.to(DEV)
    return model, orc, dict(imgs=imgs, R=R, T=T, K=Km), u


def _model_grads(model, inp, k_grad):
    """One forward + backward of the model -> (losses, the ten parameter gradients, K_live.grad, the library calls it made).  A call is
    recorded as its name and every argument that is not a pointer: sizes, flags, scales -- what decides the work a launch does."""
    model.zero_grad(set_to_none=True)
    d = {k: v.to(DEV) for k, v in inp.items()}
    if k_grad:
        d['K_live'] = d['K'][0].clone().requires_grad_(True)
    argtypes = dict(_lib.SIGNATURES)
    for f in _lib.FAMILIES.values():
        argtypes.update(f.signatures)
    calls, call = [], _lib.call

    def recording(name, *args):
        calls.append((name,) + tuple(a for a, t in zip(args, argtypes[name]) if t is not _lib.c_p))
        return call(name, *args)
    _lib.call = recording
    try:
        out = model(d, None)
        out['total'].backward()
        torch.cuda.synchronize()
    finally:
        _lib.call = call
    return out, {k: getattr(model, k).grad.clone() for k in PARAMS}, (d['K_live'].grad if k_grad else None), calls


@pytest.mark.parametrize('path', ['decoupled_mse', 'render_scene'])
def test_model_k_gradient_matches_the_oracle_model(path):
    """K.grad of the model's total loss against autograd of the oracle model with inp['K'] requiring a gradient (orc.forward keeps
    inp['K'][0] attached: asserted below), through ops._DecoupledRenderMSE (default criteria) and through ops._RenderScene (masks of ones),
    and: asking for it leaves the ten parameter gradients alone, asserted the way tests/test_gpu_pose.py does -- the call with a live K makes
    the library calls of the call without, in the same order with the same sizes, flags and scales, plus one dbw_lens_intrinsics_grad per
    render pass (accumulate flags [0, 1] for the decoupled node, [0, 0] for the general one), and both calls' parameter gradients are held
    to the oracle's and to one another within 8 units in the last place of a tensor's largest element."""
    model, orc, inp, u = _smoke_model()
    if path == 'render_scene':                                   # masks of ones: the general path (ops._RenderScene), the same loss
        inp = dict(inp, masks=torch.ones(2, 1, H, W))
    seen = []
    node = ops._DecoupledRenderMSE if path == 'decoupled_mse' else ops._RenderScene
    iK = 9 if path == 'decoupled_mse' else 6
    orig = node.backward
    node.backward = staticmethod(lambda ctx, *a: (seen.append(tuple(ctx.needs_input_grad)), orig(ctx, *a))[1])
    try:
        _model_grads(model, inp, False)                          # (a first call differs from later ones: the texture bins have no demand yet)
        out0, grads0, none, calls0 = _model_grads(model, inp, False)
        n0 = len(seen)
        out1, grads1, gK, calls1 = _model_grads(model, inp, True)
    finally:
        node.backward = staticmethod(orig)
    assert seen and none is None and not any(s[iK] for s in seen[:n0]) and all(s[iK] for s in seen[n0:])      # the node under test ran, and was asked
    with torch.no_grad():
        verts_at = {'env': model.build_env_scene().verts.cpu(), 'blocks': model.build_blocks_scene(filter_transparent=False).verts.cpu()}
    oin = {k: v for k, v in inp.items() if k != 'masks'}
    oin['K'] = inp['K'].clone().requires_grad_(True)
    ref = orc.forward(oin, training=True, coarse=True, decimate=False, opacity_noise=None, overlap_points=u, n_threads=8, verts_at=verts_at)
    ref['total'].backward()
    assert oin['K'].grad is not None and bool(oin['K'].grad[0].any()) and not oin['K'].grad[1:].any()      # the oracle lets K[0] carry the gradient
    rK = oin['K'].grad[0]
    assert abs(out1['total'].item() - ref['total'].item()) <= REL * abs(ref['total'].item())
    eK = rel_err(gK, rK)
    print(f'{path}: K.grad rel err {eK:.2e} (max {float(rK.abs().max()):.3e})\n{gK.cpu()}\n{rK}')
    assert eK < REL and not gK[2].any()
    # the same launches with the same arguments, plus the K gradient of each render pass (env and fg)
    assert not any(c[0] == GRAD for c in calls0)
    extra = [c for c in calls1 if c[0] == GRAD]
    # (one argument differs: the env pass's backward skips the geometry gradient of the sky dome's faces -- constant vertices -- unless a camera
    # gradient sums over them, which moves in the image with the camera like every other face: const_faces 0 in place of the dome's face count)
    BWD = 'dbw_render_bwd_fused'
    domeless = lambda cs: [c[:-2] + (0,) + c[-1:] if c[0] == BWD else c for c in cs]        # noqa: E731
    assert domeless([c for c in calls1 if c[0] != GRAD]) == domeless(calls0) and len(extra) == 2
    assert {c[-2] for c in calls1 if c[0] == BWD} == {0} and {c[-2] for c in calls0 if c[0] == BWD} == {0, model._n_bkg_faces}
    assert [c[-1] for c in extra] == ([0, 1] if path == 'decoupled_mse' else [0, 0])      # one accumulating buffer / one per node
    for k in PARAMS:
        d01 = rel_err(grads1[k], grads0[k])
        print(f'   {k}: with against without the K gradient {d01:.1e}{" (same bits)" if torch.equal(grads0[k], grads1[k]) else ""}')
        assert rel_err(grads0[k], orc.p[k].grad) < REL and rel_err(grads1[k], orc.p[k].grad) < REL, k
        assert d01 <= ORDER_ULPS * 2.0 ** -23, k


REFINE_STEPS, REFINE_LR = 150, 1e-3


def _refinement_run(refine):
    model, orc, inp, u = _smoke_model()
    with torch.no_grad():                                        # textures with structure: an intrinsics error has something to show in
        gen = torch.Generator().manual_seed(9)
        for name in ('texture_bkg', 'texture_ground', 'textures'):
            p = getattr(model, name)
            low = torch.randn(p.shape[0], 3, 4, 4, generator=gen) * 2.0
            p.copy_(torch.nn.functional.interpolate(low, size=p.shape[1:3], mode='bilinear', align_corners=False).permute(0, 2, 3, 1).to(DEV))
    d = {k: v.to(DEV) for k, v in inp.items()}
    K_true = d['K'][0].clone()
    with torch.no_grad():
        fg, env = model.render_layers(d)                         # (freezes K_true on the renderers: the live matrix below stands in its place)
        target = ops.composite(fg, env)[:, :3].contiguous()
    # training starts from K0: the focal lengths 2 % off, the principal point 0.01 NDC off
    K0 = K_true.clone()
    K0[0, 0] *= 1.02
    K0[1, 1] *= 1.02
    K0[0, 2] += 0.01
    K0[1, 2] -= 0.01
    ref = intrinsics.IntrinsicsRefiner(K0, DEV, lr=REFINE_LR, focal='separate', principal=True)
    batch = dict(imgs=target, R=d['R'], T=d['T'], K=d['K'], K_live=K0)
    rgb, errs = [], [float((K0 - K_true).abs().max())]
    for _ in range(REFINE_STEPS):
        model.zero_grad(set_to_none=True)                        # (the model's parameters are not stepped)
        b = ref.apply(batch) if refine else batch
        out = model(b, None)
        out['total'].backward()
        if refine:
            ref.step()
        rgb.append(float(out['rgb']))
    errs.append(float((ref.refined() - K_true).abs().max()))
    return rgb, errs, ref.flat.cpu()


def test_intrinsics_only_steps_reduce_a_known_error():
    """Targets rendered by the model itself at K_true (smooth random textures, so that an error of K shows); training starts from K0 =
    K_true with both focal lengths 2 % too long and the principal point 0.01 NDC off.  150 intrinsics-only Adam steps at lr 1e-3 with
    focal: separate, principal: true: model(inp), backward, IntrinsicsRefiner.step(); the model's parameters are not stepped.
    Observed on an MI355X (profiles/intrinsics_refine.md): rgb loss 7.545e-04 -> 2.716e-05 (27.8 x lower); max|K' - K_true| 0.0964 ->
    0.0018 (53 x); theta (-0.01943, -0.02013, -0.01029, +0.00999) where the exact answer is (-0.01980, -0.01980, -0.01, +0.01).  The
    assertions ask for a decrease only: the margins are those factors."""
    rgb, (e0, e1), theta = _refinement_run(True)
    print(f'rgb loss {rgb[0]:.6e} -> {rgb[-1]:.6e} ({rgb[0] / rgb[-1]:.1f} x); max|K - K_true| {e0:.5f} -> {e1:.5f} ({e0 / e1:.1f} x); theta {theta.tolist()}')
    assert rgb[-1] < rgb[0]
    assert e1 < e0
    # without the refiner nothing moves: the loss is the same number at every step, so the decrease above is the feature's
    rgb_off, (f0, f1), _ = _refinement_run(False)
    assert rgb_off[0] == rgb[0] and all(v == rgb_off[0] for v in rgb_off) and f0 == f1


# ---- the command line -----------------------------------------------------------------------------------------------------------------------------
def test_the_command_line_refines_the_intrinsics_of_a_custom_scene(tmp_path):
    import json
    import yaml
    root = tmp_path / 'data'
    write_capture(root, 'desk', n=6, H=24, W=32, dist=(0.0,) * 6, with_points=True)
    cfg = {'dataset': {'name': 'custom', 'tag': 'desk', 'downscale_factor': 2},
           'model': {'name': 'dbw', 'mesh': {'n_blocks': 2, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': 16},
                     'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                     'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True,
                                    'opacity_noise': False},
                     'loss': {'rgb_weight': 1, 'perceptual_weight': 0.1, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}},
           'training': {'batch_size': 2, 'n_epoches': 3, 'seed': 3, 'optimizer': {'name': 'adam', 'lr': 1e-3}, 'scheduler': {'name': 'multi_step'}}}
    path = tmp_path / 'desk.yml'
    with open(path, 'w') as f:
        yaml.safe_dump(cfg, f)
    common = ['--config', str(path), '--tag', 'run', '--data-root', str(root), '--runs-root', str(tmp_path / 'runs'), '--no-perceptual',
              '--intrinsics-refine', '1e-4', '--device', DEV]
    scores = train.main(common + ['--epochs', '2'])
    assert all(np.isfinite(float(v)) for k, v in scores.items() if k != 'LPIPS' and not isinstance(v, dict)) and scores['PSNR'] > 0
    run_dir = tmp_path / 'runs' / 'custom' / 'run'
    with open(run_dir / 'intrinsics_refined.yml') as f:
        y = yaml.safe_load(f)
    th = y['theta']
    print('theta after 2 epochs:', th)
    assert th['a_x'] != 0.0 and th['a_x'] == th['a_y'] and th['c_x'] == 0.0 and th['c_y'] == 0.0 and abs(th['a_x']) < 0.01      # the default: one shared focal scale
    assert y['n_steps'] == 6 and y['transforms_refined'] is True                                   # 2 epochs x 3 batches; a pinhole capture at zoom 1
    with open(run_dir / 'transforms_refined.json') as f:
        refined = json.load(f)
    with open(root / 'custom' / 'desk' / 'transforms.json') as f:
        src = json.load(f)
    assert refined['fl_x'] / src['fl_x'] == pytest.approx(float(np.exp(th['a_x'])), rel=1e-5) and refined['cx'] == pytest.approx(src['cx'], abs=1e-4)
    assert refined['frames'] == src['frames']
    ckpt = torch.load(run_dir / 'model.pkl', map_location='cpu', weights_only=False)
    assert ckpt['epoch'] == 2 and ckpt['intrinsics_refine']['n_steps'] == 6 and bool(ckpt['intrinsics_refine']['theta'].any())
    # --resume restores the refiner
    train.main(common + ['--epochs', '3', '--resume'])
    again = torch.load(run_dir / 'model.pkl', map_location='cpu', weights_only=False)
    assert again['epoch'] == 3 and again['intrinsics_refine']['n_steps'] == 9


def test_refined_intrinsics_are_refused_under_two_ranks():
    model, orc, inp, u = _smoke_model()
    step = ShardedTrainStep(model, lr=0.0, lr_texture=0.0, seed=1)
    step.world_size = 2                                          # (what a second rank would make it: the refusal comes before any collective)
    d = {k: v.to(DEV) for k, v in inp.items()}
    d['K_live'] = d['K'][0].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match='intrinsics'):
        step(d)
