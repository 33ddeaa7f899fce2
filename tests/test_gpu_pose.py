"""GPU tests of the camera pose refinement, `-m gpu`: dbw_lens_pose_grad against the host build of the same header
(tests/pose_ref.py, itself held to autograd of the oracle on the CPU by tests/test_host_pose_math.py) and against the oracle's autograd,
dbw_lens_pose_apply / dbw_lens_pose_chain at the angles of the host tests, the camera gradients of the model's two render nodes against
the oracle model, a pose-only refinement that has to find a known perturbation, and one run of the command line with --pose-refine.

Bars (tests/pose_ref.py says where each comes from): kernel against host build n * 2^-23 * sum|terms| (two fp32 sums of the same terms in
different orders); against the oracle's autograd 1e-4 * max|grad|; apply / chain 4 x torch's own fp32 error, floor 1e-6 relative, against
float64; the model's R.grad, T.grad rel_err < 1e-4 like the parameter gradients of tests/test_gpu_model.py."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle as O                                              # noqa: E402
import pose_ref as PR                                           # noqa: E402
import lens_ref as LR                                           # noqa: E402
import dbw_amd                                                  # noqa: E402
from custom_fixture import write_capture                        # noqa: E402
from dbw_amd import _lib, ops, pose, train                      # noqa: E402
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


def _pose_grad(dv, cl, g, B, V, F_, persp, accumulate=0, into=None):
    """dbw_lens_pose_grad on device tensors with grad_R, grad_T and the workspace between guard bytes -> g_R (B,3,3), g_T (B,3) on the CPU."""
    ws_bytes = int(_lib.family('lens').dbw_lens_pose_grad_workspace_bytes(B, F_))
    assert ws_bytes == B * ((2 * F_ + 255) // 256) * 12 * 4
    ws = Guarded(ws_bytes)
    gR = Guarded(B * 36, fill=None if into is None else into[0])
    gT = Guarded(B * 12, fill=None if into is None else into[1])
    _lib.call('dbw_lens_pose_grad', dv['verts'].data_ptr(), dv['faces'].data_ptr(), dv['R'].data_ptr(), dv['T'].data_ptr(), dv['K'].data_ptr(), B, V, F_,
              1e-8, PR.ZC, int(persp), cl['num_faces'].data_ptr(), cl['c2o'].data_ptr(), cl['clip_code'].data_ptr(), cl['clip_w'].data_ptr(),
              g.data_ptr(), ws.mem.data_ptr(), ws_bytes, gR.mem.data_ptr(), gT.mem.data_ptr(), int(accumulate), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for x in (ws, gR, gT):
        x.check()
    return gR.floats(B, 3, 3).cpu().clone(), gT.floats(B, 3).cpu().clone()


def _case(B, F_, seed=4):
    """The icosphere scene of the host tests seen by B cameras, its first F_ faces; with B > 1 the last view looks away from everything (every
    face behind the near plane).  F_ = 1, 2: the faces are chosen so that the first one is clipped in view 0."""
    verts, faces, R, T, Kmat = PR.scene(seed, B=B)
    if B > 1:
        R[B - 1], T[B - 1] = torch.eye(3), torch.tensor([0.0, 0.0, -10.0])
    if F_ < faces.shape[0]:
        cl = PR.host_project_clip(verts, faces, R[:1].contiguous(), T[:1].contiguous(), Kmat, PR.ZC, True)
        j = int((cl['clip_code'][0, :int(cl['num_faces'][0])] >= 0).nonzero()[0])
        f = int(cl['c2o'][0, j])
        faces = torch.cat([faces[f:f + 1], faces[:f], faces[f + 1:]])[:F_].contiguous()
    return verts, faces, R.contiguous(), T.contiguous(), Kmat


@pytest.mark.parametrize('persp', [True, False])
@pytest.mark.parametrize('B,F_', [(1, 320), (3, 320), (65, 320), (3, 1), (3, 2), (65, 2), (1, 1), (65, 1), (1, 2)])
def test_pose_grad_against_the_host_build_and_the_oracle(B, F_, persp):
    verts, faces, R, T, Kmat = _case(B, F_)
    V = verts.shape[0]
    dv = {k: v.to(DEV) for k, v in dict(verts=verts, faces=faces, R=R, T=T, K=Kmat).items()}
    cl = ops.project_clip(dv['verts'], dv['faces'], dv['R'], dv['T'], dv['K'], 1e-8, PR.ZC, persp)
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
    gR, gT = _pose_grad(dv, cl, gd, B, V, F_, persp)
    # the host build of the same header: the derived bound of two fp32 sums of the same terms
    hR, hT, abs_terms, n_terms = PR.host_pose_grad(verts, faces, R, T, Kmat, clh, g, PR.ZC, persp)
    bound = PR.sum_bound(n_terms, abs_terms)
    eR, eT = (gR.double() - hR.double()).abs().reshape(B, 9), (gT.double() - hT.double()).abs()
    print(f'B={B} F={F_} persp={persp}: vs host g_R {float(eR.max()):.3e}, g_T {float(eT.max()):.3e} (smallest nonzero bound '
          f'{float(bound[bound > 0].min()) if bool((bound > 0).any()) else 0.0:.3e})')
    assert bool((eR <= bound[:, :9]).all()) and bool((eT <= bound[:, 9:]).all())
    # the oracle's autograd
    rR, rT, _ = PR.oracle_cam_grad(verts, faces, R, T, Kmat, g, PR.ZC, persp)
    print(f'   vs oracle g_R {float((gR - rR).abs().max()):.3e} (max {float(rR.abs().max()):.3e}), g_T {float((gT - rT).abs().max()):.3e} '
          f'(max {float(rT.abs().max()):.3e})')
    assert float((gR - rR).abs().max()) <= 1e-4 * float(rR.abs().max()) and float((gT - rT).abs().max()) <= 1e-4 * float(rT.abs().max())
    if B > 1:
        assert not gR[B - 1].any() and not gT[B - 1].any()                 # exactly 0 for the view without faces
    # two identical calls: the same bits
    gR2, gT2 = _pose_grad(dv, cl, gd, B, V, F_, persp)
    assert torch.equal(gR, gR2) and torch.equal(gT, gT2)
    # accumulate: a second pass with other gradients is added to the first (one fp64 add, one rounding: |acc - (r1 + r2)| <= 2^-23 (|r1| + |r2|))
    g2 = torch.randn(B, 2 * F_, 3, 3, generator=gen)
    g2d = g2.to(DEV)
    sR, sT = _pose_grad(dv, cl, g2d, B, V, F_, persp)
    aR, aT = _pose_grad(dv, cl, g2d, B, V, F_, persp, accumulate=1, into=(gR, gT))
    for a, r1, r2 in ((aR, gR, sR), (aT, gT, sT)):
        assert bool(((a.double() - (r1.double() + r2.double())).abs() <= 2.0 ** -23 * (r1.double().abs() + r2.double().abs())).all())
    # ... and through ops: the pair of buffers of the env and fg passes
    oR, oT = ops.project_clip_bwd_cam(dv['verts'], dv['faces'], dv['R'], dv['T'], dv['K'], cl, gd, 1e-8, PR.ZC, persp)
    assert torch.equal(oR.cpu(), gR) and torch.equal(oT.cpu(), gT)
    pR, pT = ops.project_clip_bwd_cam(dv['verts'], dv['faces'], dv['R'], dv['T'], dv['K'], cl, g2d, 1e-8, PR.ZC, persp, out=(oR, oT))
    assert pR is oR and torch.equal(pR.cpu(), aR) and torch.equal(pT.cpu(), aT)


def test_pose_grad_validates_its_arguments():
    verts, faces, R, T, Kmat = _case(3, 2)
    dv = {k: v.to(DEV) for k, v in dict(verts=verts, faces=faces, R=R, T=T, K=Kmat).items()}
    cl = ops.project_clip(dv['verts'], dv['faces'], dv['R'], dv['T'], dv['K'], 1e-8, PR.ZC, True)
    g = torch.zeros(3, 4, 3, 3, device=DEV)
    out, ws = torch.zeros(3, 12, device=DEV), torch.zeros(64, device=DEV)
    lib = _lib.family('lens')
    assert lib.dbw_lens_pose_grad_workspace_bytes(0, 5) == 0 and lib.dbw_lens_pose_grad_workspace_bytes(3, 2) == 3 * 12 * 4

    def call(B=3, ws_ptr=ws.data_ptr(), ws_bytes=144, gR=out.data_ptr()):
        _lib.call('dbw_lens_pose_grad', dv['verts'].data_ptr(), dv['faces'].data_ptr(), dv['R'].data_ptr(), dv['T'].data_ptr(), dv['K'].data_ptr(), B,
                  verts.shape[0], 2, 1e-8, PR.ZC, 1, cl['num_faces'].data_ptr(), cl['c2o'].data_ptr(), cl['clip_code'].data_ptr(), cl['clip_w'].data_ptr(),
                  g.data_ptr(), ws_ptr, ws_bytes, gR, out.data_ptr() + 108, 0, None)
    call()
    call(B=0, ws_ptr=None, ws_bytes=0)                                     # no views: OK, nothing launched
    with pytest.raises(RuntimeError, match='workspace'):
        call(ws_bytes=143)
    with pytest.raises(RuntimeError, match='workspace'):
        call(ws_ptr=None)
    with pytest.raises(RuntimeError, match='null'):
        call(gR=None)
    with pytest.raises(RuntimeError, match='bad size'):
        call(B=-1)
    torch.cuda.synchronize()


# ---- apply / chain ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ids', [[3, 0, 5, 1, 4, 2], [4, 1, 2]], ids=['permutation', 'subset'])
def test_pose_apply_and_chain_at_the_angles_of_the_host_tests(ids):
    V, B = len(PR.ANGLES), len(ids)
    cases = [PR.pose_case(a, 10 + k) for k, a in enumerate(PR.ANGLES)]       # row v of delta: |w| = ANGLES[v]
    delta = torch.stack([c[2] for c in cases])
    R0, T0 = torch.stack([cases[v][0] for v in ids]), torch.stack([cases[v][1] for v in ids])
    gR, gT = torch.stack([cases[v][3] for v in ids]), torch.stack([cases[v][4] for v in ids])
    idt = torch.tensor(ids, dtype=torch.int32)
    d = delta.to(DEV).requires_grad_(True)
    R1, T1 = ops.pose_apply(R0.to(DEV), T0.to(DEV), d, idt.to(DEV))
    ((R1 * gR.to(DEV)).sum() + (T1 * gT.to(DEV)).sum()).backward()
    gd, R1, T1 = d.grad.cpu(), R1.detach(), T1.detach()
    hR, hT = PR.host_pose_apply(R0, T0, delta, idt)
    hd = PR.host_pose_chain(R0, T0, delta, idt, gR, gT)
    outside = [v for v in range(V) if v not in ids]
    assert not gd[outside].any() and bool(gd[ids].any())                     # rows outside ids stay 0
    for b, v in enumerate(ids):
        ref = PR.pose_reference(cases[v][0], cases[v][1], cases[v][2], cases[v][3], cases[v][4])
        errs = dict(R=float((R1[b].cpu().double() - ref['R']).abs().max()), T=float((T1[b].cpu().double() - ref['T']).abs().max()),
                    gw=float((gd[v, :3].double() - ref['g'][:3]).abs().max()), gt=float((gd[v, 3:].double() - ref['g'][3:]).abs().max()))
        same = torch.equal(R1[b].cpu(), hR[b]) and torch.equal(T1[b].cpu(), hT[b]) and torch.equal(gd[v], hd[v])
        print(f'|w|={PR.ANGLES[v]:.3g}: ' + ', '.join(f'{k} err {e:.2e} (bar {ref["tol_" + k]:.2e})' for k, e in errs.items())
              + f'; host build: {"same bits" if same else "max diff %.2e" % float((gd[v] - hd[v]).abs().max())}')
        for k, e in errs.items():
            assert e <= ref['tol_' + k], (PR.ANGLES[v], k, e, ref['tol_' + k])
        # against the host build of the same header.  Below the series threshold (|w| < 0.25) no library function is called: both builds
        # evaluate the same expressions with one rounding per operation (no contraction, correctly rounded division) -> the same bits.
        # Above it sqrtf, sinf and cosf come from two libraries: the bar each build is held to against float64.
        if PR.ANGLES[v] ** 2 < 0.0625:
            assert same, PR.ANGLES[v]
        else:
            for k, dev_, host_ in (('R', R1[b].cpu(), hR[b]), ('T', T1[b].cpu(), hT[b]), ('gw', gd[v, :3], hd[v, :3]), ('gt', gd[v, 3:], hd[v, 3:])):
                assert float((dev_.double() - host_.double()).abs().max()) <= ref['tol_' + k], (PR.ANGLES[v], k)
        if PR.ANGLES[v] == 0.0:                                              # delta = (0, tau): the pose comes back bit for bit
            assert torch.equal(R1[b].cpu(), R0[b]) and torch.equal(T1[b].cpu(), T0[b] + delta[v, 3:])
    with pytest.raises(ValueError, match='distinct'):
        ops.pose_apply(R0.to(DEV), T0.to(DEV), d, torch.tensor([ids[0]] * B, device=DEV))


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
H, W, NB, TS, FPP = 32, 48, 3, 16, 4                             # the geometry of __graft_entry__.smoke()
PARAMS = ('sq_eps', 'S', 'R_6d', 'T', 'alpha_logit', 'R_6d_ground', 'T_ground', 'texture_bkg', 'texture_ground', 'textures')


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


# Two calls that enqueue the same work differ only in the order of the float atomic additions: reordered fp32 sums differ in their last bits.
# Eight units in the last place of the largest element of a tensor is the room given to that (two identical calls without camera gradients
# were measured up to 2.3 such units apart, a call with against a call without up to 2.6: the reference's own spread); anything larger would be another computation.
ORDER_ULPS = 8


def _model_grads(model, inp, cam_grad):
    """One forward + backward of the model -> (losses, the ten parameter gradients, (R.grad, T.grad), the library calls it made).  A call is
    recorded as its name and every argument that is not a pointer: sizes, flags, scales -- what decides the work a launch does."""
    model.zero_grad(set_to_none=True)
    d = {k: v.to(DEV) for k, v in inp.items()}
    if cam_grad:
        d['R'], d['T'] = d['R'].clone().requires_grad_(True), d['T'].clone().requires_grad_(True)
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
    return out, {k: getattr(model, k).grad.clone() for k in PARAMS}, (d['R'].grad, d['T'].grad), calls


@pytest.mark.parametrize('path', ['decoupled_mse', 'render_scene'])
def test_model_camera_gradients_match_the_oracle_model(path):
    """R.grad, T.grad of the model's total loss against autograd of the oracle model, through ops._DecoupledRenderMSE (default criteria) and
    through ops._RenderScene (masks of ones), and: asking for them changes nothing of the ten parameter gradients.

    That last property cannot be read off the gradients' bits.  The vertex and texel gradients of the existing backward are summed by float
    atomics, so two IDENTICAL calls of the model do not give the same bits: measured on an MI355X on this geometry, three calls without a
    camera gradient differ from one another in 8 of the 10 tensors (all but alpha_logit and texture_bkg) by 0.6e-7 .. 2.7e-7 of the largest
    element, and a call with the camera gradient differs from them by the same 0.1e-7 .. 2.7e-7.  What is exact is the work enqueued: the
    call with camera gradients makes the library calls of the call without them, in the same order with the same sizes, flags and scales,
    plus one dbw_lens_pose_grad per render pass -- and that one writes nothing but its own outputs (the guard bytes of
    test_pose_grad_against_the_host_build_and_the_oracle).  This is asserted, with both calls' parameter gradients held to the oracle's and
    to one another within ORDER_ULPS = 8 units in the last place of a tensor's largest element (9.5e-7)."""
    model, orc, inp, u = _smoke_model()
    if path == 'render_scene':                                   # masks of ones: the general path (ops._RenderScene), the same loss
        inp = dict(inp, masks=torch.ones(2, 1, H, W))
    seen = []
    node = ops._DecoupledRenderMSE if path == 'decoupled_mse' else ops._RenderScene
    orig = node.backward
    node.backward = staticmethod(lambda ctx, *a: (seen.append(tuple(ctx.needs_input_grad)), orig(ctx, *a))[1])
    try:
        _model_grads(model, inp, False)                          # (a first call differs from later ones: the texture bins have no demand yet)
        out0, grads0, cam0, calls0 = _model_grads(model, inp, False)
        out1, grads1, (gR, gT), calls1 = _model_grads(model, inp, True)
    finally:
        node.backward = staticmethod(orig)
    assert seen and cam0 == (None, None)                          # the node under test is the one that ran
    with torch.no_grad():
        verts_at = {'env': model.build_env_scene().verts.cpu(), 'blocks': model.build_blocks_scene(filter_transparent=False).verts.cpu()}
    oin = {k: v for k, v in inp.items() if k != 'masks'}
    oin['R'], oin['T'] = inp['R'].clone().requires_grad_(True), inp['T'].clone().requires_grad_(True)
    ref = orc.forward(oin, training=True, coarse=True, decimate=False, opacity_noise=None, overlap_points=u, n_threads=8, verts_at=verts_at)
    ref['total'].backward()
    assert abs(out1['total'].item() - ref['total'].item()) <= REL * abs(ref['total'].item())
    eR, eT = rel_err(gR, oin['R'].grad), rel_err(gT, oin['T'].grad)
    print(f'{path}: R.grad rel err {eR:.2e} (max {float(oin["R"].grad.abs().max()):.3e}), T.grad rel err {eT:.2e} (max {float(oin["T"].grad.abs().max()):.3e})')
    assert eR < REL and eT < REL
    # the same launches with the same arguments, plus the camera gradient of each render pass (env and fg)
    assert not any(c[0] == 'dbw_lens_pose_grad' for c in calls0)
    extra = [c for c in calls1 if c[0] == 'dbw_lens_pose_grad']
    # (one argument differs: the env pass's backward skips the geometry gradient of the sky dome's faces -- constant vertices -- unless a camera
    # gradient sums over them, which moves in the image with the camera like every other face: const_faces 0 in place of the dome's face count)
    BWD = 'dbw_render_bwd_fused'
    domeless = lambda cs: [c[:-2] + (0,) + c[-1:] if c[0] == BWD else c for c in cs]        # noqa: E731
    assert domeless([c for c in calls1 if c[0] != 'dbw_lens_pose_grad']) == domeless(calls0) and len(extra) == 2
    assert {c[-2] for c in calls1 if c[0] == BWD} == {0} and {c[-2] for c in calls0 if c[0] == BWD} == {0, model._n_bkg_faces}
    assert [c[-1] for c in extra] == ([0, 1] if path == 'decoupled_mse' else [0, 0])      # one accumulating pair of buffers / one per node
    for k in PARAMS:
        d01 = rel_err(grads1[k], grads0[k])
        print(f'   {k}: with against without camera gradients {d01:.1e}{" (same bits)" if torch.equal(grads0[k], grads1[k]) else ""}')
        assert rel_err(grads0[k], orc.p[k].grad) < REL and rel_err(grads1[k], orc.p[k].grad) < REL, k
        assert d01 <= ORDER_ULPS * 2.0 ** -23, k


def _pose_errors(R, T, P_R, P_T):
    """Mean rotation angle (rad) of R^T P_R and mean |T - P_T| over the views."""
    M = R.double().transpose(1, 2) @ P_R.double()
    cos = ((M.diagonal(dim1=1, dim2=2).sum(1) - 1) / 2).clamp(-1, 1)
    return float(torch.acos(cos).mean()), float((T.double() - P_T.double()).norm(dim=1).mean())


REFINE_STEPS, REFINE_LR = 150, 1e-3


def _refinement_run(refine):
    model, orc, inp, u = _smoke_model()
    with torch.no_grad():                                        # textures with structure: a pose error has something to show in
        gen = torch.Generator().manual_seed(9)
        for name in ('texture_bkg', 'texture_ground', 'textures'):
            p = getattr(model, name)
            low = torch.randn(p.shape[0], 3, 4, 4, generator=gen) * 2.0
            p.copy_(torch.nn.functional.interpolate(low, size=p.shape[1:3], mode='bilinear', align_corners=False).permute(0, 2, 3, 1).to(DEV))
    P_R, P_T = inp['R'].to(DEV), inp['T'].to(DEV)
    d = {k: v.to(DEV) for k, v in inp.items()}
    with torch.no_grad():
        fg, env = model.render_layers(d)
        target = ops.composite(fg, env)[:, :3].contiguous()
    # the training views' poses: P perturbed by a known delta* of about 1 degree and 1 % of the camera distance (2.8)
    star = torch.tensor([[0.012, -0.009, 0.008, 0.02, -0.015, 0.018], [-0.010, 0.011, -0.009, -0.018, 0.02, 0.015]], device=DEV)
    R0, T0 = ops.pose_apply(P_R, P_T, star, torch.arange(2, device=DEV))
    ref = pose.PoseRefiner(2, DEV, lr=REFINE_LR)
    batch = dict(imgs=target, R=R0, T=T0, K=d['K'], view_ids=torch.arange(2, device=DEV))
    rgb, errs = [], [_pose_errors(R0, T0, P_R, P_T)]
    for _ in range(REFINE_STEPS):
        model.zero_grad(set_to_none=True)                        # (the model's parameters are not stepped)
        b = ref.apply(batch) if refine else batch
        out = model(b, None)
        out['total'].backward()
        if refine:
            ref.step()
        rgb.append(float(out['rgb']))
    errs.append(_pose_errors(*ref.refined(R0, T0), P_R, P_T))
    return rgb, errs


def test_pose_only_steps_find_a_known_perturbation():
    """Targets rendered by the model itself at poses P (smooth random textures, so that a pose error shows); the training views start at P
    perturbed by a known delta* of about 1 degree and 1 % of the camera distance.  150 pose-only Adam steps at lr 1e-3: model(inp),
    backward, PoseRefiner.step(); the model's parameters are not stepped.
    Observed on an MI355X (profiles/pose_refine.md): rgb loss 1.830e-03 -> 8.53e-06 (215 x lower); mean rotation error 0.985 -> 0.239 deg
    (4.1 x); mean translation error 0.0518 -> 0.0024 (22 x).  After 60 steps: 3.25e-05, 0.434 deg, 0.0040.  The assertions ask for a
    decrease only: the margins are those factors."""
    rgb, (e0, e1) = _refinement_run(True)
    print(f'rgb loss {rgb[0]:.6e} -> {rgb[-1]:.6e}; rotation error {math.degrees(e0[0]):.3f} -> {math.degrees(e1[0]):.3f} deg; '
          f'translation error {e0[1]:.4f} -> {e1[1]:.4f}')
    assert rgb[-1] < rgb[0]
    assert e1[0] < e0[0] and e1[1] < e0[1]
    # without the refiner nothing moves: the loss is the same number at every step, so the decrease above is the feature's
    rgb_off, (f0, f1) = _refinement_run(False)
    assert rgb_off[0] == rgb[0] and all(v == rgb_off[0] for v in rgb_off) and f0 == f1


# ---- the command line -----------------------------------------------------------------------------------------------------------------------------
def test_the_command_line_refines_the_poses_of_a_custom_scene(tmp_path):
    import json
    import yaml
    root = tmp_path / 'data'
    write_capture(root, 'desk', n=6, H=24, W=32, dist=LR.COEFFS[0], with_points=True)
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
    scores = train.main(['--config', str(path), '--tag', 'run', '--data-root', str(root), '--runs-root', str(tmp_path / 'runs'),
                         '--no-perceptual', '--epochs', '2', '--pose-refine', '1e-4', '--device', DEV])
    assert all(np.isfinite(float(v)) for k, v in scores.items() if k != 'LPIPS' and not isinstance(v, dict)) and scores['PSNR'] > 0
    run_dir = tmp_path / 'runs' / 'custom' / 'run'
    with open(run_dir / 'transforms_refined.json') as f:
        refined = json.load(f)
    with open(root / 'custom' / 'desk' / 'transforms.json') as f:
        src = json.load(f)
    diff = [float(np.abs(np.asarray(a['transform_matrix']) - np.asarray(b['transform_matrix'])).max()) for a, b in zip(refined['frames'], src['frames'])]
    print('largest change of a transform_matrix entry per frame:', ['%.2e' % x for x in diff])
    assert len(diff) == 6 and all(np.isfinite(x) and 0 < x < 0.1 for x in diff)          # 6 frames, all training views: every pose moved a little
    ckpt = torch.load(run_dir / 'model.pkl', map_location='cpu', weights_only=False)
    assert ckpt['epoch'] == 2 and ckpt['pose_refine']['n_steps'] == 6 and bool(ckpt['pose_refine']['delta'].any())      # 2 epochs x 3 batches
    # --resume restores the refiner
    train.main(['--config', str(path), '--tag', 'run', '--data-root', str(root), '--runs-root', str(tmp_path / 'runs'), '--no-perceptual',
                '--epochs', '3', '--pose-refine', '1e-4', '--resume', '--device', DEV])
    again = torch.load(run_dir / 'model.pkl', map_location='cpu', weights_only=False)
    assert again['epoch'] == 3 and again['pose_refine']['n_steps'] == 9


def test_refined_poses_are_refused_under_two_ranks():
    model, orc, inp, u = _smoke_model()
    step = ShardedTrainStep(model, lr=0.0, lr_texture=0.0, seed=1)
    step.world_size = 2                                          # (what a second rank would make it: the refusal comes before any collective)
    d = {k: v.to(DEV) for k, v in inp.items()}
    d['R'] = d['R'].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match='pose'):
        step(d)
