"""No GPU.  (1) Every float64 reference of tests/model_kernels_ref.py against torch float64 autograd of the same expression on the CPU, to
1e-12 of the element's magnitude M.  (2) The arithmetic the kernels share with the host (csrc/loss_math.h, csrc/model_math.h, built by g++:
tests/host_loss_math.cpp, tests/host_model_math.cpp) on the edge values of tests/test_gpu_model_kernels.py against the same references
with the same metric and the same bars -- so that a failure that shows only on the GPU lies in a launch, not in the arithmetic.  (3) The
conditioning of the inputs whose value is continuous and whose gradient is not (overlap: sum = thresh, the safe_pow clamps, |inv| = 5;
the opacity mask; the parsimony clamp): no sample within the stated margin of a branch, none left out."""
import ctypes

import numpy as np
import pytest
import torch

import model_kernels_ref as R
from host_build import host_lib

F64, F32, CPU = torch.float64, torch.float32, 'cpu'
c_f = ctypes.c_float


def rnd(seed):
    return np.random.RandomState(seed)


def agree(ref, auto, keys, tol=1e-12):
    for k in keys:
        a, b, M = R.f64(ref[k]), R.f64(auto[k]), R.f64(ref['M_' + k])
        assert a.shape == b.shape, k
        e = float((np.abs(a - b) / (M + 1e-300)).max()) if a.size else 0.0
        assert e <= tol, (k, e)


def f32(*xs):
    return [np.ascontiguousarray(x, dtype=np.float32) for x in xs]


# ---- (1) references against float64 autograd ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,shape', [(1, (2, 5, 7)), (2, (3, 4, 6)), (3, (2, 6, 9)), (16, (1, 16, 32))])
def test_texture_preparation_reference(d, shape):
    n, h, w = shape
    g = rnd(d)
    tex, gmaps, gsig = f32(g.randn(n, h, w, 3) * 4, g.randn(n, h // d, w // d, 3), g.randn(n, h, w, 3))
    tex.reshape(-1)[:5] = (0, 20, -20, 90, -90)
    for gs in (gsig, None):
        ref = dict(R.texture_prep_fwd(tex, d), **R.texture_prep_bwd(tex, d, gmaps, gs))
        agree(ref, R.torch_texture_prep(tex, d, gmaps, gs, F64, CPU), ('sig', 'maps', 'gtex'))


@pytest.mark.parametrize('wrap', [0, 1])
@pytest.mark.parametrize('shape', [(1, 2, 2), (1, 2, 9), (3, 7, 2), (3, 6, 5)])
def test_tv_reference(shape, wrap):
    m, = f32(rnd(sum(shape)).rand(*shape, 3))
    for scale in (1.0, 0.37):
        agree(R.tv_l2sq(m, wrap, scale), R.torch_tv(m, wrap, scale, F64, CPU), ('value', 'grad'))


def test_composite_reference():
    g = rnd(0)
    fg, env, img = f32(g.rand(2, 4, 3, 5), g.rand(2, 4, 3, 5), g.rand(2, 3, 3, 5))
    fg[0, 3, 0, 0], fg[1, 3, 2, 4] = 0.0, 1.0
    ref = R.composite_mse(fg, env, img, 0.01, 1.7)
    agree(ref, R.torch_composite(fg, env, img, 0.01, 1.7, F64, CPU), ('rec', 'value', 'gfg', 'genv'))
    assert (ref['genv'][:, 3] == 0).all()
    agree(R.composite_mse(fg, env), R.torch_composite(fg, env, None, 1.0, 1.0, F64, CPU), ('rec',))


@pytest.mark.parametrize('step', [1, 7, 100000])
def test_adam_reference(step):
    g = rnd(step % 10)
    n = 60
    p, grad, m, v = f32(g.randn(n), g.randn(n), g.randn(n) * 0.1, g.rand(n) * 0.01)
    grad[:5], v[0] = (0.0, 1e-30, -1e-30, 1e15, -1e15), 0.0
    ends, lrs = [0, 7, 7, n], [1e-3, 5e-2, 5e-3, 1e-2]
    agree(R.adam(p, grad, m, v, step, R.group_lr(ends, lrs, n), 0.9, 0.999, 1e-8),
          R.torch_adam(p, grad, m, v, step, lrs, 0.9, 0.999, 1e-8, F64, CPU, ends), ('p', 'm', 'v'))
    agree(R.adam(p, grad, m, v, step, 5e-3, 0.9, 0.999, 1e-8), R.torch_adam(p, grad, m, v, step, 5e-3, 0.9, 0.999, 1e-8, F64, CPU), ('p', 'm', 'v'))


@pytest.mark.parametrize('thresh', R.ALPHA_THRESH)
def test_block_opacity_reference(thresh):
    lg, nz = R.alpha_logits(65)
    g = rnd(1)
    ga, gf = f32(g.randn(65, 3), g.randn(65))
    for noise in (None, nz):
        fwd = R.block_alpha_fwd(lg, noise, 0.3, thresh)
        ref = dict(fwd, **R.block_alpha_bwd(fwd['alpha'], fwd['keep'], ga, gf))
        auto = R.torch_block_alpha(lg, noise, 0.3, thresh, ga, gf, F64, CPU)
        agree(ref, auto, ('alpha', 'alpha_full', 'g_logit'))
        assert np.array_equal(ref['keep'], auto['keep'])


def test_parsimony_reference():
    x = R.parsimony_values(65)
    off = x != np.float32(R.PARSIMONY_EPS)          # (at x == eps torch.clamp passes the gradient; the reference takes the kernel's side: none)
    ref, auto = R.sqrt_mean(x, R.PARSIMONY_EPS, 0.01), R.torch_sqrt_mean(x, R.PARSIMONY_EPS, 0.01, F64, CPU)
    agree(ref, auto, ('value',))
    agree({k: v[off] for k, v in ref.items() if 'grad' in k}, {'grad': auto['grad'][off]}, ('grad',))
    assert ref['grad'][2] == 0 and auto['grad'][2] != 0


def _mesh_inputs(nv, seed):
    g = rnd(seed)
    return f32(g.randn(nv, 3), g.randn(6), g.randn(3), g.randn(3, 3), g.randn(3), g.randn(nv, 3))


def test_posed_mesh_reference():
    base, R6, T, Rw, Tw, gv = _mesh_inputs(70, 3)
    agree(R.posed_mesh(base, R6, T, 0.5, Rw, Tw, gv), R.torch_posed_mesh(base, R6, T, 0.5, Rw, Tw, gv, F64, CPU), ('verts', 'g_R6', 'g_T'))


def _block_inputs(Kb, nv, seed):
    g = rnd(seed)
    sq = np.stack([np.linspace(-8, 8, Kb), np.linspace(8, -8, Kb)], 1) + g.randn(Kb, 2) * 0.3
    eta, om = g.rand(Kb, nv) * np.pi - np.pi / 2, g.rand(Kb, nv) * 2 * np.pi - np.pi
    trig = np.stack([np.cos(eta), np.sin(eta), np.cos(om), np.sin(om)])
    for v, pole in enumerate(((0, 1, 1, 0), (1, 0, 0, -1), (0, -1, -1, 0))):          # the poles
        trig[:, :, v] = np.array(pole)[:, None]
    return f32(sq, g.randn(Kb, 3) * 0.3, g.randn(Kb, 6), g.randn(Kb, 3), trig, g.randn(Kb, nv, 3))


def test_superquadric_blocks_reference():
    sq, S, R6, T, trig, gv = _block_inputs(5, 20, 2)
    _, _, _, Rw, Tw, _ = _mesh_inputs(1, 4)
    agree(R.sq_blocks(sq, S, R6, T, trig, 0.5, 0.2, 0.5, Rw, Tw, gv), R.torch_sq_blocks(sq, S, R6, T, trig, 0.5, 0.2, 0.5, Rw, Tw, gv, F64, CPU),
          ('verts', 'g_sq_eps', 'g_S', 'g_R6', 'g_T'))


def test_block_frame_points_and_their_exponent_derivatives_reference():
    """sq_local_points (what the step's prologue keeps for its tail): d / d eps1 and d / d eps2 against a central float64 difference in the
    exponent, and the points against the vertices of sq_blocks under the identity pose.  A difference of step h of a function with
    third derivative f''' is off by h^2 f''' / 6 + rounding 1e-16 / h.  Here f = |t|^e, f''' = f log^3 |t|, and |log|^3 < 1e3 for a cosine
    down to 1e-4: at h = 1e-5 that is 2e-8 f + 1e-11 -- held to 1e-6 of M, which a derivative wrong in a factor or a sign misses by 1."""
    sq, S, R6, T, trig, gv = _block_inputs(5, 20, 2)
    e, _ = R.exponents(sq)
    ref = R.sq_local_points(e, trig, 0.5)
    assert not ref['de1'][:, :3].any() and not ref['de2'][:, :3].any() and not ref['de2'][..., 1].any()          # the poles; y does not depend on eps2
    h = 1e-5
    for j, key in enumerate(('de1', 'de2')):
        d = np.zeros((1, 2)); d[0, j] = h
        fd = (R.sq_local_points(e + d, trig, 0.5)['loc'] - R.sq_local_points(e - d, trig, 0.5)['loc']) / (2 * h)
        M = ref['M_' + key] + ref['M_loc']          # (a point's own size: where the derivative vanishes the difference still rounds on it)
        assert float((np.abs(fd - ref[key]) / (M + 1e-300)).max()) <= 1e-6, key          # (M = 0: a coordinate that is exactly 0, its difference too)
        assert float(np.abs(ref[key]).max()) > 0.05          # not a comparison of zeros
    # the points themselves: sq_blocks with S = 0 and scale_min = 0 (exp(S) + scale_min = 1), R = 1, T = 0, world = identity
    ident6 = np.tile(np.array([1, 0, 0, 0, 1, 0], np.float64), (5, 1))
    v = R.sq_blocks(sq, np.zeros((5, 3)), ident6, np.zeros((5, 3)), trig, 0.5, 0.0, 1.0, np.eye(3), np.zeros(3))
    assert float(np.abs(v['verts'] - R.sq_local(sq, trig, 0.5)['loc']).max()) <= 1e-12
    # and through them the shape gradient of sq_blocks: g_sq_eps = sum gloc . de * d eps / d sq_eps is what autograd holds above


def test_loss_values_reference():
    g = rnd(4)
    part, = f32(g.rand(1000) * 3)
    vals = np.array([0, 0.25, 1.5, 0.125, 0, 0, 0, 0], np.float32)
    ref = R.loss_finish(part, 1e-3, 0.5, vals)
    t = torch.from_numpy(part).double().sum() * R.f32v(1e-3)
    assert abs(ref['rgb'] - float(t)) <= 1e-12 * ref['M_rgb'] and ref['M_rgb'] == ref['rgb']
    assert np.array_equal(ref['out5'][1:4], [0.25, 0.75, 0.125]) and abs(ref['out5'][4] - (float(t) + 1.125)) <= 1e-12
    assert R.loss_finish(np.zeros(0, np.float32), 1e-3, 0.5, vals)['rgb'] == 0


@pytest.mark.parametrize('name', list(R.OVERLAP_CASES) + list(R.STEP_OVERLAP_CASES) + list(R.STEP_BITWISE_CASES))
def test_overlap_reference_and_its_conditioning(name):
    c = R.overlap_case(name)
    ref = R.overlap_ref(c)
    cond = ref['cond']
    assert cond['points'] == c['Kb'] * c['npts']
    for k, margin in R.OVERLAP_MARGINS.items():          # conditions, not measurements: no sample within the margin of a branch, none left out
        assert cond[k] > margin, (name, k, cond[k])
    if name.endswith('below-threshold'):
        assert cond['active'] == 0 and ref['value'] == 0 and all(not ref[k].any() for k in ('g_sq_eps', 'g_S', 'g_R6', 'g_T', 'g_alpha'))
    elif cond['points'] == 1:
        assert cond['active'] == 1 and ref['value'] > 1e-3          # (the step's one-point case: that point is above the threshold)
    else:
        assert cond['active'] > 10 and ref['value'] > 1e-3
    if name in R.STEP_OVERLAP_CASES:                           # ... and float32 as such less than half of it (small cases: few samples to average over)
        assert R.overlap_float32_cost(c, ref) < R.FLOAT32_COST_MARGIN * R.FLOOR['overlap'][1], name
    if name in R.STEP_BITWISE_CASES:                           # (held to the operator kernels bit for bit and not to float64: why -- float32 itself is above the floor)
        assert R.overlap_float32_cost(c, ref) > R.FLOOR['overlap'][1] and c['Kb'] * c['npts'] <= 64, name
    if name in {**R.STEP_OVERLAP_CASES, **R.STEP_BITWISE_CASES} and c['Kb'] >= 5:          # the parsimony term of the same launch: at its clamp and just above it
        assert c['alpha'][2] == np.float32(R.PARSIMONY_EPS) and c['alpha'][3] > np.float32(R.PARSIMONY_EPS) and c['alpha'][3] < np.float32(1.000001e-6)
    # what float32 sample points alone cost the gradients, everything else exact: well below the floor, so that the floor is about the kernel
    assert R.overlap_point_rounding(c, ref) < R.POINT_ROUNDING_MARGIN * R.FLOOR['overlap'][1], name
    if c['Kb'] >= 3:
        assert cond['clamped'] > 0 and c['alpha'][1] == 0          # the far block's clamp masks gradients; an exact 0 among the opacities
    auto = R.torch_overlap(c['u'], c['sq_eps'], c['S'], c['R6'], c['T'], c['alpha'], c['ratio'], c['scale_min'], c['temperature'], c['thresh'],
                           c['scale'], F64, CPU)
    agree(ref, auto, ('value', 'g_sq_eps', 'g_S', 'g_R6', 'g_T', 'g_alpha'))


def implicit_points(seed):
    """points in [-6, 6]^3 (some beyond the clamp), with coordinates planted at exactly 0 (below safe_pow's clamp: no gradient) and
    exactly +-5 (inside the range the kernel's `>= -5 && <= 5` keeps, as torch.clamp's backward does); none within 1e-4 (relative) of
    x^2 = 1e-6 or within 1e-4 of |x| = 5 otherwise"""
    g = rnd(seed)
    pts = (g.rand(200, 3) * 12 - 6).astype(np.float32)
    pts[0], pts[1], pts[2], pts[3] = (0, 0.5, 0.5), (0.3, 0, -0.2), (5, -5, 0.1), (0, 0, 0)
    sq, ab = R.f64(pts) ** 2, np.abs(R.f64(pts))
    assert (np.abs(sq - 1e-6) / 1e-6 > 1e-4).all() and ((np.abs(ab - 5) > 1e-4) | (ab == 5)).all()
    return pts, g.randn(200).astype(np.float32)


IMPLICIT_EXPONENTS = [(0.1, 1.9), (1.0, 1.0), (1.9, 0.1), (0.37, 1.22), (1.9, 1.9)]


@pytest.mark.parametrize('e1,e2', IMPLICIT_EXPONENTS)
def test_implicit_superquadric_reference(e1, e2):
    pts, w = implicit_points(3)
    ref, auto = R.implicit_sdf(pts, e1, e2, w), R.torch_implicit_sdf(pts, e1, e2, w, F64, CPU)
    agree(ref, auto, ('sdf', 'gpts'))
    agree(dict(ge_sum=ref['ge'].sum(0), M_ge_sum=ref['M_ge'].sum(0)), auto, ('ge_sum',))


def test_conditioning_of_the_opacity_mask_and_of_the_parsimony_clamp():
    for Kb in R.ALPHA_KB:
        lg, _ = R.alpha_logits(Kb)
        assert R.alpha_margin(lg) > R.ALPHA_MARGIN, Kb
    for n in R.PARSIMONY_N:
        x = R.parsimony_values(n)
        assert R.parsimony_margin(x) > 1e-4, n
        if n >= 64:
            assert x[2] == np.float32(R.PARSIMONY_EPS) and (x[:2] < np.float32(R.PARSIMONY_EPS)).all()


# ---- (2) the host builds of the shared headers on the edge values ------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def held(name, family, which, got, ref, M, count=1):
    e, b = R.err(got, ref, M, count), R.bar(family, which)
    assert e <= b, (name, e, b)


@pytest.mark.parametrize('wrap', [0, 1])
@pytest.mark.parametrize('shape', [(1, 2, 2), (1, 2, 300), (3, 200, 5), (3, 200, 300)])
def test_host_tv_texel(shape, wrap):
    L = host_lib('loss_math')
    L.host_tv.restype = ctypes.c_double
    n, h, w = shape
    m, = f32(rnd(7 + w).rand(n, h, w, 3))
    grad = np.full_like(m, np.nan)
    v = L.host_tv(_p(m), n, h, w, wrap, _p(grad))
    ref = R.tv_l2sq(m, wrap, 1.0)
    held('value', 'tv', 0, v, ref['value'], ref['M_value'], ref['terms'])
    held('grad', 'tv', 1, grad, ref['grad'], ref['M_grad'], 4)
    const = np.full_like(m, 0.3)
    assert L.host_tv(_p(const), n, h, w, wrap, _p(grad)) == 0 and not grad.any()


def test_host_composite_pixel():
    L = host_lib('loss_math')
    L.host_composite_mse.restype = ctypes.c_double
    P = 1025
    g = rnd(2)
    fg, env, img = f32(g.rand(4, P), g.rand(4, P), g.rand(3, P))
    fg[3, 0], fg[3, -1], fg[3, 7] = 1.0, 0.0, 1.0
    scale = 1.0 / (3 * P)
    rec, gfg, genv = np.full((3, P), np.nan, np.float32), np.full((4, P), np.nan, np.float32), np.full((3, P), np.nan, np.float32)
    v = L.host_composite_mse(_p(fg), _p(env), _p(img), P, c_f(scale), _p(rec), _p(gfg), _p(genv))
    ref = R.composite_mse(fg[None, :, None], env[None, :, None], img[None, :, None], scale, 1.0)
    held('value', 'composite', 0, v, ref['value'], ref['M_value'], 3 * P)
    held('rec', 'composite', 0, rec, ref['rec'][0, :, 0], ref['M_rec'][0, :, 0], 2)
    held('gfg', 'composite', 1, gfg, ref['gfg'][0, :, 0], ref['M_gfg'][0, :, 0], 9)
    held('genv', 'composite', 1, genv, ref['genv'][0, :3, 0], ref['M_genv'][0, :3, 0], 3)


@pytest.mark.parametrize('step', [1, 7, 100000])
def test_host_adam_update(step):
    L = host_lib('loss_math')
    n = 257
    g = rnd(step % 10)
    p, grad, m, v = f32(g.randn(n), g.randn(n), g.randn(n) * 0.1, g.rand(n) * 0.01)
    grad[:5], v[0], v[2] = (0.0, 1e-30, -1e-30, 1e15, -1e15), 0.0, 0.0
    m[5], grad[5], m[6], grad[6] = 0.5, -0.5, -0.05, 0.45
    ref = R.adam(p, grad, m, v, step, 5e-3, 0.9, 0.999, 1e-8)
    L.host_adam(_p(p), _p(grad), _p(m), _p(v), n, c_f(5e-3), c_f(0.9), c_f(0.999), c_f(1e-8), step)
    for k, x in (('p', p), ('m', m), ('v', v)):
        held(k, 'adam', 0, x, ref[k], ref['M_' + k], 3)


def test_host_posing_and_rotation():
    L = host_lib('model_math')
    for nv in (1, 65, 1000):
        base, R6, T, Rw, Tw, gv = _mesh_inputs(nv, nv)
        S_raw = np.zeros(3, np.float32)
        world, g_S, g_R6, g_T, g_v = (np.full(s, np.nan, np.float32) for s in ((nv, 3), (3,), (6,), (3,), (nv, 3)))
        # load_pose with S given: exp(0) + scale_min = 1 with scale_min = 0
        L.host_pose(_p(S_raw), _p(R6), _p(T), c_f(0.0), _p(base), nv, c_f(0.5), _p(Rw), _p(Tw), _p(gv), _p(world), _p(g_S), _p(g_R6), _p(g_T), _p(g_v))
        ref = R.posed_mesh(base, R6, T, 0.5, Rw, Tw, gv)
        held('verts', 'mesh', 0, world, ref['verts'], ref['M_verts'], 7)
        held('g_R6', 'mesh', 1, g_R6, ref['g_R6'], ref['M_g_R6'], nv * 9)
        held('g_T', 'mesh', 1, g_T, ref['g_T'], ref['M_g_T'], nv * 9)


def test_host_superquadric_points_at_the_poles_and_over_the_exponent_range():
    L = host_lib('model_math')
    sq, S, R6, T, trig, gv = _block_inputs(5, 65, 6)
    e, _ = R.exponents(sq)
    for k in range(5):
        e1, e2 = np.float32(e[k, 0]), np.float32(e[k, 1])
        loc, de1, de2 = (np.full((65, 3), np.nan, np.float32) for _ in range(3))
        t = [np.ascontiguousarray(trig[i, k]) for i in range(4)]
        L.host_parametric(_p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), 65, c_f(e1), c_f(e2), c_f(0.5), _p(loc), _p(de1), _p(de2))
        A, dA = R._spow(R.f64(t[0]), float(e1)); C, dC = R._spow(R.f64(t[1]), float(e1))
        Bc, dBc = R._spow(R.f64(t[2]), float(e2)); Bs, dBs = R._spow(R.f64(t[3]), float(e2))
        rl = np.stack([A * Bs, C, A * Bc], -1) * 0.5
        r1 = np.stack([dA * Bs, dC, dA * Bc], -1) * 0.5
        r2 = np.stack([A * dBs, np.zeros(65), A * dBc], -1) * 0.5
        held('loc', 'blocks', 0, loc, rl, np.abs(rl))
        held('de1', 'blocks', 1, de1, r1, np.abs(r1))
        held('de2', 'blocks', 1, de2, r2, np.abs(r2))
        assert not de1[:3].any() and not de2[:3].any()          # the poles: |cos|, |sin| in {0, 1} -> d / d exponent is exactly 0 there


@pytest.mark.parametrize('e1,e2', IMPLICIT_EXPONENTS)
def test_host_implicit_superquadric(e1, e2):
    L = host_lib('model_math')
    pts, w = implicit_points(3)
    e1, e2 = float(np.float32(e1)), float(np.float32(e2))
    ref = R.implicit_sdf(pts, e1, e2, w)
    sdf, gpts, ge = (np.full(s_, np.nan, np.float32) for s_ in ((200,), (200, 3), (200, 2)))
    L.host_implicit(_p(pts), 200, c_f(e1), c_f(e2), _p(w), _p(sdf), _p(gpts), _p(ge))
    held('sdf', 'overlap', 0, sdf, ref['sdf'], ref['M_sdf'], 2)
    held('gpts', 'overlap', 1, gpts, ref['gpts'], ref['M_gpts'])
    held('ge', 'overlap', 1, ge, ref['ge'], ref['M_ge'], 3)
    assert not gpts[3].any() and gpts[0, 0] == 0 and gpts[1, 1] == 0          # below safe_pow's clamp: exactly no gradient
    assert gpts[2, 0] != 0 and gpts[2, 1] != 0                                 # exactly +-5: in range
