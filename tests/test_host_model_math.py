"""CPU tests of the product's model arithmetic (csrc/model_math.h, the header model_ops.hip compiles) built for the host with g++
(tests/host_model_math.cpp), against golden vectors of the REAL reference functions (tests/golden/, made by make_golden.py from
src/utils/superquadric.py:10-38 and src/utils/pytorch.py:31-36) and against torch autograd of the oracle's restatements:
superquadric surface points and their exponent gradients, the implicit superquadric distance of the overlap term with all its
gradients, signed_pow / safe_pow, the 6D rotation and the posing chain with their hand-derived backward."""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle as O
from host_build import host_lib


def lib():
    return host_lib('model_math')


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _f(x):
    return ctypes.c_float(float(x))


def _load(golden_dir, name):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(golden_dir, name)).items()}


def test_parametric_sq_points_and_exponent_gradients_match_the_reference_golden(golden_dir):
    g = _load(golden_dir, 'parametric_sq.npz')
    eta, omega = g['eta'].double(), g['omega'].double()
    trig = [t.float().contiguous() for t in (eta.cos(), eta.sin(), omega.cos(), omega.sin())]     # tabulated on the host, as the model does
    n = eta.numel()
    for i in range(4):
        for j in range(4):
            e1, e2 = [float(x) for x in g[f'{i}{j}/eps']]
            loc, de1, de2 = torch.empty(n, 3), torch.empty(n, 3), torch.empty(n, 3)
            assert lib().host_parametric(*[_p(t) for t in trig], n, _f(e1), _f(e2), _f(1.0), _p(loc), _p(de1), _p(de2)) == 0
            ref = g[f'{i}{j}/pts'][0]
            torch.testing.assert_close(loc, ref, rtol=2e-5, atol=2e-6)
            w = g[f'{i}{j}/w'][0]
            for d, key in ((de1, 'g_eps1'), (de2, 'g_eps2')):
                got, exp = float((d * w).sum()), float(g[f'{i}{j}/{key}'])
                if np.isnan(exp):          # 0 * inf at a pole / on the equator in the reference: the product returns 0 there
                    continue
                assert abs(got - exp) <= 1e-4 * max(abs(exp), 1.0), (i, j, key, got, exp)


def test_implicit_sq_safe_pow_signed_pow_match_the_reference_golden(golden_dir):
    g = _load(golden_dir, 'implicit_misc.npz')
    for b in range(g['pts'].shape[0]):
        pts, w = g['pts'][b].contiguous(), g['w'][b].contiguous()
        e1, e2 = float(g['eps1'][b]), float(g['eps2'][b])
        n = pts.shape[0]
        sdf, gpts, ge = torch.empty(n), torch.empty(n, 3), torch.empty(n, 2)
        assert lib().host_implicit(_p(pts), n, _f(e1), _f(e2), _p(w), _p(sdf), _p(gpts), _p(ge)) == 0
        torch.testing.assert_close(sdf, g['sdf'][b], rtol=2e-5, atol=2e-6)
        ref = g['g_pts'][b]
        assert float((gpts - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
        # d / d eps: a sum of 64 cancelling terms, judged against their magnitude.  The fp32 golden itself is 1.3e-4 of that magnitude
        # away from the same function evaluated in float64 (the product: 2e-5), so the bar against the golden is 2e-4 and the float64
        # evaluation of the oracle's restatement arbitrates at 5e-5
        E = [torch.tensor([[e]], dtype=torch.float64, requires_grad=True) for e in (e1, e2)]
        (O.implicit_sq_sdf2(pts[None].double(), E[0], E[1])[0] * w.double()).sum().backward()
        for k, key in enumerate(('g_eps1', 'g_eps2')):
            got, exp, mag = float(ge[:, k].double().sum()), float(g[key][b]), float(ge[:, k].double().abs().sum())
            assert abs(got - exp) <= 2e-4 * mag, (b, key, got, exp, mag)
            assert abs(got - float(E[k].grad)) <= 5e-5 * mag, (b, key, got, float(E[k].grad), mag)
    t = g['spow_in'].contiguous()
    sp, _s, _d = torch.empty_like(t), torch.empty_like(t), torch.empty_like(t)
    lib().host_pows(_p(t), t.numel(), _f(0.37), _p(sp), _p(_s), _p(_d))
    torch.testing.assert_close(sp, g['spow_out'], rtol=1e-6, atol=1e-7)
    a = g['sp_in'].contiguous()
    _sp, safe, dt = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
    lib().host_pows(_p(a), a.numel(), _f(0.5), _p(_sp), _p(safe), _p(dt))
    torch.testing.assert_close(safe, g['sp_out'], rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(dt, g['sp_grad'], rtol=1e-5, atol=1e-6)


def test_rotation_6d_and_posing_match_autograd_of_the_oracle():
    gen = torch.Generator().manual_seed(3)
    for _ in range(5):
        a6 = torch.randn(6, generator=gen)
        G = torch.randn(3, 3, generator=gen)
        R9, ga = torch.empty(9), torch.empty(6)
        lib().host_rot6d(_p(a6), _p(G.contiguous()), _p(R9), _p(ga))
        a = a6.clone().requires_grad_(True)
        R = O.rotation_6d_to_matrix(a[None])[0]
        torch.testing.assert_close(R9.view(3, 3), R.detach(), rtol=1e-5, atol=1e-6)
        (R * G).sum().backward()
        torch.testing.assert_close(ga, a.grad, rtol=1e-4, atol=1e-5)
        # posing: ((v * (exp(S) + s_min)) @ R + T) * S_world @ R_world + T_world, row vectors (dbw.py:297-311,343-344)
        n = 17
        S_raw, T = torch.randn(3, generator=gen) * 0.3, torch.randn(3, generator=gen)
        v, g = torch.randn(n, 3, generator=gen), torch.randn(n, 3, generator=gen)
        Rw, Tw = O.world_rotation(115, 0, 0), torch.randn(3, generator=gen)
        world, gS, gR6, gT, gv = torch.empty(n, 3), torch.empty(3), torch.empty(6), torch.empty(3), torch.empty(n, 3)
        lib().host_pose(_p(S_raw), _p(a6), _p(T), _f(0.2), _p(v.contiguous()), n, _f(0.5), _p(Rw.contiguous()), _p(Tw), _p(g.contiguous()),
                        _p(world), _p(gS), _p(gR6), _p(gT), _p(gv))
        leaves = [t.clone().requires_grad_(True) for t in (S_raw, a6, T, v)]
        s_, a_, t_, v_ = leaves
        ref = (((v_ * (s_.exp() + 0.2)) @ O.rotation_6d_to_matrix(a_[None])[0] + t_) * 0.5) @ Rw + Tw
        torch.testing.assert_close(world, ref.detach(), rtol=1e-5, atol=1e-5)
        (ref * g).sum().backward()
        for got, leaf in ((gS, s_), (gR6, a_), (gT, t_), (gv, v_)):
            assert float((got - leaf.grad).abs().max()) <= 1e-4 * float(leaf.grad.abs().max()) + 1e-6


# ---- rng_math.h: the counter-based generator of the training step --------------------------------------------------------------------
def _philox_py(ctr, key):
    """Independent restatement of Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)."""
    M0, M1, W0, W1, mask = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xffffffff
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k[0]) & mask, p1 & mask, ((p0 >> 32) ^ c[3] ^ k[1]) & mask, p0 & mask]
        k = [(k[0] + W0) & mask, (k[1] + W1) & mask]
    return c


def test_philox_matches_the_published_known_answers_and_an_independent_restatement():
    L = lib()
    out = (ctypes.c_uint32 * 4)()
    # known-answer vectors of Random123 (kat_vectors: philox4x32 10)
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        L.host_philox(*[ctypes.c_uint32(x) for x in ctr + key], out)
        assert tuple(out) == want == tuple(_philox_py(ctr, key)), (ctr, [hex(x) for x in out])
    rng = np.random.default_rng(0)
    for _ in range(200):
        v = [int(x) for x in rng.integers(0, 2 ** 32, 6)]
        L.host_philox(*[ctypes.c_uint32(x) for x in v], out)
        assert list(out) == _philox_py(v[:4], v[4:])


def test_step_draws_have_the_distributions_the_reference_draws_from():
    """dbw.py:301 draws the opacity noise from N(0, 1) (randn_like), dbw.py:393 the overlap samples from U[0, 1) (torch.rand): moments and
    range of the step's own draws, their dependence on (seed, step) and nothing else."""
    L = lib()
    L.host_step_noise.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]
    L.host_step_uniform.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]
    n = 200000
    z = torch.empty(n)
    L.host_step_noise(227391, 5, n, _p(z))
    assert abs(float(z.mean())) < 0.01 and abs(float(z.std()) - 1) < 0.01 and abs(float((z ** 4).mean()) - 3) < 0.1 and torch.isfinite(z).all()
    u = torch.empty(n, 3)
    L.host_step_uniform(227391, 5, n, _p(u))
    assert float(u.min()) >= 0 and float(u.max()) < 1 and abs(float(u.mean()) - 0.5) < 0.005 and abs(float(u.var()) - 1 / 12) < 0.002
    assert abs(float(torch.corrcoef(u.T)[0, 1])) < 0.01
    z2, z3 = torch.empty(16), torch.empty(16)
    L.host_step_noise(227391, 5, 16, _p(z2))
    L.host_step_noise(227391, 6, 16, _p(z3))
    assert torch.equal(z2, z[:16]) and not torch.equal(z3, z2)          # a function of (seed, step, index): reproducible, fresh every step
    L.host_step_noise(227392, 5, 16, _p(z3))
    assert not torch.equal(z3, z2)
