"""CPU tests of csrc/icp_math.h built by g++ (tests/host_icp_math.cpp), no GPU needed:
  * the chain from the 2 x 13 sums to the gradients of R6, T, s against torch autograd in fp64, isotropic and anisotropic;
  * the Adam update against torch.optim.Adam in fp32 over 20 steps, bit for bit;
  * the keep-best rule against a ten-line restatement of icp.py:27-28,65-74 on a loss sequence that rises and falls;
  * the transform expression against its numpy restatement, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from dbw_amd import mesh
from host_build import host_lib


def lib():
    L = host_lib('icp_math')
    L.host_icp_grad_MT.restype = ctypes.c_double
    vp = ctypes.c_void_p
    L.host_icp_transform.argtypes = [vp, vp, ctypes.c_longlong, vp]
    L.host_icp_moments.argtypes = [vp, vp, vp, ctypes.c_longlong, vp]
    L.host_icp_step.argtypes = [vp, vp, vp, vp] + [ctypes.c_int] * 5 + [ctypes.c_double, ctypes.c_int, vp, vp]
    L.host_icp_adam.argtypes = [vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double]
    return L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


@pytest.mark.parametrize('anisotropic', [0, 1])
def test_chain_matches_autograd(anisotropic):
    """L = sum(dM * (diag(s) R(R6))) + sum(dT * T) has dL/dM = dM: autograd of it in fp64 is the chain the header writes out.  Bar: fp32
    rounding of a handful of operations, 1e-6 relative to the largest term of the gradient."""
    rng = np.random.default_rng(5 + anisotropic)
    for _ in range(20):
        R6 = (np.array([1, 0, 0, 0, 1, 0]) + 0.4 * rng.standard_normal(6)).astype(np.float32)
        s = (1 + 0.2 * rng.standard_normal(3 if anisotropic else 1)).astype(np.float32)
        dM = rng.standard_normal(9).astype(np.float32)
        s3 = np.ascontiguousarray(np.broadcast_to(s, (3,)), dtype=np.float32)
        gR6, gs = np.zeros(6, np.float32), np.zeros(3, np.float32)
        lib().host_icp_chain(_p(R6), _p(s3), _p(dM), anisotropic, _p(gR6), _p(gs))
        tR6 = torch.tensor(R6, dtype=torch.float64, requires_grad=True)
        ts = torch.tensor(s, dtype=torch.float64, requires_grad=True)
        M = ts.expand(3)[:, None] * mesh.rotation_6d_to_matrix(tR6)
        (M * torch.tensor(dM, dtype=torch.float64).view(3, 3)).sum().backward()
        scale = max(np.abs(dM).max() * max(1.0, np.abs(s).max()), 1.0)
        assert np.abs(gR6 - tR6.grad.numpy()).max() <= 1e-6 * max(scale, tR6.grad.abs().max().item())
        ref_s = ts.grad.numpy()
        assert np.abs(gs[:len(ref_s)] - ref_s).max() <= 1e-6 * 3 * scale
        if not anisotropic:
            assert gs[1] == 0 and gs[2] == 0


def test_sums_to_dM_dT_and_loss():
    rng = np.random.default_rng(0)
    sums = rng.standard_normal(26)
    sums[0], sums[13] = abs(sums[0]), abs(sums[13])
    N, P1, P2 = 3, 2300, 1900
    dM, dT = np.zeros(9, np.float32), np.zeros(3, np.float32)
    loss = lib().host_icp_grad_MT(_p(sums), N, P1, P2, _p(dM), _p(dT))
    w1, w2 = 2 / (N * P1), 2 / (N * P2)
    assert loss == sums[0] / P1 + sums[13] / P2
    assert np.array_equal(dT, (w1 * sums[1:4] + w2 * sums[14:17]).astype(np.float32))
    assert np.array_equal(dM, (w1 * sums[4:13] + w2 * sums[17:26]).astype(np.float32))


@pytest.mark.parametrize('lr', [0.01, 0.3])
def test_adam_matches_torch_bit_for_bit(lr):
    rng = np.random.default_rng(1)
    n, steps = 12, 20
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = (rng.standard_normal((steps, n)) * np.exp(rng.uniform(-12, 2, (steps, n)))).astype(np.float32)
    grads[3, 5] = 0.0
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=lr)
    p, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t in range(steps):
        tp.grad = torch.from_numpy(grads[t].copy())
        opt.step()
        g = np.ascontiguousarray(grads[t])
        lib().host_icp_adam(_p(p), _p(m), _p(v), _p(g), n, 1, t + 1, lr)
        st = opt.state[tp]
        assert np.array_equal(m, st['exp_avg'].numpy()), t
        assert np.array_equal(v, st['exp_avg_sq'].numpy()), t
        assert np.array_equal(p, tp.detach().numpy()), t


def _keep_best_python(losses, N):
    """icp.py:27-28,65-74 with the AverageMeter of utils/metrics.py:17-35"""
    loss_min, best, s, cnt, kept = 1e6, -1, 0.0, 0, []
    for it, loss in enumerate(losses):
        s += loss * N
        cnt += N
        if it % 10 == 0:
            if s / cnt < loss_min:
                loss_min, best = s / cnt, it
                kept.append(it)
            s, cnt = 0.0, 0
    return best, loss_min, kept


@pytest.mark.parametrize('N', [1, 3])
def test_keep_best_rule(N):
    it = np.arange(75)
    seqs = [np.concatenate([[0.5], 0.2 + 0.1 * np.sin(it[1:] / 6.0) + 0.002 * it[1:]]),     # rises and falls: some checks pass, some do not
            np.full(25, 2e6),                                                                # never beats 1e6: nothing kept
            np.linspace(1.0, 0.1, 41),                                                       # every check passes
            np.array([0.3])]
    for losses in seqs:
        losses = np.ascontiguousarray(losses, dtype=np.float64)
        kept = np.zeros(len(losses), np.int32)
        lmin = ctypes.c_double()
        best = lib().host_icp_keep_best(_p(losses), len(losses), N, _p(kept), ctypes.byref(lmin))
        ref_best, ref_min, ref_kept = _keep_best_python(losses.tolist(), N)
        assert best == ref_best and lmin.value == ref_min and np.flatnonzero(kept).tolist() == ref_kept
    assert _keep_best_python(seqs[0].tolist(), 1)[2] not in ([], list(range(0, 75, 10)))
    assert _keep_best_python(seqs[1].tolist(), 1)[0] == -1


def test_transform_expression():
    rng = np.random.default_rng(2)
    rts = rng.standard_normal(15).astype(np.float32)
    p = rng.standard_normal((101, 3)).astype(np.float32)
    q = np.zeros_like(p)
    lib().host_icp_transform(_p(rts), _p(p), len(p), _p(q))
    M = (rts[12:15, None] * rts[:9].reshape(3, 3)).astype(np.float32)
    ref = ((p[:, 0:1] * M[0] + p[:, 1:2] * M[1]) + p[:, 2:3] * M[2]) + rts[9:12]
    assert ref.dtype == np.float32 and np.array_equal(q, ref)
