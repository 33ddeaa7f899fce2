"""Checker side of the intrinsics refinement, shared by tests/test_host_intrinsics_math.py, tests/test_intrinsics_refine_host.py
and tests/test_gpu_intrinsics.py: the host build of csrc/intrinsics_math.h (tests/host_intrinsics_math.cpp) behind tensor-in / tensor-out
functions, the float64 restatement of the parameterisation, the oracle's gradient of K by autograd, and the bars.  The scene, the host
forward and the bound of an fp32 sum are those of tests/pose_ref.py.

Bars.  Gradient of K against autograd of the oracle: 1e-4 * max|g_K|, the bar of the pose tests on the same scene.  Two fp32 evaluations of
the same sum in different orders (host build / kernel / a float64 sum of the same terms): pose_ref.sum_bound, n * 2^-23 * sum|terms| per view
and component, added over the views for the one matrix they share.  Apply / chain: 4 x the error of torch's own fp32 evaluation of the same
formula, floor 1e-6 relative (the rule of the Rodrigues test)."""
import ctypes
import os
import subprocess

import torch

import oracle as O
import pose_ref as PR
from host_build import host_lib

HERE = os.path.dirname(os.path.abspath(__file__))
THETAS = (0.0, 1e-6, -1e-6, 1e-2, -1e-2, 0.5, -0.5)
ZC = PR.ZC
ROWS = (0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15)          # the entries of K (flat) of the twelve accumulators
_p = PR._p


def lib():
    return host_lib('intrinsics_math')


def sanitized_program():
    """tests/_build/host_intrinsics_math_san: tests/host_intrinsics_math.cpp as a program of its own (-DINTRINSICS_MATH_MAIN) under
    -fsanitize=address,undefined."""
    out = os.path.join(HERE, '_build')
    os.makedirs(out, exist_ok=True)
    src, exe = os.path.join(HERE, 'host_intrinsics_math.cpp'), os.path.join(out, 'host_intrinsics_math_san')
    csrc = os.path.join(HERE, '..', 'differentiable-blocksworld_amd', 'csrc')
    deps = [src, os.path.join(HERE, 'host_slot_loop.h')] + [os.path.join(csrc, h) for h in ('intrinsics_math.h', 'camera_math.h', 'raster_math.h')]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in deps):
        subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                               '-DINTRINSICS_MATH_MAIN', src, '-o', exe])
    return exe


# ---- gradient of K --------------------------------------------------------------------------------------------------------------------
def host_intrinsics_grad(verts, faces, R, T, Kmat, cl, g, zc, persp, eps=1e-8):
    """-> g_K (4,4), per-view accumulators (B,12), abs_terms (B,12) float64, n_terms (B) int32, gv (B,2F,3,3): the ndc gradients of every
    slot's three original vertices, of the host build (CPU tensors)."""
    B, F_ = R.shape[0], faces.shape[0]
    gK, gKv = torch.zeros(4, 4), torch.zeros(B, 12)
    at, nt, gv = torch.zeros(B, 12, dtype=torch.float64), torch.zeros(B, dtype=torch.int32), torch.zeros(B, 2 * F_, 3, 3)
    args = [t.contiguous() for t in (verts, faces, R, T, Kmat, cl['num_faces'], cl['c2o'], cl['clip_code'], cl['clip_w'], g)]
    assert lib().host_intrinsics_grad(_p(args[0]), _p(args[1]), _p(args[2]), _p(args[3]), _p(args[4]), B, F_, ctypes.c_float(eps),
                                      ctypes.c_float(zc or 0.0), int(persp), _p(args[5]), _p(args[6]), _p(args[7]), _p(args[8]), _p(args[9]), _p(gK),
                                      _p(gKv), _p(at), _p(nt), _p(gv)) == 0
    return gK, gKv, at, nt, gv


def k_bound(n_terms, abs_terms):
    """(16,) float64: pose_ref.sum_bound of every view, added over the views, at the entries of K the accumulators belong to (row 2: 0)."""
    out = torch.zeros(16, dtype=torch.float64)
    out[list(ROWS)] = PR.sum_bound(n_terms, abs_terms).sum(0)
    return out


def oracle_k_grad(verts, faces, R, T, Kmat, g, zc, persp, dtype=torch.float32):
    """Autograd of O.transform_to_ndc + O.clip_faces with Kmat requiring grad, of sum(face_verts * g) over every view's first num_faces
    slots -> g_K (4,4) (and the oracle's clip dict)."""
    B, Fs = R.shape[0], faces.shape[0]
    Kr = Kmat.to(dtype).clone().requires_grad_(True)
    ndc = O.transform_to_ndc(verts.to(dtype), R.to(dtype), T.to(dtype), Kr, 1e-8)
    ref = O.clip_faces(ndc[:, faces.long()].reshape(B * Fs, 3, 3), torch.arange(B) * Fs, torch.full((B,), Fs), zc, persp)
    loss = 0
    for b in range(B):
        n, s = int(ref['num_faces'][b]), int(ref['first_idx'][b])
        loss = loss + (ref['face_verts'][s:s + n] * g[b, :n].to(dtype)).sum()
    if not torch.is_tensor(loss) or not loss.requires_grad:          # (every face of every view dropped)
        return torch.zeros_like(Kr), ref
    loss.backward()
    return Kr.grad, ref


def k_grad_from_vertex_gradients(verts, faces, R, T, Kmat, cl, gv, b, eps=1e-8):
    """The twelve sums of view b in float64 from the vertex backward's intermediate quantities: gv (B,2F,3,3), the ndc gradient of each
    slot's three original vertices, and the projected view coordinates -- gpx = g.x / denom, gpy = g.y / denom, gpw = -(g.x px + g.y py) /
    denom^2 where |pw| >= eps, each times (vx, vy, vz, 1).  -> (12,) float64."""
    n = int(cl['num_faces'][b])
    vi = faces.long()[cl['c2o'][b, :n].long()].reshape(-1)                                   # (3n,) mesh vertices, slot by slot
    g = gv[b, :n].reshape(-1, 3).double()
    K = Kmat.double()
    v = verts.double()[vi] @ R[b].double() + T[b].double()
    v1 = torch.cat([v, torch.ones(len(v), 1, dtype=torch.float64)], 1)                       # (vx, vy, vz, 1)
    px, py, pw = v1 @ K[0], v1 @ K[1], v1 @ K[3]
    denom = torch.where(pw >= 0, 1.0, -1.0) * pw.abs().clamp(min=eps)
    gpx, gpy = g[:, 0] / denom, g[:, 1] / denom
    gpw = torch.where(pw.abs() >= eps, -(g[:, 0] * px + g[:, 1] * py) / (denom * denom), torch.zeros_like(pw))
    return torch.cat([(gp[:, None] * v1).sum(0) for gp in (gpx, gpy, gpw)])


# ---- refinement -----------------------------------------------------------------------------------------------------------------------
K0 = torch.tensor([[2.1, 0, 0.05, 0], [0, 2.3, -0.03, 0], [0, 0, 0, 1], [0, 0, 1, 0]], dtype=torch.float32)


def refine_torch(K0_, theta, dtype):
    """K' of csrc/intrinsics_math.h in `dtype`, differentiable in theta."""
    K0_, th = K0_.to(dtype), theta.to(dtype)
    K = K0_.clone()
    K[0, 0] = K0_[0, 0] * torch.exp(th[0])
    K[1, 1] = K0_[1, 1] * torch.exp(th[1])
    K[0, 2] = K0_[0, 2] + th[2]
    K[1, 2] = K0_[1, 2] + th[3]
    return K


def theta_case(value, seed):
    """(theta, g_K): the four components of size |value| with the sign of `value` on the scales and alternating on the offsets."""
    gen = torch.Generator().manual_seed(seed)
    theta = torch.tensor([value, value * 0.7, -value * 0.3, value * 0.2], dtype=torch.float32)
    return theta, torch.randn(4, 4, generator=gen)


def intrinsics_reference(K0_, theta, gK):
    """float64 values and the bars from torch's own fp32 evaluation: dict(K, g (4), tol_K, tol_g)."""
    out = {}
    for dtype in (torch.float64, torch.float32):
        th = theta.to(dtype).clone().requires_grad_(True)
        K = refine_torch(K0_, th, dtype)
        (K * gK.to(dtype)).sum().backward()
        out[dtype] = (K.detach().double(), th.grad.double())
    r64, r32 = out[torch.float64], out[torch.float32]
    tol = lambda a64, a32: max(4 * (a32 - a64).abs().max().item(), 1e-6 * a64.abs().max().item())
    return dict(K=r64[0], g=r64[1], tol_K=tol(r64[0], r32[0]), tol_g=tol(r64[1], r32[1]))


def host_intrinsics_apply(K0_, theta):
    K0_, theta = K0_.contiguous(), theta.detach().contiguous()
    K1 = torch.zeros(4, 4)
    assert lib().host_intrinsics_apply(_p(K0_), _p(theta), _p(K1)) == 0
    return K1


def host_intrinsics_chain(K0_, theta, gK):
    K0_, theta, gK = K0_.contiguous(), theta.detach().contiguous(), gK.contiguous()
    gt = torch.zeros(4)
    assert lib().host_intrinsics_chain(_p(K0_), _p(theta), _p(gK), _p(gt)) == 0
    return gt
