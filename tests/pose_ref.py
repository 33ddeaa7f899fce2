"""Checker side of the camera pose refinement, shared by tests/test_host_pose_math.py, tests/test_pose_refine_host.py and
tests/test_gpu_pose.py: the host build of csrc/pose_math.h (tests/host_pose_math.cpp) behind tensor-in / tensor-out functions, the float64
restatement of the refinement (torch.matrix_exp of the skew matrix, autograd), the oracle's camera gradient by autograd, and the bars.

Bars.  Camera gradient against autograd of the oracle: 1e-4 * max|grad| per tensor, the project's bar for the vertex backward on the same
scene.  Two fp32 evaluations of the same sum in different orders (host build / kernel / the existing vertex backward): n * 2^-23 * sum|terms|
per component -- each order is within (n - 1) * 2^-24 * sum|terms| of the exact sum of its terms -- with n the number of terms: a term is
what one vertex of one slot adds, and the host build counts them (vertices whose gradient is all zero add nothing and are not counted).
Rodrigues: 4 x the error of torch's own fp32 evaluation of the same formula, floor 1e-6 relative (the rule of tests/masked_loss_ref.py)."""
import ctypes
import math
import os
import subprocess

import torch

import oracle as O
from host_build import host_lib
from test_host_camera_math import _scene, host_project_clip      # noqa: F401  (the camera tests' scene and host forward)

HERE = os.path.dirname(os.path.abspath(__file__))
ANGLES = (0.0, 1e-8, 1e-4, 1e-2, 1.0, math.pi - 1e-3)
ZC = 0.25


def lib():
    return host_lib('pose_math')


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def sanitized_program():
    """tests/_build/host_pose_math_san: tests/host_pose_math.cpp as a program of its own (-DPOSE_MATH_MAIN) under -fsanitize=address,undefined."""
    out = os.path.join(HERE, '_build')
    os.makedirs(out, exist_ok=True)
    src, exe = os.path.join(HERE, 'host_pose_math.cpp'), os.path.join(out, 'host_pose_math_san')
    csrc = os.path.join(HERE, '..', 'differentiable-blocksworld_amd', 'csrc')
    deps = [src, os.path.join(HERE, 'host_slot_loop.h')] + [os.path.join(csrc, h) for h in ('pose_math.h', 'camera_math.h', 'raster_math.h')]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in deps):
        subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                               '-DPOSE_MATH_MAIN', src, '-o', exe])
    return exe


# ---- camera gradient ------------------------------------------------------------------------------------------------------------------
def scene(seed, B=3):
    """The scene of tests/test_host_camera_math.py (its _scene, imported: one definition): an icosphere around the cameras, many faces straddle
    z = ZC."""
    return _scene(seed, B=B)


def host_pose_grad(verts, faces, R, T, Kmat, cl, g, zc, persp, eps=1e-8):
    """-> g_R (B,3,3), g_T (B,3), abs_terms (B,12) float64, n_terms (B) int32 of the host build (CPU tensors)."""
    B, F_ = R.shape[0], faces.shape[0]
    gR, gT, at, nt = torch.zeros(B, 3, 3), torch.zeros(B, 3), torch.zeros(B, 12, dtype=torch.float64), torch.zeros(B, dtype=torch.int32)
    args = [t.contiguous() for t in (verts, faces, R, T, Kmat, cl['num_faces'], cl['c2o'], cl['clip_code'], cl['clip_w'], g)]
    assert lib().host_pose_grad(_p(args[0]), _p(args[1]), _p(args[2]), _p(args[3]), _p(args[4]), B, F_, ctypes.c_float(eps), ctypes.c_float(zc or 0.0),
                                int(persp), _p(args[5]), _p(args[6]), _p(args[7]), _p(args[8]), _p(args[9]), _p(gR), _p(gT), _p(at), _p(nt)) == 0
    return gR, gT, at, nt


def sum_bound(n_terms, abs_terms):
    """(B,12) float64: n * 2^-23 * sum|terms| per view and component, n the number of terms (module docstring)."""
    return n_terms.double()[:, None] * 2.0 ** -23 * abs_terms


def oracle_cam_grad(verts, faces, R, T, Kmat, g, zc, persp, dtype=torch.float32):
    """Autograd of O.transform_to_ndc + O.clip_faces with R, T requiring grad, of sum(face_verts * g) over every view's first num_faces
    slots -> g_R, g_T (and the oracle's clip dict)."""
    B, Fs = R.shape[0], faces.shape[0]
    Rr, Tr = R.to(dtype).clone().requires_grad_(True), T.to(dtype).clone().requires_grad_(True)
    ndc = O.transform_to_ndc(verts.to(dtype), Rr, Tr, Kmat.to(dtype), 1e-8)
    ref = O.clip_faces(ndc[:, faces.long()].reshape(B * Fs, 3, 3), torch.arange(B) * Fs, torch.full((B,), Fs), zc, persp)
    loss = 0
    for b in range(B):
        n, s = int(ref['num_faces'][b]), int(ref['first_idx'][b])
        loss = loss + (ref['face_verts'][s:s + n] * g[b, :n].to(dtype)).sum()
    if not torch.is_tensor(loss) or not loss.requires_grad:          # (every face of every view dropped)
        return torch.zeros_like(Rr), torch.zeros_like(Tr), ref
    loss.backward()
    return Rr.grad, Tr.grad, ref


# ---- refinement -----------------------------------------------------------------------------------------------------------------------
def skew(w):
    """[w]x with the sign convention of csrc/pose_math.h: K x = w x x for a column x."""
    z = torch.zeros((), dtype=w.dtype)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def refine_torch(R0, T0, delta, dtype):
    """R' = R0.E(w), T' = T0.E(w) + tau for ONE view, E = matrix_exp([w]x), in `dtype` (differentiable in delta)."""
    d = delta.to(dtype)
    E = torch.matrix_exp(skew(d[:3]))
    return R0.to(dtype) @ E, T0.to(dtype) @ E + d[3:], E


def pose_case(angle, seed):
    """One view's (R0, T0, delta, gR, gT) in fp32: a random rotation-like R0, |w| = angle about a random axis, tau of a few percent."""
    gen = torch.Generator().manual_seed(seed)
    axis = torch.randn(3, generator=gen, dtype=torch.float64)
    w = (axis / axis.norm() * angle).float()
    tau = 0.05 * torch.randn(3, generator=gen)
    R0, _ = O.look_at_cameras(torch.randn(1, 3, generator=gen) * 0.4, at=(0.3, 0.2, 2.5))
    T0 = torch.randn(3, generator=gen)
    return R0[0].contiguous(), T0, torch.cat([w, tau]).contiguous(), torch.randn(3, 3, generator=gen), torch.randn(3, generator=gen)


def pose_reference(R0, T0, delta, gR, gT):
    """float64 values and the bars from torch's own fp32 evaluation: dict(R, T, E, g (6), tol_R, tol_T, tol_E, tol_gw, tol_gt)."""
    out = {}
    for dtype in (torch.float64, torch.float32):
        d = delta.to(dtype).clone().requires_grad_(True)
        R1, T1, E = refine_torch(R0, T0, d, dtype)
        ((R1 * gR.to(dtype)).sum() + (T1 * gT.to(dtype)).sum()).backward()
        out[dtype] = (R1.detach().double(), T1.detach().double(), E.detach().double(), d.grad.double())
    r64, r32 = out[torch.float64], out[torch.float32]
    tol = lambda a64, a32: max(4 * (a32 - a64).abs().max().item(), 1e-6 * a64.abs().max().item())
    return dict(R=r64[0], T=r64[1], E=r64[2], g=r64[3], tol_R=tol(r64[0], r32[0]), tol_T=tol(r64[1], r32[1]), tol_E=tol(r64[2], r32[2]),
                tol_gw=tol(r64[3][:3], r32[3][:3]), tol_gt=tol(r64[3][3:], r32[3][3:]))


def host_rodrigues(w):
    E = torch.zeros(3, 3)
    assert lib().host_rodrigues(_p(w.contiguous()), _p(E)) == 0
    return E


def host_pose_apply(R0, T0, delta, ids):
    R0, T0, delta, ids = R0.contiguous(), T0.contiguous(), delta.detach().contiguous(), ids.to(torch.int32).contiguous()
    R1, T1 = torch.zeros_like(R0), torch.zeros_like(T0)
    assert lib().host_pose_apply(_p(R0), _p(T0), _p(delta), _p(ids), R0.shape[0], delta.shape[0], _p(R1), _p(T1)) == 0
    return R1, T1


def host_pose_chain(R0, T0, delta, ids, gR, gT):
    R0, T0, delta, ids, gR, gT = R0.contiguous(), T0.contiguous(), delta.detach().contiguous(), ids.to(torch.int32).contiguous(), gR.contiguous(), gT.contiguous()
    gd = torch.zeros_like(delta)
    assert lib().host_pose_chain(_p(R0), _p(T0), _p(delta), _p(ids), R0.shape[0], delta.shape[0], _p(gR), _p(gT), _p(gd)) == 0
    return gd
