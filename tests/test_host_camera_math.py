"""CPU tests of the product's camera transform + near-plane clipping arithmetic (csrc/camera_math.h, the header project_clip.hip
compiles) built for the host with g++ (tests/host_camera_math.cpp): bit-exact clipped faces and identical bookkeeping against the
oracle's transform_to_ndc + clip_faces on a scene that exercises every clipping case, and the hand-derived backward
against autograd of the oracle.  The GPU test (tests/test_gpu_parity.py::test_project_clip_bit_exact) holds the kernel to the same."""
import ctypes

import pytest
import torch

import oracle as O
from host_build import host_lib


def lib():
    return host_lib('camera_math')


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _scene(seed, B=3):
    """A closed icosphere around the cameras (like the sky dome): many faces straddle z = z_clip (cases 3 and 4)."""
    torch.manual_seed(seed)
    verts, faces = O.get_icosphere(2, flip_faces=True)
    verts = verts * 3.0 + 0.05 * torch.randn_like(verts)
    C = torch.randn(B, 3) * 0.4
    R, T = O.look_at_cameras(C, at=(0.3, 0.2, 2.5))
    Kmat = torch.tensor([[2.1, 0, 0.05, 0], [0, 2.1, -0.03, 0], [0, 0, 0, 1], [0, 0, 1, 0]], dtype=torch.float32)
    return verts.contiguous(), faces.to(torch.int32).contiguous(), R.contiguous(), T.contiguous(), Kmat


def host_project_clip(verts, faces, R, T, Kmat, zc, persp):
    B, F_ = R.shape[0], faces.shape[0]
    fvc = torch.zeros(B, 2 * F_, 3, 3)
    num = torch.zeros(B, dtype=torch.int32)
    c2o, nbr, code = [torch.full((B, 2 * F_), -7, dtype=torch.int32) for _ in range(3)]
    cw = torch.zeros(B, 2 * F_, 2)
    assert lib().host_project_clip(_p(verts), _p(faces), _p(R), _p(T), _p(Kmat), B, verts.shape[0], F_, ctypes.c_float(1e-8), int(zc is not None),
                                   ctypes.c_float(zc or 0.0), int(persp), _p(fvc), _p(num), _p(c2o), _p(nbr), _p(code), _p(cw)) == 0
    return dict(face_verts=fvc, num_faces=num, c2o=c2o, neighbor=nbr, clip_code=code, clip_w=cw)


@pytest.mark.parametrize('persp', [True, False])
def test_projection_and_clipping_are_bit_exact_against_the_oracle(persp):
    verts, faces, R, T, Kmat = _scene(0)
    B, Fs = R.shape[0], faces.shape[0]
    zc = 0.25
    ndc = O.transform_to_ndc(verts, R, T, Kmat, 1e-8)
    fv = ndc[:, faces.long()].reshape(B * Fs, 3, 3)
    ref = O.clip_faces(fv, torch.arange(B) * Fs, torch.full((B,), Fs), zc, persp)
    cl = host_project_clip(verts, faces, R, T, Kmat, zc, persp)
    assert torch.equal(cl['num_faces'].long(), ref['num_faces'])
    assert (ref['neighbor'] >= 0).any() and ref['has_conv'].any(), 'test scene must exercise cases 3 and 4'
    for b in range(B):
        n, s = int(cl['num_faces'][b]), int(ref['first_idx'][b])
        assert torch.equal(cl['face_verts'][b, :n], ref['face_verts'][s:s + n]), f'view {b}'
        assert torch.equal(cl['c2o'][b, :n].long(), ref['clipped_to_orig'][s:s + n] - b * Fs)
        nb_ref = ref['neighbor'][s:s + n]
        nb_ref = torch.where(nb_ref >= 0, nb_ref - s + b * 2 * Fs, nb_ref)
        assert torch.equal(cl['neighbor'][b, :n].long(), nb_ref)
        assert torch.equal(cl['clip_code'][b, :n] >= 0, ref['has_conv'][s:s + n])
    # no clipping plane: plain projection
    cl0 = host_project_clip(verts, faces, R, T, Kmat, None, persp)
    assert torch.all(cl0['num_faces'] == Fs) and torch.equal(cl0['face_verts'][:, :Fs], ndc[:, faces.long()])


@pytest.mark.parametrize('persp', [True, False])
def test_projection_and_clipping_backward_matches_autograd_of_the_oracle(persp):
    verts, faces, R, T, Kmat = _scene(4)
    B, Fs = R.shape[0], faces.shape[0]
    zc = 0.25
    cl = host_project_clip(verts, faces, R, T, Kmat, zc, persp)
    g = torch.randn(B, 2 * Fs, 3, 3, generator=torch.Generator().manual_seed(1))
    gverts = torch.zeros_like(verts)
    for b in range(B):
        assert lib().host_project_clip_bwd(_p(verts), _p(faces), _p(R), _p(T), _p(Kmat), b, Fs, ctypes.c_float(1e-8), ctypes.c_float(zc), int(persp),
                                           int(cl['num_faces'][b]), _p(cl['c2o']), _p(cl['clip_code']), _p(cl['clip_w']), _p(g), _p(gverts)) == 0
    v = verts.clone().requires_grad_(True)
    ndc = O.transform_to_ndc(v, R, T, Kmat, 1e-8)
    ref = O.clip_faces(ndc[:, faces.long()].reshape(B * Fs, 3, 3), torch.arange(B) * Fs, torch.full((B,), Fs), zc, persp)
    loss = 0
    for b in range(B):
        n, s = int(ref['num_faces'][b]), int(ref['first_idx'][b])
        loss = loss + (ref['face_verts'][s:s + n] * g[b, :n]).sum()
    loss.backward()
    assert float((gverts - v.grad).abs().max()) <= 1e-4 * float(v.grad.abs().max())
