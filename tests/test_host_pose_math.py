"""CPU tests of the camera pose refinement arithmetic: csrc/pose_math.h, the header csrc/camera_grad.hip compiles, built for
the host by g++ (tests/host_pose_math.cpp).  The gradient of the clipped faces with respect to R and T against autograd of the oracle's
transform_to_ndc + clip_faces on a scene where every clipping case occurs, and against the existing vertex backward; the Rodrigues forward
and backward against a float64 restatement; the same file once as a program of its own under -fsanitize=address,undefined.
tests/pose_ref.py has the helpers and says where each bar comes from."""
import ctypes
import subprocess

import pytest
import torch

import pose_ref as PR
from host_build import host_lib

_p = PR._p


@pytest.mark.parametrize('persp', [True, False])
def test_camera_gradient_matches_autograd_of_the_oracle(persp):
    verts, faces, R, T, Kmat = PR.scene(4)
    B, Fs = R.shape[0], faces.shape[0]
    cl = PR.host_project_clip(verts, faces, R, T, Kmat, PR.ZC, persp)
    kinds = {int(k) for b in range(B) for k in (cl['clip_code'][b, :int(cl['num_faces'][b])] >> 2).unique()}
    assert kinds == {-1, 0, 1, 2}, f'the test scene must exercise untouched faces and clip kinds 0, 1, 2: {kinds}'
    g = torch.randn(B, 2 * Fs, 3, 3, generator=torch.Generator().manual_seed(1))
    gR, gT, _, _ = PR.host_pose_grad(verts, faces, R, T, Kmat, cl, g, PR.ZC, persp)
    rR, rT, ref = PR.oracle_cam_grad(verts, faces, R, T, Kmat, g, PR.ZC, persp)
    assert torch.equal(cl['num_faces'].long(), ref['num_faces']) and (ref['neighbor'] >= 0).any() and ref['has_conv'].any()
    eR, eT = float((gR - rR).abs().max()), float((gT - rT).abs().max())
    print(f'persp={persp}: g_R err {eR:.3e} (max {float(rR.abs().max()):.3e}), g_T err {eT:.3e} (max {float(rT.abs().max()):.3e})')
    assert eR <= 1e-4 * float(rR.abs().max()) and eT <= 1e-4 * float(rT.abs().max())


def test_the_oracle_in_fp32_is_far_inside_the_bar():
    """The reference's own error: its fp32 evaluation against its fp64 one stays an order below the 1e-4 bar (1.2e-6 relative here), so the
    bar measures the header, not the reference."""
    verts, faces, R, T, Kmat = PR.scene(4)
    g = torch.randn(R.shape[0], 2 * faces.shape[0], 3, 3, generator=torch.Generator().manual_seed(1))
    r32 = PR.oracle_cam_grad(verts, faces, R, T, Kmat, g, PR.ZC, True)
    r64 = PR.oracle_cam_grad(verts, faces, R, T, Kmat, g, PR.ZC, True, dtype=torch.float64)
    for a, b in zip(r32[:2], r64[:2]):
        assert float((a.double() - b).abs().max()) <= 1e-5 * float(b.abs().max())


@pytest.mark.parametrize('persp', [True, False])
def test_camera_gradient_is_the_vertex_backward_seen_from_the_camera(persp):
    """For one view g_T = sum_v R^T gworld_v and g_R = sum_v X_v (x) R^T gworld_v with gworld what host_project_clip_bwd returns for that view."""
    verts, faces, R, T, Kmat = PR.scene(4)
    B, Fs = R.shape[0], faces.shape[0]
    cl = PR.host_project_clip(verts, faces, R, T, Kmat, PR.ZC, persp)
    g = torch.randn(B, 2 * Fs, 3, 3, generator=torch.Generator().manual_seed(2))
    gR, gT, abs_terms, n_terms = PR.host_pose_grad(verts, faces, R, T, Kmat, cl, g, PR.ZC, persp)
    assert torch.equal(n_terms, 3 * cl['num_faces'])                 # a random gradient: every vertex of every slot is a term
    bound = PR.sum_bound(n_terms, abs_terms)
    for b in range(B):
        gworld = torch.zeros_like(verts)
        assert host_lib('camera_math').host_project_clip_bwd(_p(verts), _p(faces), _p(R), _p(T), _p(Kmat), b, Fs, ctypes.c_float(1e-8),
                                                             ctypes.c_float(PR.ZC), int(persp), int(cl['num_faces'][b]), _p(cl['c2o']), _p(cl['clip_code']),
                                                             _p(cl['clip_w']), _p(g), _p(gworld)) == 0
        gview = gworld.double() @ R[b].double()                     # R^T gworld as row vectors
        want_T, want_R = gview.sum(0), verts.double().t() @ gview
        eT, eR = (gT[b].double() - want_T).abs(), (gR[b].double() - want_R).abs()
        print(f'view {b}: g_T err {eT.max():.3e} (bound {bound[b, 9:].min():.3e}), g_R err {eR.max():.3e} (bound {bound[b, :9].min():.3e})')
        assert bool((eT <= bound[b, 9:]).all()) and bool((eR.reshape(-1) <= bound[b, :9]).all())


def test_slots_behind_num_faces_reach_nothing():
    verts, faces, R, T, Kmat = PR.scene(4)
    cl = PR.host_project_clip(verts, faces, R, T, Kmat, PR.ZC, True)
    g = torch.randn(R.shape[0], 2 * faces.shape[0], 3, 3, generator=torch.Generator().manual_seed(3))
    a = PR.host_pose_grad(verts, faces, R, T, Kmat, cl, g, PR.ZC, True)
    for b in range(R.shape[0]):
        g[b, int(cl['num_faces'][b]):] = 1e30
    b_ = PR.host_pose_grad(verts, faces, R, T, Kmat, cl, g, PR.ZC, True)
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1])


@pytest.mark.parametrize('angle', PR.ANGLES, ids=[f'{a:.3g}' for a in PR.ANGLES])
def test_rodrigues_forward_and_backward_against_fp64(angle):
    for seed in range(3):
        R0, T0, delta, gR, gT = PR.pose_case(angle, seed)
        ref = PR.pose_reference(R0, T0, delta, gR, gT)
        ids = torch.zeros(1, dtype=torch.int32)
        E = PR.host_rodrigues(delta[:3])
        R1, T1 = PR.host_pose_apply(R0[None], T0[None], delta[None], ids)
        gd = PR.host_pose_chain(R0[None], T0[None], delta[None], ids, gR[None], gT[None])[0]
        errs = dict(E=float((E.double() - ref['E']).abs().max()), R=float((R1[0].double() - ref['R']).abs().max()),
                    T=float((T1[0].double() - ref['T']).abs().max()), gw=float((gd[:3].double() - ref['g'][:3]).abs().max()),
                    gt=float((gd[3:].double() - ref['g'][3:]).abs().max()))
        print(f'|w|={angle:.3g} seed {seed}: ' + ', '.join(f'{k} err {v:.2e} (bar {ref["tol_" + k]:.2e})' for k, v in errs.items()))
        for k, v in errs.items():
            assert v <= ref['tol_' + k], (k, v, ref['tol_' + k])


def test_zero_refinement_is_the_identity_bit_for_bit():
    R0, T0, delta, gR, gT = PR.pose_case(0.0, 7)
    assert not delta[:3].any() and delta[3:].any()
    assert torch.equal(PR.host_rodrigues(delta[:3]), torch.eye(3))
    R1, T1 = PR.host_pose_apply(R0[None], T0[None], delta[None], torch.zeros(1, dtype=torch.int32))
    assert torch.equal(R1[0], R0) and torch.equal(T1[0], T0 + delta[3:])
    # the gradient in w at 0 is the contraction of g_E with the three generators: g_w = (gE[2][1] - gE[1][2], gE[0][2] - gE[2][0], gE[1][0] - gE[0][1])
    gE = R0.double().t() @ gR.double() + torch.outer(T0.double(), gT.double())
    want = torch.stack([gE[2, 1] - gE[1, 2], gE[0, 2] - gE[2, 0], gE[1, 0] - gE[0, 1]])
    gd = PR.host_pose_chain(R0[None], T0[None], delta[None], torch.zeros(1, dtype=torch.int32), gR[None], gT[None])[0]
    ref = PR.pose_reference(R0, T0, delta, gR, gT)
    assert float((ref['g'][:3] - want).abs().max()) <= 1e-12                 # (the float64 restatement agrees with the generators)
    assert float((gd[:3].double() - want).abs().max()) <= ref['tol_gw'] and torch.equal(gd[3:], gT)


def test_an_id_outside_the_table_changes_nothing():
    R0, T0, delta, gR, gT = PR.pose_case(1.0, 3)
    R1, T1 = PR.host_pose_apply(R0[None], T0[None], delta[None], torch.tensor([5], dtype=torch.int32))
    assert torch.equal(R1[0], R0) and torch.equal(T1[0], T0)


def test_sanitized_program_runs_clean():
    r = subprocess.run([PR.sanitized_program()], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.count(': ok') == len(PR.ANGLES) + 2
