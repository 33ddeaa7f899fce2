"""CPU tests of the intrinsics refinement arithmetic: csrc/intrinsics_math.h, the header csrc/camera_grad.hip compiles,
built for the host by g++ (tests/host_intrinsics_math.cpp).  The gradient of the clipped faces with respect to K against autograd of the
oracle's transform_to_ndc + clip_faces on a scene where every clipping case occurs, and against a float64 sum over the vertex backward's
own intermediate quantities; the parameterisation and its chain rule against a float64 restatement; the same file once as a program of its
own under -fsanitize=address,undefined.  tests/intrinsics_ref.py has the helpers and says where each bar comes from."""
import subprocess

import pytest
import torch

import intrinsics_ref as IR
import pose_ref as PR


def _inputs(persp, seed):
    verts, faces, R, T, Kmat = PR.scene(4)
    cl = PR.host_project_clip(verts, faces, R, T, Kmat, IR.ZC, persp)
    g = torch.randn(R.shape[0], 2 * faces.shape[0], 3, 3, generator=torch.Generator().manual_seed(seed))
    return verts, faces, R, T, Kmat, cl, g


@pytest.mark.parametrize('persp', [True, False])
def test_k_gradient_matches_autograd_of_the_oracle(persp):
    verts, faces, R, T, Kmat, cl, g = _inputs(persp, 1)
    B = R.shape[0]
    kinds = {int(k) for b in range(B) for k in (cl['clip_code'][b, :int(cl['num_faces'][b])] >> 2).unique()}
    assert kinds == {-1, 0, 1, 2}, f'the test scene must exercise untouched faces and clip kinds 0, 1, 2: {kinds}'
    gK = IR.host_intrinsics_grad(verts, faces, R, T, Kmat, cl, g, IR.ZC, persp)[0]
    rK, ref = IR.oracle_k_grad(verts, faces, R, T, Kmat, g, IR.ZC, persp)
    assert torch.equal(cl['num_faces'].long(), ref['num_faces']) and (ref['neighbor'] >= 0).any() and ref['has_conv'].any()
    err = float((gK - rK).abs().max())
    print(f'persp={persp}: g_K err {err:.3e} (max {float(rK.abs().max()):.3e})')
    assert err <= 1e-4 * float(rK.abs().max())
    assert not gK[2].any() and not rK[2].any()                     # row 2 is never read: exactly 0 on both sides
    assert bool(gK[[0, 1, 3]].ne(0).all())                         # ... and the other twelve entries all receive something


def test_the_oracle_in_fp32_is_far_inside_the_bar():
    """The reference's own error: its fp32 evaluation against its fp64 one has to sit at least 10 x inside the 1e-4 bar (measured: 3.4e-7
    relative, persp true; 4.6e-7, persp false), so the bar measures the header, not the reference."""
    for persp in (True, False):
        verts, faces, R, T, Kmat, cl, g = _inputs(persp, 1)
        r32 = IR.oracle_k_grad(verts, faces, R, T, Kmat, g, IR.ZC, persp)[0]
        r64 = IR.oracle_k_grad(verts, faces, R, T, Kmat, g, IR.ZC, persp, dtype=torch.float64)[0]
        rel = float((r32.double() - r64).abs().max() / r64.abs().max())
        print(f'persp={persp}: the oracle in fp32 against fp64: {rel:.3e} relative')
        assert rel <= 1e-5


@pytest.mark.parametrize('persp', [True, False])
def test_k_gradient_is_the_sum_over_the_vertex_backward_quantities(persp):
    """Per view, the twelve accumulators against the float64 sum of gp (x) (vx, vy, vz, 1) over the vertices of the view's slots, gp formed
    from the ndc gradients clip_slot_bwd hands to the vertex backward and the projected view coordinates (intrinsics_ref.
    k_grad_from_vertex_gradients), within the derived fp32 sum error n * 2^-23 * sum|terms|."""
    verts, faces, R, T, Kmat, cl, g = _inputs(persp, 2)
    B = R.shape[0]
    gK, gKv, abs_terms, n_terms, gv = IR.host_intrinsics_grad(verts, faces, R, T, Kmat, cl, g, IR.ZC, persp)
    assert torch.equal(n_terms, 3 * cl['num_faces'])                 # a random gradient: every vertex of every slot is a term
    bound = PR.sum_bound(n_terms, abs_terms)
    total = torch.zeros(12, dtype=torch.float64)
    for b in range(B):
        want = IR.k_grad_from_vertex_gradients(verts, faces, R, T, Kmat, cl, gv, b)
        err = (gKv[b].double() - want).abs()
        print(f'view {b}: err {err.max():.3e} (smallest bound {bound[b].min():.3e}, n = {int(n_terms[b])})')
        assert bool((err <= bound[b]).all())
        total += want
    # the matrix: the views' sums added (one fp64 sum rounded once, against the sum of the bounds)
    assert bool(((gK.reshape(-1)[list(IR.ROWS)].double() - total).abs() <= bound.sum(0) + 2.0 ** -24 * total.abs()).all())


def test_slots_behind_num_faces_reach_nothing():
    verts, faces, R, T, Kmat, cl, g = _inputs(True, 3)
    a = IR.host_intrinsics_grad(verts, faces, R, T, Kmat, cl, g, IR.ZC, True)
    for b in range(R.shape[0]):
        g[b, int(cl['num_faces'][b]):] = 1e30
    b_ = IR.host_intrinsics_grad(verts, faces, R, T, Kmat, cl, g, IR.ZC, True)
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1])


def test_zero_refinement_returns_k0_bit_for_bit():
    for K0 in (IR.K0, PR.scene(4)[4], torch.randn(4, 4, generator=torch.Generator().manual_seed(5))):
        assert torch.equal(IR.host_intrinsics_apply(K0, torch.zeros(4)), K0)
        gK = torch.randn(4, 4, generator=torch.Generator().manual_seed(6))
        want = torch.stack([gK[0, 0] * K0[0, 0], gK[1, 1] * K0[1, 1], gK[0, 2], gK[1, 2]])
        assert torch.equal(IR.host_intrinsics_chain(K0, torch.zeros(4), gK), want)


@pytest.mark.parametrize('value', IR.THETAS, ids=[f'{v:g}' for v in IR.THETAS])
def test_apply_and_chain_against_fp64(value):
    for seed in range(3):
        theta, gK = IR.theta_case(value, seed)
        ref = IR.intrinsics_reference(IR.K0, theta, gK)
        K1, gt = IR.host_intrinsics_apply(IR.K0, theta), IR.host_intrinsics_chain(IR.K0, theta, gK)
        eK, eg = float((K1.double() - ref['K']).abs().max()), float((gt.double() - ref['g']).abs().max())
        print(f'theta={value:g} seed {seed}: K err {eK:.2e} (bar {ref["tol_K"]:.2e}), g_theta err {eg:.2e} (bar {ref["tol_g"]:.2e})')
        assert eK <= ref['tol_K'] and eg <= ref['tol_g']
        untouched = torch.ones(4, 4, dtype=torch.bool)
        untouched[0, 0] = untouched[1, 1] = untouched[0, 2] = untouched[1, 2] = False
        assert torch.equal(K1[untouched], IR.K0[untouched])         # twelve entries are K0's own


def test_sanitized_program_runs_clean():
    r = subprocess.run([IR.sanitized_program()], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.count(': ok') == len(IR.THETAS) + 2
