"""CPU: the host build of csrc/plane_math.h (tests/host_plane_math.cpp) against an independent Philox restatement, fp64 numpy and the
reference's own Ransac (tests/golden/ransac_plane.npz)."""
import ctypes
import math

import numpy as np

import plane_ref as PR
import worldfit_fixture as WF


def _philox(counter, key):
    """Philox4x32-10 of the paper (Salmon et al., SC'11), on Python integers"""
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xffffffff, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xffffffff]
        k = [(k[0] + 0x9E3779B9) & 0xffffffff, (k[1] + 0xBB67AE85) & 0xffffffff]
    return c


def test_philox_restatement_known_answer():
    # the published vectors of Random123 (kat_vectors): counter and key of zeros, of ones
    assert _philox([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert _philox([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_plane_draw_matches_the_restatement():
    from dbw_amd import eval3d
    L, idx = PR.lib(), (ctypes.c_int32 * 3)()
    for seed, N in ((0, 3), (1, 4097), (0xfedcba9876543210, (1 << 31) - 1), (1 << 32, 1000)):
        drawn = eval3d.plane_draw(seed, 40, N)
        for j in (0, 1, 7, 39):
            L.host_plane_draw(ctypes.c_uint64(seed), ctypes.c_uint32(j), ctypes.c_int64(N), idx)
            w = _philox([j, 0, 0, 0x504C414E], [seed & 0xffffffff, seed >> 32])
            assert list(idx) == [(w[k] * N) >> 32 for k in range(3)] == drawn[j].tolist()
            assert all(0 <= i < N for i in idx)


def test_plane_from_triple_residuals_and_counts_against_fp64():
    rng = np.random.RandomState(0)
    pts = rng.randn(500, 3).astype(np.float32)
    p64 = pts.astype(np.float64)
    L = PR.lib()
    for trial in range(50):
        a, b, c = pts[rng.choice(500, 3, replace=False)]
        up = rng.randn(3).astype(np.float32) if trial % 2 else None
        for mode in (PR.ORTHOGONAL, PR.VERTICAL):
            ok, pl = PR.from_triple(a, b, c, mode, up)
            assert ok
            m = np.cross(b.astype(np.float64) - a, c.astype(np.float64) - a)
            n = m / m[2] if mode == PR.VERTICAL else m / np.linalg.norm(m)
            if mode == PR.ORTHOGONAL and up is not None and n @ up < 0:
                n = -n
            d = n @ a
            # fp32 against fp64.  The edges carry eps |coordinate| each, the products of the cross product eps |e1||e2|; what divides, |m| or
            # m.z, is smaller than |e1||e2| by kappa, so a component of n is off by about eps kappa (1 + |coordinate| / |edge|) |n|: 16 of
            # those are allowed.  d = n . a sums three such errors times |a|, and rounds.
            e1, e2 = np.linalg.norm(b - a), np.linalg.norm(c - a)
            kappa = e1 * e2 / (abs(m[2]) if mode == PR.VERTICAL else np.linalg.norm(m))
            tol = 16 * 2.0 ** -24 * kappa * (1 + np.abs([a, b, c]).max() / min(e1, e2)) * max(1.0, np.abs(n).max())
            assert np.abs(pl[:3] - n).max() <= tol and abs(pl[3] - d) <= 3 * np.abs(a).max() * tol + 4 * 2.0 ** -24 * max(1.0, abs(d)), (trial, mode)
            if mode == PR.VERTICAL:
                assert pl[2] == 1.0
            r = np.zeros(500, np.float32)
            L.host_plane_residuals(PR._ptr(pl), PR._ptr(pts), ctypes.c_int64(500), PR._ptr(r))
            r64 = p64 @ pl[:3].astype(np.float64) - float(pl[3])
            assert np.abs(r - r64).max() <= 4 * 2.0 ** -24 * (np.abs(p64) @ np.abs(pl[:3].astype(np.float64)) + abs(float(pl[3]))).max()
            thresh2 = np.float32(0.3)
            got = L.host_plane_count(PR._ptr(pl), PR._ptr(pts), ctypes.c_int64(500), ctypes.c_float(thresh2))
            edge = int((np.abs(r64 ** 2 - float(thresh2)) < 1e-5).sum())
            assert abs(got - int((r64 ** 2 < float(thresh2)).sum())) <= edge


def test_degenerate_triples():
    a, b = np.array([0.1, 0.2, 0.3], np.float32), np.array([1.0, -1.0, 0.5], np.float32)
    for mode in (PR.ORTHOGONAL, PR.VERTICAL):
        assert not PR.from_triple(a, a, b, mode)[0]                              # a repeated index
        assert not PR.from_triple(a, b, b, mode)[0]
        assert not PR.from_triple(a, b, a + 2.5 * (b - a), mode)[0]              # collinear
        ok, pl = PR.from_triple(a, b, a + 2.5 * (b - a), mode)
        assert not ok and not pl.any()
        assert not PR.from_triple(a, b, np.array([np.inf, 0, 0], np.float32), mode)[0]
    # a vertical triangle: m.z == 0 exactly (all three share x)
    v = [np.array([0.5, y, z], np.float32) for y, z in ((0, 0), (1, 0), (0, 1))]
    assert PR.from_triple(*v, PR.ORTHOGONAL)[0] and not PR.from_triple(*v, PR.VERTICAL)[0]
    # through host_plane_fit: counts -1 at exactly those hypotheses
    pts = np.stack([a, b, a + 2.5 * (b - a), np.array([0, 1, 0], np.float32), np.array([1, 1, 1], np.float32)])
    o = PR.host_fit(pts, 4, PR.ORTHOGONAL, 0.01, triples=[[0, 1, 3], [0, 0, 3], [0, 1, 2], [1, 3, 4]])
    assert o['rc'] == 0 and (o['counts'] < 0).tolist() == [False, True, True, False]


def test_admissibility_at_the_bounds():
    L = PR.lib()
    pl = np.array([0.0, 0.6, 0.8, 0.25], np.float32)
    up = np.array([0, 0, 1], np.float32)
    adm = lambda cos_tilt, cams=None, tau=0.0, min_cams=0: bool(L.host_plane_admissible(              # noqa: E731
        PR._ptr(pl), PR._ptr(up), ctypes.c_float(cos_tilt), PR._ptr(cams), 0 if cams is None else len(cams), ctypes.c_float(tau), min_cams))
    assert adm(np.float32(0.8)) and not adm(np.nextafter(np.float32(0.8), np.float32(1)))           # tilt exactly at the bound passes
    # cameras at height tau exactly (residual == tau: not above), just above, below
    tau = np.float32(0.125)
    at = np.array([[0, 0, (0.25 + 0.125) / 0.8]], np.float32)
    r = np.zeros(1, np.float32)
    L.host_plane_residuals(PR._ptr(pl), PR._ptr(at), ctypes.c_int64(1), PR._ptr(r))
    at[0, 2] += (tau - r[0]) / np.float32(0.8)                                   # land on tau exactly
    L.host_plane_residuals(PR._ptr(pl), PR._ptr(at), ctypes.c_int64(1), PR._ptr(r))
    assert r[0] == tau
    above = at + np.array([[0, 0, 1e-3]], np.float32)
    assert not adm(0.0, at, tau, 1) and adm(0.0, above, tau, 1) and adm(0.0, at, tau, 0)
    both = np.ascontiguousarray(np.concatenate([at, above, above]))
    assert adm(0.0, both, tau, 2) and not adm(0.0, both, tau, 3)


def test_jacobi_against_eigh():
    """1000 seeded covariance matrices, a third of them near-planar (smallest eigenvalue 1e-12 .. 1e-4 of the middle one).

    Bound.  One Jacobi rotation changes every entry it touches by a few roundings: the computed decomposition is the exact one of C + E
    with |E| <= (8 sweeps x 3 rotations x 4 roundings) eps |C|_F = 96 eps |C|_F.  By Davis-Kahan the smallest eigenvector then turns by
    sin(angle) <= |E| / gap, gap = lambda_1 - lambda_0.  LAPACK's answer gets the same allowance: 192 eps |C|_F / gap between the two.
    The residual |C v - (v.C v) v| <= 96 eps |C|_F is held too, gap or no gap."""
    rng = np.random.RandomState(7)
    eps = 2.0 ** -52
    Cs, gaps = [], []
    for i in range(1000):
        Q, _ = np.linalg.qr(rng.randn(3, 3))
        lam = np.sort(rng.uniform(0.05, 1.0, 3)) * 10.0 ** rng.uniform(-3, 3)
        if i % 3 == 0:
            lam[0] = lam[1] * 10.0 ** rng.uniform(-12, -4)
        C = (Q * lam) @ Q.T
        C = (C + C.T) / 2
        Cs.append([C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]])
    Cs = np.ascontiguousarray(Cs)
    v = np.zeros((1000, 3))
    PR.lib().host_sym3_smallest_eigvec(PR._ptr(Cs), ctypes.c_int64(1000), PR._ptr(v))
    worst = 0.0
    for c6, vi in zip(Cs, v):
        C = np.array([[c6[0], c6[1], c6[2]], [c6[1], c6[3], c6[4]], [c6[2], c6[4], c6[5]]])
        w, V = np.linalg.eigh(C)
        fro = np.linalg.norm(C)
        assert abs(np.linalg.norm(vi) - 1) <= 4 * eps
        assert np.linalg.norm(C @ vi - (vi @ C @ vi) * vi) <= 96 * eps * fro
        sin = np.linalg.norm(np.cross(vi, V[:, 0]))
        bound = 192 * eps * fro / (w[1] - w[0])
        worst = max(worst, sin / bound)
        assert sin <= bound, (sin, bound)
    print('jacobi: worst sin(angle) / bound', worst)


def test_vertical_mode_against_the_reference_ransac():
    g = PR.golden()
    o = PR.host_fit(g['points'], 100, PR.VERTICAL, float(np.float32(g['thresh'])), triples=g['triples'])
    assert o['rc'] == 0 and np.array_equal(o['triples'], g['triples'])
    PR.check_golden(g, o['counts'], int(o['info'][0]), int(o['info'][1]))
    assert o['info'][2] == o['info'][1] and o['info'][3] == 0
    # the best model: p = (d, -n.x, -n.y) against the reference's (fp32 normal equations: held to 1e-4 of the parameters' size)
    p = np.array([o['plane'][3], -o['plane'][0], -o['plane'][1]])
    assert o['plane'][2] == 1.0 and np.abs(p - g['params']).max() <= 1e-4 * max(1.0, np.abs(g['params']).max())
    edge, _ = PR.golden_restated(g)
    assert int((o['mask'].astype(bool) != g['mask']).sum()) <= edge[int(g['best'])]


def test_orthogonal_fit_with_refinement_and_priors():
    pts, cams, up = WF.plane_cloud(4097, 3)
    tau = np.float32(0.02)
    o = PR.host_fit(pts, 64, PR.ORTHOGONAL, float(tau * tau), seed=5, up=up, cos_tilt=float(np.float32(math.cos(math.radians(60)))), cams=cams,
                    tau=float(tau), min_cams=5, refine=2)
    assert o['rc'] == 0 and o['info'][0] >= 0 and o['info'][3] == 2 and o['info'][2] >= o['info'][1]
    n = np.array([-0.2, 0.1, 1.0]) / np.linalg.norm([-0.2, 0.1, 1.0])
    assert np.degrees(np.arccos(o['plane'][:3] @ n)) < 0.2 and abs(o['plane'][3] - 0.05 * n[2]) < 2e-3
    assert int(o['mask'].sum()) == o['info'][2]
    # cameras on the wrong side: nothing is admissible, the call still succeeds
    o = PR.host_fit(pts, 64, PR.ORTHOGONAL, float(tau * tau), seed=5, up=up, cos_tilt=0.5, cams=cams - np.float32([0, 0, 5]), tau=float(tau), min_cams=5, refine=2)
    assert o['rc'] == 0 and o['info'].tolist() == [-1, 0, 0, 0] and not o['plane'].any() and not o['mask'].any() and (o['counts'] == -1).all()
