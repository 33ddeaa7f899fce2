"""CPU: the g++ build of csrc/surface_math.h (tests/host_surface.cpp) against the float64 reference of tests/surface_ref.py, which finds the
closest point by Ericson's region classification -- another algorithm than the header's plane projection with a fall-back to the sides.

Bounds.  Where the arithmetic is exact (small integers and dyadic fractions) d2, u, v are compared for equality.  On random triangles d2 and
the closest point are held to the element-wise bar of surface_ref.bars (1e-4 |b| + 1e-6 max|b|) at one bar; the worst figure is printed and
recorded in profiles/surface_term.md.  The barycentrics themselves are compared through the closest point they give: on a sliver they are
ill-conditioned while the point is not."""
import ctypes

import numpy as np
import pytest

import surface_ref as SR

# a = (0,0,0), b = (4,0,0), c = (0,4,0): every product below is a small integer or a dyadic fraction
TRI = np.array([0, 0, 0, 4, 0, 0, 0, 4, 0], np.float32)


def _one(p, tri=TRI):
    return SR.host_closest(tri[None], np.asarray(p, np.float32)[None])[0]


def test_the_seven_regions_have_their_analytic_closest_points():
    cases = [((1.0, 1.0, 3.0), (1, 1, 0)),        # interior
             ((2.0, -3.0, 1.0), (2, 0, 0)),       # edge ab
             ((4.0, 4.0, 2.0), (2, 2, 0)),        # edge bc
             ((-2.0, 1.0, -1.0), (0, 1, 0)),      # edge ca
             ((-1.0, -2.0, 1.0), (0, 0, 0)),      # vertex a
             ((7.0, -1.0, 0.0), (4, 0, 0)),       # vertex b
             ((-1.0, 9.0, 2.0), (0, 4, 0))]       # vertex c
    for p, c in cases:
        d2, u, v = _one(p)
        got = np.array([4 * u, 4 * v, 0.0])
        want = float(((np.array(p) - np.array(c)) ** 2).sum())
        assert np.array_equal(got, np.array(c, np.float64)) and d2 == want, (p, c, d2, u, v)
        r2, bary = SR.closest_on_triangles(np.array(p), TRI[0:3], TRI[3:6], TRI[6:9])
        assert r2 == want and np.allclose(bary, [1 - u - v, u, v], atol=1e-15)


def test_points_on_the_face_have_distance_zero_exactly():
    for p in [(0, 0, 0), (4, 0, 0), (0, 4, 0), (2, 0, 0), (2, 2, 0), (0, 1, 0), (1, 0.5, 0), (0.25, 3.5, 0)]:
        d2, u, v = _one(p)
        assert d2 == 0.0 and (4 * u, 4 * v) == (p[0], p[1]), (p, d2, u, v)


def test_degenerate_faces_stay_finite():
    rng = np.random.default_rng(0)
    p = rng.uniform(-2, 2, (200, 3)).astype(np.float32)
    seg = np.array([0, 0, 0, 2, 0, 0, 1, 0, 0], np.float32)       # zero area: c on ab
    rep = np.array([1, 1, 1, 1, 1, 1, 3, 1, 1], np.float32)       # a == b
    pt = np.array([0.5, -1, 2] * 3, np.float32)                   # zero length: one point
    for tri in (seg, rep, pt):
        out = SR.host_closest(np.tile(tri, (len(p), 1)), p).astype(np.float64)
        assert np.isfinite(out).all()
        t = tri.astype(np.float64).reshape(3, 3)
        ref, _ = SR.closest_on_triangles(p.astype(np.float64), t[0], t[1], t[2])
        print('degenerate: bars', SR.bars(out[:, 0], ref))
        assert SR.bars(out[:, 0], ref) <= 1.0
        c = t[0] + out[:, 1:2] * (t[1] - t[0]) + out[:, 2:3] * (t[2] - t[0])
        assert np.abs(((p - c) ** 2).sum(1) - out[:, 0]).max() < 1e-5          # d2 is the distance to the point (u, v) names
    assert np.array_equal(SR.host_closest(pt[None], pt[None, :3])[0], np.zeros(3, np.float32))


def test_random_triangles_match_the_fp64_reference():
    rng = np.random.default_rng(11)
    n = 200000
    tri = rng.uniform(-2, 2, (n, 9)).astype(np.float32)
    p = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    out = SR.host_closest(tri, p).astype(np.float64)
    t = tri.astype(np.float64).reshape(n, 3, 3)
    ref_d2, ref_b = SR.closest_on_triangles(p.astype(np.float64), t[:, 0], t[:, 1], t[:, 2])
    assert np.isfinite(out).all()
    c = t[:, 0] + out[:, 1:2] * (t[:, 1] - t[:, 0]) + out[:, 2:3] * (t[:, 2] - t[:, 0])
    ref_c = (ref_b[..., None] * t).sum(1)
    k_d2, k_c = SR.bars(out[:, 0], ref_d2), SR.bars(c, ref_c)
    print(f'random triangles: d2 {k_d2:.4f} bars, closest point {k_c:.4f} bars, worst |d2 - ref| {np.abs(out[:, 0] - ref_d2).max():.3e}')
    assert k_d2 <= 1.0 and k_c <= 1.0
    assert (out[:, 1] >= 0).all() and (out[:, 2] >= 0).all() and (out[:, 1] + out[:, 2] <= 1 + 1e-6).all()


def test_the_box_bound_never_exceeds_the_distance():
    rng = np.random.default_rng(5)
    n = 100000
    tri = rng.uniform(-2, 2, (n, 3, 3))
    tri[: n // 2] = tri[: n // 2, :1] + 0.1 * tri[: n // 2]         # half of them small faces: the box is tight, the point mostly outside
    tri = tri.astype(np.float32)
    p = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    p[::7] = tri[::7, 0]                                           # points on a vertex: distance zero
    lo, hi = tri.min(1), tri.max(1)
    bound = SR.host_box_bound(lo, hi, p)
    d2 = SR.host_closest(tri.reshape(n, 9), p)[:, 0]
    t = tri.astype(np.float64)
    ref, _ = SR.closest_on_triangles(p.astype(np.float64), t[:, 0], t[:, 1], t[:, 2])
    assert (bound >= 0).all() and (bound <= d2).all() and (bound.astype(np.float64) <= ref).all()
    assert (bound > 0).mean() > 0.3                                # ... and it is a bound that culls
    exact = (np.maximum(np.maximum(lo - p, p - hi), 0).astype(np.float64) ** 2).sum(1)
    assert np.median(bound[exact > 1e-2] / exact[exact > 1e-2]) > 0.99


def test_keys_order_by_distance_then_face_and_rho_truncates():
    L = SR.host()
    assert L.host_surface_key(0.25, 7) < L.host_surface_key(0.25, 9) < L.host_surface_key(0.5, 0)
    assert L.host_surface_key(0.0, 3) == 3 and L.host_surface_key(np.float32(np.nan), 0) > L.host_surface_key(np.float32(np.inf), 0xffffffff)
    assert L.host_surface_rho(0.5, 1.0) == 0.5 and L.host_surface_rho(1.0, 1.0) == 1.0 and L.host_surface_rho(3.0, 1.0) == 1.0
    assert L.host_surface_rho(np.float32(np.nan), 1.0) == 1.0
    from dbw_amd import _lib
    assert L.host_surface_segment() == _lib.EVAL_SURFACE_SEGMENT


def test_the_draw_is_philox_word_zero_of_stream_two():
    L = SR.host()
    # Philox4x32-10 known answers (Random123 kat_vectors) on the restatement the draw is checked against
    assert SR._philox([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert SR._philox([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert SR._philox([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    for seed, step, n in ((0, 0, 1), (1, 0, 1000), (0xdeadbeefcafe, 12345, 262144), ((1 << 64) - 1, (1 << 40) + 3, (1 << 31) - 1), (7, 1 << 33, 999)):
        for i in (0, 1, 63, 64, 16383, (1 << 24) - 1):
            assert L.host_surface_draw_index(seed, step, i, n) == SR.draw_index(seed, step, i, n), (seed, step, i, n)
    idx = SR.draw_indices(3, 9, 4096, 1000)
    assert idx.min() >= 0 and idx.max() < 1000 and len(np.unique(idx)) > 900
    assert not np.array_equal(idx, SR.draw_indices(3, 10, 4096, 1000))


@pytest.mark.parametrize('ratio', [1e-3, 1e-5, 1e-6, 1e-7, 1e-8, 1e-10, 1e-12, 1e-14])
def test_sliver_faces_keep_the_distance_and_bound_the_closest_point(ratio):
    """Faces whose sin^2 of the angle at a is about `ratio`, on both sides of SURFACE_SLIVER = 2^-24 (above it the plane branch, whose (u, v)
    cancel to a relative 2^-24 / sin; at and below it the sides, which miss an interior closest point by at most the sliver's width).  d2 is
    held to the bar of the random triangles.  The closest point is ill-conditioned ACROSS a sliver by construction, so its bound is reasoned,
    not the bar: both branches stay within 2^-12 of the lengths in play, |e1| + |e2| + |p - a|."""
    rng = np.random.default_rng(21)
    n = 20000
    a, e1 = rng.uniform(-1, 1, (n, 3)), rng.uniform(-1, 1, (n, 3))
    perp = np.cross(e1, rng.normal(size=(n, 3)))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    e2 = rng.uniform(0.2, 0.8, (n, 1)) * e1 + np.sqrt(ratio) * np.linalg.norm(e1, axis=1, keepdims=True) * perp
    tri = np.stack([a, a + e1, a + e2], 1).astype(np.float32)
    p = (a + rng.uniform(0, 1, (n, 1)) * e1 + rng.normal(0, 0.3, (n, 3))).astype(np.float32)
    near = tri[::4, 0] * 0.3 + tri[::4, 1] * 0.3 + tri[::4, 2] * 0.4                 # a quarter of the points next to the face's interior
    p[::4] = near + rng.normal(0, 1e-3, near.shape).astype(np.float32)
    out = SR.host_closest(tri.reshape(n, 9), p).astype(np.float64)
    t = tri.astype(np.float64)
    ref_d2, ref_b = SR.closest_on_triangles(p.astype(np.float64), t[:, 0], t[:, 1], t[:, 2])
    c = t[:, 0] + out[:, 1:2] * (t[:, 1] - t[:, 0]) + out[:, 2:3] * (t[:, 2] - t[:, 0])
    ref_c = (ref_b[..., None] * t).sum(1)
    lengths = np.linalg.norm(t[:, 1] - t[:, 0], axis=1) + np.linalg.norm(t[:, 2] - t[:, 0], axis=1) + np.linalg.norm(p - t[:, 0], axis=1)
    k, worst = SR.bars(out[:, 0], ref_d2), float((np.abs(c - ref_c).max(1) / lengths).max())
    print(f'slivers sin^2 ~ {ratio:g}: d2 {k:.4f} bars, closest point off by {worst:.3e} of the lengths (bound {2.0 ** -12:.3e})')
    assert np.isfinite(out).all() and k <= 1.0 and worst <= 2.0 ** -12
    assert (out[:, 1] >= 0).all() and (out[:, 2] >= 0).all() and (out[:, 1] + out[:, 2] <= 1 + 1e-6).all()
