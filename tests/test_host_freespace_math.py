"""CPU: the g++ build of csrc/freespace_math.h (tests/host_freespace.cpp) against the float64 restatement of tests/freespace_ref.py, which
finds the hit from the plane equation and a Gram-matrix solve -- another route than the header's Moeller-Trumbore on triple products.

Bounds.  Where the arithmetic is exact (small integers and dyadic fractions) t, u, v are compared for equality.  On random triangles the
candidate decision must agree wherever the float64 numbers are not within 1e-5 of one of the definition's thresholds (fp32 carries
about 1e-7 of the coordinates here, and a threshold can amplify it by the ray's inclination: two decades of room).  t, u and v are held
to the element-wise bar at one bar on faces and rays whose angles are bounded away from 0 (the fixture is chosen for the bar, not the bar
for the fixture); on the unrestricted triangles t meets the bar too, and, as an extra, t, u and v stay within 32 roundings of 2^-24 in
units of their own conditioning (a needle of a face or a flat ray makes the barycentrics ill-conditioned in any arithmetic)."""
import numpy as np
import pytest

import freespace_ref as FR

# a = (0,0,0), b = (4,0,0), c = (0,4,0): every product below is a small integer or a dyadic fraction
TRI = np.array([0, 0, 0, 4, 0, 0, 0, 4, 0], np.float32)


def _one(o, p, tri=TRI):
    o, p = np.asarray(o, np.float32), np.asarray(p, np.float32)
    return FR.host_hit(tri[None], o[None], (p - o)[None])[0]


def test_exact_cases_hit_miss_behind_and_the_ends_of_the_segment():
    hit, t, u, v = _one((1, 1, 2), (1, 1, -2))                      # straight down through (1,1,0)
    assert (hit, t, u, v) == (1.0, 0.5, 0.25, 0.25)
    hit, t, u, v = _one((1, 1, -2), (1, 1, 2))                      # from behind: two-sided
    assert (hit, t, u, v) == (1.0, 0.5, 0.25, 0.25)
    c = np.array([4 / 3, 4 / 3, 0.0])                               # through the centroid
    hit, t, u, v = _one(c + [0, 0, 3], c - [0, 0, 1])
    assert hit == 1.0 and t == 0.75 and abs(u - 1 / 3) < 1e-6 and abs(v - 1 / 3) < 1e-6
    assert _one((3, 3, 2), (3, 3, -2))[0] == 0.0                     # u + v > 1: a miss
    assert _one((-1, 1, 2), (-1, 1, -2))[0] == 0.0                   # u < 0
    assert _one((1, -0.5, 2), (1, -0.5, -2))[0] == 0.0               # v < 0
    assert _one((0, 0, 2), (0, 0, -2))[0] == 1.0 and _one((4, 0, 2), (4, 0, -2))[0] == 1.0 and _one((2, 2, 2), (2, 2, -2))[0] == 1.0   # the rim counts
    # t just either side of 0 and 1: the segment is open at both ends
    assert _one((1, 1, 0), (1, 1, -4))[0] == 0.0                     # starts on the face: t = 0
    assert _one((1, 1, 4), (1, 1, 0))[0] == 0.0                      # ends on the face: t = 1
    assert _one((1, 1, 2 ** -20), (1, 1, -4))[0] == 1.0 and _one((1, 1, -(2 ** -20)), (1, 1, -4))[0] == 0.0
    assert _one((1, 1, 4), (1, 1, -(2 ** -20)))[0] == 1.0 and _one((1, 1, 4), (1, 1, 2 ** -20))[0] == 0.0
    hit, t, _, _ = _one((1, 1, 4), (1, 1, -(2 ** -20)))
    assert 0.0 < t < 1.0
    assert _one((1, 1, 2), (1, 1, 2))[0] == 0.0                      # a ray of zero length
    assert _one((1, 1, 2), (3, 1, 2))[0] == 0.0                      # parallel to the plane


def test_random_triangles_match_the_fp64_reference():
    rng = np.random.default_rng(11)
    n = 200000
    tri = rng.uniform(-2, 2, (n, 3, 3)).astype(np.float32)
    o = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    w = rng.dirichlet(np.ones(3), n)
    through = (w[:, :, None] * tri).sum(1) + rng.normal(0, 0.3, (n, 3))             # most rays aim at the face, some miss it
    p = (o + rng.uniform(0.5, 2.5, (n, 1)) * (through - o)).astype(np.float32)
    e = p - o
    out = FR.host_hit(tri, o, e).astype(np.float64)
    t64 = tri.astype(np.float64)
    r = FR.intersect(o.astype(np.float64), e.astype(np.float64), t64[:, 0], t64[:, 1], t64[:, 2])
    assert np.isfinite(out).all()
    with np.errstate(invalid='ignore'):
        w3 = np.minimum(np.minimum(r['u'], r['v']), 1 - r['u'] - r['v'])
        clear = (np.abs(w3) > 1e-5) & (np.abs(r['t']) > 1e-5) & (np.abs(r['t'] - 1) > 1e-5) & ((r['det2'] > 1.01 * r['thr']) | (r['det2'] < 0.99 * r['thr']))
    hit = out[:, 0] > 0
    print(f'random triangles: {hit.mean():.3f} hit, {clear.mean():.4f} clear of every threshold')
    assert clear.mean() > 0.99 and 0.2 < hit.mean() < 0.8
    assert np.array_equal(hit[clear], r['cand'][clear])
    both = hit & r['cand']
    k_t = FR.bars(out[both, 1], r['t'][both])
    # u, v and t in units of their conditioning: each is a quotient of triple products of |s| |e| |e_k| over det = |n| |e| sin(ray, plane),
    # |n| = |e1| |e2| sin(e1, e2), so a rounding of 2^-24 of the numerator's terms becomes |s| / (|e1| sin sin) of u.  About 16 roundings
    # lie on the way of a numerator and as many on det's: 32 of them is the bound.
    e64 = e.astype(np.float64)
    e1, e2, s = t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0], o.astype(np.float64) - t64[:, 0]
    norm = lambda x: np.linalg.norm(x, axis=1)        # noqa: E731
    nrm = np.cross(e1, e2)
    sin_tri, sin_ray = norm(nrm) / (norm(e1) * norm(e2)), np.sqrt(r['det2'] / ((nrm * nrm).sum(1) * (e64 * e64).sum(1)))
    eps = 2.0 ** -24
    k_u = (np.abs(out[:, 2] - r['u']) * sin_tri * sin_ray * norm(e1) / norm(s) / eps)[both].max()
    k_v = (np.abs(out[:, 3] - r['v']) * sin_tri * sin_ray * norm(e2) / norm(s) / eps)[both].max()
    k_c = (np.abs(out[:, 1] - r['t']) * sin_ray * norm(e64) / norm(s) / eps)[both].max()
    print(f'random triangles: t {k_t:.4f} bars; in roundings of their conditioning t {k_c:.1f}, u {k_u:.1f}, v {k_v:.1f} (bound 32); worst |t - ref| '
          f'{np.abs(out[both, 1] - r["t"][both]).max():.3e}')
    assert k_t <= 1.0 and max(k_c, k_u, k_v) <= 32.0
    assert (out[hit, 1] > 0).all() and (out[hit, 1] < 1).all() and (out[hit, 2] >= 0).all() and (out[hit, 3] >= 0).all() and (out[hit, 2] + out[hit, 3] <= 1 + 1e-6).all()


def test_t_u_and_v_meet_the_bar_on_well_conditioned_faces_and_rays():
    """t, u and v at one element-wise bar each.  The bar's floor is 1e-6 of max|b| = 1, about 16 roundings of 2^-24; a numerator of u or v
    carries about that many roundings of terms of size |s| |e| |e_k| and is divided by det = |e1| |e2| sin(e1, e2) |e| sin(ray, plane), so
    the fixture is the faces and rays whose conditioning |s| / (|e_k| sin sin) is at most 1: face angles of 60 to 120 degrees, sides of
    1 to 2, rays within 30 degrees of the normal, and of those the rays whose origin is no farther from `a` than that -- selected from the
    float64 numbers alone, the share asserted."""
    rng = np.random.default_rng(12)
    n = 200000
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)        # noqa: E731
    norm = lambda x: np.linalg.norm(x, axis=1)        # noqa: E731
    a = rng.uniform(-0.5, 0.5, (n, 3))
    d1 = unit(rng.normal(size=(n, 3)))
    nrm = unit(np.cross(d1, rng.normal(size=(n, 3))))
    ang = rng.uniform(np.pi / 3, 2 * np.pi / 3, (n, 1))
    e1 = d1 * rng.uniform(1, 2, (n, 1))
    e2 = (np.cos(ang) * d1 + np.sin(ang) * np.cross(nrm, d1)) * rng.uniform(1, 2, (n, 1))
    w = rng.dirichlet(np.ones(3), n)
    x = a + w[:, 1:2] * e1 + w[:, 2:3] * e2
    tilt = rng.uniform(0, np.pi / 6, (n, 1))
    d = (np.cos(tilt) * nrm + np.sin(tilt) * unit(np.cross(nrm, rng.normal(size=(n, 3))))) * np.where(rng.random((n, 1)) < 0.5, 1.0, -1.0)
    o32 = (x - d * rng.uniform(0.2, 1.0, (n, 1))).astype(np.float32)
    e32 = (x + d * rng.uniform(0.2, 1.0, (n, 1))).astype(np.float32) - o32
    tri = np.stack([a, a + e1, a + e2], 1).astype(np.float32)
    out = FR.host_hit(tri, o32, e32).astype(np.float64)
    t64, o64, e64 = tri.astype(np.float64), o32.astype(np.float64), e32.astype(np.float64)
    r = FR.intersect(o64, e64, t64[:, 0], t64[:, 1], t64[:, 2])
    E1, E2, S = t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0], o64 - t64[:, 0]
    N = np.cross(E1, E2)
    sin_tri, sin_ray = norm(N) / (norm(E1) * norm(E2)), np.sqrt(r['det2'] / ((N * N).sum(1) * (e64 * e64).sum(1)))
    sel = r['cand'] & (norm(S) <= norm(E1) * sin_tri * sin_ray) & (norm(S) <= norm(E2) * sin_tri * sin_ray)
    assert sin_tri.min() > 0.86 and sin_ray.min() > 0.86 and sel.mean() > 0.5 and (out[sel, 0] > 0).all()
    k = [FR.bars(out[sel, c], r[name][sel]) for c, name in ((1, 't'), (2, 'u'), (3, 'v'))]
    print(f'well-conditioned faces and rays ({sel.sum()} of {n}): t {k[0]:.4f}, u {k[1]:.4f}, v {k[2]:.4f} bars')
    assert max(k) <= 1.0


@pytest.mark.parametrize('sin2', [1e-2, 1e-3, 1e-4, 3e-5, 8e-6, 1e-6, 1e-8, 1e-10, 1e-12])
def test_the_graze_rule_on_faces_at_falling_inclinations(sin2):
    """Rays through the interior of a face whose plane they meet at sin^2 = `sin2`: candidates above FREESPACE_GRAZE = 2^-16, none below it
    (the two values next to it, 3e-5 and 8e-6, are a factor two to either side), and nothing but finite numbers at any of them."""
    rng = np.random.default_rng(21)
    n = 5000
    a, e1 = rng.uniform(-1, 1, (n, 3)), rng.normal(size=(n, 3))
    e2 = rng.normal(size=(n, 3))
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    inplane = e1 / np.linalg.norm(e1, axis=1, keepdims=True)
    d = np.sqrt(1 - sin2) * inplane + np.sqrt(sin2) * nrm
    x = a + 0.3 * e1 + 0.3 * e2
    o, p = x - 1.5 * d, x + 1.5 * d
    tri = np.stack([a, a + e1, a + e2], 1).astype(np.float32)
    o32, p32 = o.astype(np.float32), p.astype(np.float32)
    out = FR.host_hit(tri, o32, p32 - o32)
    assert np.isfinite(out).all()
    t64 = tri.astype(np.float64)
    r = FR.intersect(o32.astype(np.float64), (p32 - o32).astype(np.float64), t64[:, 0], t64[:, 1], t64[:, 2])
    share = float((out[:, 0] > 0).mean())
    print(f'graze sin^2 = {sin2:g}: {share:.3f} candidates (fp64: {r["cand"].mean():.3f}), threshold {FR.host().host_freespace_graze():g}')
    assert FR.host().host_freespace_graze() == 2.0 ** -16
    if sin2 >= 3e-5:
        assert share > 0.95 if sin2 >= 1e-4 else share > 0.5
    else:
        assert share == 0.0 if sin2 <= 1e-6 else share < 0.5
    clear = (r['det2'] > 2 * r['thr']) | (r['det2'] < 0.5 * r['thr'])
    with np.errstate(invalid='ignore'):
        inside = np.minimum(np.minimum(r['u'], r['v']), 1 - r['u'] - r['v']) > 1e-2
    sel = clear & (inside | ~(r['det2'] > r['thr']))
    assert np.array_equal(out[sel, 0] > 0, r['cand'][sel])


def test_zero_area_faces_and_repeated_vertices_are_never_candidates():
    rng = np.random.default_rng(0)
    n = 2000
    o = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    p = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    p[::2] = -o[::2]                                                # half of the rays pass through the origin, where the faces lie
    seg = np.array([-1, 0, 0, 2, 0, 0, 1, 0, 0], np.float32)        # zero area: c on ab
    rep = np.array([1, 1, 1, 1, 1, 1, 3, 1, 1], np.float32)         # a == b
    rep2 = np.array([0.3, -0.7, 0.2, 1.1, 0.4, -0.9, 1.1, 0.4, -0.9], np.float32)   # b == c, no round numbers
    pt = np.array([0.5, -1, 2] * 3, np.float32)                     # zero length: one point
    for tri in (seg, rep, rep2, pt):
        out = FR.host_hit(np.tile(tri, (n, 1)), o, p - o)
        assert np.isfinite(out).all() and not out[:, 0].any() and not out[:, 1:].any()
    # a ray that runs exactly through the degenerate face's own points
    assert _one((1, 0, 1), (1, 0, -1), seg)[0] == 0.0 and _one((1, 1, 2), (1, 1, 0), rep)[0] == 0.0 and _one((0, -1, 2), (1, -1, 2), pt)[0] == 0.0


def test_the_slab_bound_never_skips_a_face_inside_its_box():
    """10^5 segments against boxes that hold a face: wherever the host build OR the float64 reference has a candidate at t <= t_max, the slab
    test reaches the box.  Half of the faces are small (a tight box that most segments miss: the test must also cull)."""
    rng = np.random.default_rng(5)
    n = 100000
    tri = rng.uniform(-2, 2, (n, 3, 3))
    tri[: n // 2] = tri[: n // 2, :1] + 0.1 * tri[: n // 2]
    tri = tri.astype(np.float32)
    o = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    w = rng.dirichlet(np.ones(3), n)
    aim = (w[:, :, None] * tri).sum(1) + rng.normal(0, 0.02, (n, 3))
    aim[::3] = rng.uniform(-2, 2, (len(aim[::3]), 3))                # a third of the segments go anywhere
    p = (o + rng.uniform(0.7, 2.5, (n, 1)) * (aim - o)).astype(np.float32)
    e = p - o
    e[::11, 1] = 0.0                                                # some axis-parallel segments: the branch without a division
    lo, hi = tri.min(1), tri.max(1)
    out = FR.host_hit(tri, o, e)
    t64 = tri.astype(np.float64)
    r = FR.intersect(o.astype(np.float64), e.astype(np.float64), t64[:, 0], t64[:, 1], t64[:, 2])
    t_max = np.where(rng.random(n) < 0.5, 1.0, rng.uniform(0.05, 1.0, n)).astype(np.float32)
    reach = FR.host_slab(lo, hi, o, e, t_max)
    need = ((out[:, 0] > 0) & (out[:, 1] <= t_max)) | (r['cand'] & (r['t'] <= t_max))
    print(f'slab: {need.mean():.3f} of the segments hit their face below t_max, {reach.mean():.3f} reach the box')
    assert need.mean() > 0.2 and reach[need].all()
    assert reach.mean() < 0.8                                       # ... and it is a bound that culls
    # a box far off the segment, on each axis and in t
    far = FR.host_slab([[5, 5, 5]], [[6, 6, 6]], [[0, 0, 0]], [[1, 0, 0]], [1.0])
    behind = FR.host_slab([[-3, -1, -1]], [[-2, 1, 1]], [[0, 0, 0]], [[1, 0, 0]], [1.0])
    beyond = FR.host_slab([[2, -1, -1]], [[3, 1, 1]], [[0, 0, 0]], [[4, 0, 0]], [0.25])
    inside = FR.host_slab([[2, -1, -1]], [[3, 1, 1]], [[0, 0, 0]], [[4, 0, 0]], [0.6])
    assert not far[0] and not behind[0] and not beyond[0] and inside[0]


def test_keys_order_by_t_then_face_and_the_penalty_is_a_huber_shape():
    L = FR.host()
    assert L.host_freespace_key(0.25, 7) < L.host_freespace_key(0.25, 9) < L.host_freespace_key(0.5, 0)
    assert L.host_freespace_key(2.0 ** -149, 0) > 0 and L.host_freespace_key(0.999, 0xffffffff) < L.host_freespace_key(1.0, 0)
    assert L.host_freespace_psi(-1.0, 0.5) == 0.0 and L.host_freespace_psi(0.0, 0.5) == 0.0 and L.host_freespace_psi(np.float32(np.nan), 0.5) == 0.0
    assert L.host_freespace_psi(0.25, 0.5) == 0.0625 and L.host_freespace_psi(0.5, 0.5) == 0.25 and L.host_freespace_psi(2.0, 0.5) == 0.5 * 3.5
    assert L.host_freespace_g(0.75, 2.0, 0.125) == 0.375 and L.host_freespace_g(1.0, 2.0, 0.125) == -0.125
    g = np.linspace(-0.2, 1.0, 1201)
    got = np.array([L.host_freespace_psi(float(x), 0.1) for x in g])
    assert FR.bars(got, FR.psi(g.astype(np.float32).astype(np.float64), np.float64(np.float32(0.1)))) <= 1.0 and (np.diff(got) >= 0).all()
    from dbw_amd import _lib
    assert L.host_freespace_segment() == _lib.EVAL_FREESPACE_SEGMENT


def test_the_draw_is_philox_word_zero_of_stream_three():
    import surface_ref as SR
    L = FR.host()
    for seed, step, n in ((0, 0, 1), (1, 0, 1000), (0xdeadbeefcafe, 12345, 1 << 20), ((1 << 64) - 1, (1 << 40) + 3, (1 << 31) - 1), (7, 1 << 33, 999)):
        for i in (0, 1, 63, 64, 16383, (1 << 24) - 1):
            assert L.host_freespace_draw_index(seed, step, i, n) == FR.draw_index(seed, step, i, n), (seed, step, i, n)
    idx = FR.draw_indices(3, 9, 4096, 1000)
    assert idx.min() >= 0 and idx.max() < 1000 and len(np.unique(idx)) > 900
    assert not np.array_equal(idx, SR.draw_indices(3, 9, 4096, 1000))          # another stream than the surface term's
    from dbw_amd import ops
    assert np.array_equal(ops.freespace_draw(3, 9, 4096, 1000).numpy(), idx)
    assert np.array_equal(ops.freespace_draw((1 << 63) - 5, (1 << 40) + 3, 64, 77).numpy(), FR.draw_indices((1 << 63) - 5, (1 << 40) + 3, 64, 77))
