"""CPU tests of the arithmetic of the depth cloud: csrc/depth_math.h built for the host with g++ (tests/host_depth_math.cpp, through
tests/depth_ref.py) against an fp64 numpy restatement of the formulas of DESIGN.md 6r written here, and the range and edge rules, which
are integer arithmetic, exactly on hand-made maps.

Bounds, all derived (eps = 2^-23, a rounding moves a value by at most eps of it):
  * source coordinates: delta_uv = 65 * eps * max(H, W, 2) px -- the 64 roundings tests/test_host_rectify_math.py holds the map of
    lens_rect_source to, and one for u + 0.5;
  * a world coordinate p_a = ((A0*cx + A1*cy) + A2*z) + t: x takes 3 roundings (j + 0.5, - cx0, * inv_fx0; the first is exact for the
    small integers here and is counted all the same), cx = x*z one more and A0*cx a fifth: 5 roundings of |A0 cx|; the same 5 for
    |A1 cy|; z = (float)d is exact, so A2*z has 1; the two sums and + t have 1 each: 5 + 5 + 1 + 1 + 1 + 1 = 14 roundings, every one of a
    value of at most Mx, the largest magnitude among the terms, the partial sums and p over the fixture: |dp| <= 14 * eps * Mx;
  * the quantised coordinate f = (p - lo) * inv_step: the difference and the product are one rounding each of a value whose image in
    steps is at most |f|: delta_q = eps * (14 * Mx * inv_step + 2 * max|f|) steps.  inv_step is the same fp32 number on both sides.
A sample whose fp64 u + 0.5 or v + 0.5 lies within delta_uv of an integer (the header may pick the neighbouring source pixel), or whose
fp64 f lies within delta_q of an integer on some axis (the header may floor to the neighbouring step), is set aside and counted; every
other sample must agree EXACTLY: dropped or not, inside the box or not, q on the three axes, the cell.  The fixtures keep the share set
aside under 1 %: the scene of tests/depth_ref.py shrunk by 0.4 (Mx about 1.6) in the cube [-2, 2]^3 at G = 1, so that Mx * inv_step is
about 420 steps and delta_q about 1e-3 of a step, on three axes and both sides of an integer (a step is 2^-10 of the cube's side at
G = 1; a finer grid has finer steps and sets more aside).  For G = 2, 8, 64 the cells are compared instead, in the cube [-1, 1]^3, with the
samples within delta_q of a CELL boundary (a multiple of 1024 steps) set aside: a handful."""
import numpy as np
import pytest

import depth_ref as DR
import rectify_ref as RF

EPS = 2.0 ** -23
SCALE = 0.4
FIXTURES = [(9, 24, 32), (5, 37, 67), (17, 5, 7)]           # (enough samples at stride 3 for a share of 1 % to mean more than two of them)


def source64(cam, tgt, i, j):
    """(x, y, u, v) in fp64 of target pixels (i, j) for one fp32 camera row and the fp32 target."""
    model, fx, fy, cx, cy, k1, k2, k3, k4, p1, p2 = [float(v) for v in cam[:11]]
    cx0, cy0, ifx, ify = [float(v) for v in tgt]
    x, y = (j + 0.5 - cx0) * ifx, (i + 0.5 - cy0) * ify
    r2 = x * x + y * y
    if model == RF.FISHEYE:
        r = np.sqrt(r2)
        safe = np.where(r == 0, 1.0, r)
        th = np.arctan(safe)
        t2 = th * th
        s = np.where(r == 0, 1.0, th * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) / safe)
        return x, y, x * s * fx + cx - 0.5, y * s * fy + cy - 0.5
    d = 1 + r2 * (k1 + r2 * (k2 + r2 * (k3 + r2 * k4)))
    xd, yd = x * d + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * d + 2 * p2 * x * y + p1 * (r2 + 2 * y * y)
    return x, y, xd * fx + cx - 0.5, yd * fy + cy - 0.5


def jump(d, nb, permille):
    return nb == 0 or 1000 * abs(d - nb) > permille * d


def restate64(depth, cams, tgt, poses, bx, G, d_min=1, d_max=65535, stride=1, permille=0):
    """The formulas in fp64, pixel by pixel: status (N,Hs,Ws) (the cell, -1 dropped, -2 outside the box), f (N,Hs,Ws,3) fp64 steps (nan where
    dropped), us, vs (N,Hs,Ws): u + 0.5, v + 0.5, and Mx."""
    N, H, W = depth.shape
    ii, jj = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing='ij')
    status = np.full((N,) + ii.shape, -1, np.int64)
    f = np.full((N,) + ii.shape + (3,), np.nan)
    us, vs = np.zeros((N,) + ii.shape), np.zeros((N,) + ii.shape)
    lo, inv = bx[:3].astype(np.float64), float(bx[3])
    Mx = 0.0
    for n in range(N):
        x, y, u, v = source64(cams[n], tgt, ii.astype(np.float64), jj.astype(np.float64))
        us[n], vs[n] = u + 0.5, v + 0.5
        A, t = poses[n, :9].astype(np.float64).reshape(3, 3), poses[n, 9:].astype(np.float64)
        for a in range(ii.shape[0]):
            for b in range(ii.shape[1]):
                sx, sy = np.floor(us[n, a, b]), np.floor(vs[n, a, b])
                if not (0 <= sx <= W - 1 and 0 <= sy <= H - 1):
                    continue
                sx, sy = int(sx), int(sy)
                d = int(depth[n, sy, sx])
                if d < d_min or d > d_max:
                    continue
                if permille > 0 and any(jump(d, int(depth[n, yy, xx]), permille) for yy, xx in ((sy, sx - 1), (sy, sx + 1), (sy - 1, sx), (sy + 1, sx))
                                        if 0 <= yy < H and 0 <= xx < W):
                    continue
                c = np.array([x[a, b] * d, y[a, b] * d, float(d)])
                terms = A * c[None]
                p = terms.sum(1) + t
                Mx = max(Mx, float(np.abs(terms).max()), float(np.abs(terms[:, :2].sum(1)).max()), float(np.abs(terms.sum(1)).max()), float(np.abs(p).max()))
                f[n, a, b] = (p - lo) * inv
                q = np.floor(f[n, a, b])
                if not ((q >= 0) & (q < G * 1024)).all():
                    status[n, a, b] = -2
                    continue
                q = q.astype(np.int64) >> 10
                status[n, a, b] = (q[0] * G + q[1]) * G + q[2]
    return status, f, us, vs, Mx


def near_integer(a, delta, period=1.0):
    a = a / period
    return np.abs(a - np.round(a)) * period <= delta


def _deltas(H, W, f, Mx, inv):
    return 65 * EPS * max(H, W, 2), EPS * (14 * Mx * inv + 2 * float(np.nanmax(np.abs(f), initial=0.0)))


@pytest.mark.parametrize('kind', DR.KINDS)
@pytest.mark.parametrize('N,H,W', FIXTURES)
def test_the_header_against_the_fp64_restatement_step_for_step(N, H, W, kind):
    G = 1
    depth, cams, tgt, poses = DR.case(N, H, W, kind, scale=SCALE)
    bx = DR.box(-2.0, 2.0, G)
    for stride, permille in ((1, 0), (3, 50)):
        status, f, us, vs, Mx = restate64(depth, cams, tgt, poses, bx, G, 1, 65535, stride, permille)
        cell, q = DR.samples_host(depth, cams, tgt, poses, bx, G, 1, 65535, stride, permille)
        duv, dq = _deltas(H, W, f, Mx, float(bx[3]))
        aside = near_integer(us, duv) | near_integer(vs, duv) | (near_integer(f, dq) & np.isfinite(f)).any(-1)
        share = aside.mean()
        print(f'{N}x{H}x{W} {kind} stride {stride} edge {permille}: Mx {Mx:.3f}, delta_uv {duv:.3g} px, delta_q {dq:.3g} steps, {int(aside.sum())} of '
              f'{aside.size} samples set aside ({100 * share:.3f} %), {int((status >= 0).sum())} in the box, {int((status == -2).sum())} outside')
        assert share < 0.01
        keep = ~aside
        assert np.array_equal(cell[keep], status[keep])
        inside = keep & (status >= 0)
        assert np.array_equal(q[inside], np.floor(f[inside]).astype(np.int64))
        assert not q[cell < 0].any()
        # counts per cell over the samples not set aside
        assert np.array_equal(np.bincount(cell[inside], minlength=G ** 3), np.bincount(status[inside], minlength=G ** 3))
    assert (status >= 0).sum() > 0.5 * status.size or H * W < 40


@pytest.mark.parametrize('G', (2, 8, 64))
@pytest.mark.parametrize('kind', DR.KINDS)
def test_the_cells_of_finer_grids(G, kind):
    N, H, W = 5, 24, 32
    depth, cams, tgt, poses = DR.case(N, H, W, kind, seed=G, scale=SCALE)
    bx = DR.box(-1.0, 1.0, G)
    status, f, us, vs, Mx = restate64(depth, cams, tgt, poses, bx, G, 1, 65535, 1, 50)
    cell, _ = DR.samples_host(depth, cams, tgt, poses, bx, G, 1, 65535, 1, 50)
    duv, dq = _deltas(H, W, f, Mx, float(bx[3]))
    aside = near_integer(us, duv) | near_integer(vs, duv) | (near_integer(f, dq, 1024.0) & np.isfinite(f)).any(-1)
    print(f'G {G} {kind}: delta_q {dq:.3g} steps, {int(aside.sum())} of {aside.size} set aside, {len(np.unique(status[status >= 0]))} cells')
    assert aside.mean() < 0.01
    assert np.array_equal(cell[~aside], status[~aside])
    assert len(np.unique(status[status >= 0])) > (1 if G == 2 else G)


def _identity_camera(H, W):
    """A pinhole whose lens map is the identity, exactly: focal length 4 (a power of two, so is its reciprocal), the principal point on
    the pixel grid: u = j, v = i.  Poses: 2^-10 of a step each way, everything inside a box of [-64, 64]."""
    cams = RF.table([(4.0, 4.0, W / 2, H / 2)], [(0.0,) * 6], [RF.RADTAN])
    tgt = RF.target((4.0, 4.0, W / 2, H / 2))
    poses = np.float32([[2.0 ** -10, 0, 0, 0, 2.0 ** -10, 0, 0, 0, 2.0 ** -10, 0, 0, 0]])
    return cams, tgt, poses, DR.box(-64.0, 64.0, 1)


def test_the_range_rule_is_exact():
    d_min, d_max = 100, 2000
    m = np.uint16([[[d_min - 1, d_min, d_min + 1], [d_max - 1, d_max, d_max + 1], [0, 1, 65535]]])
    cams, tgt, poses, bx = _identity_camera(3, 3)
    cell, q = DR.samples_host(m, cams, tgt, poses, bx, 1, d_min, d_max)
    assert (cell[0] >= 0).tolist() == [[False, True, True], [True, True, False], [False, False, False]]
    assert (cell[0][cell[0] < 0] == -1).all()
    cell, _ = DR.samples_host(m, cams, tgt, poses, bx, 1, 1, 65535)
    assert (cell[0] >= 0).tolist() == [[True, True, True], [True, True, True], [False, True, True]]              # 0 is never a measurement
    # pixel (1, 1) is the principal point, x = y = 0, and z = (float)d exactly: the third axis is d * 2^-10 + 64 in steps of 1/8
    assert q[0, 1, 1, 2] == int(np.floor((2000 * 2.0 ** -10 + 64) * 8))


def test_the_edge_rule_is_exact():
    """permille = 50 around d = 1000: a neighbour of 1050 is exactly at the threshold (1000 * 50 > 50 * 1000 is false: kept), 1051 is one
    above (dropped); the rule is relative to the pixel's OWN depth, so 1050 and 1051 keep their neighbour of 1000 (50000 and 51000 against
    52500 and 52550).  A 0 neighbour drops its four neighbours at any threshold, 1000 included; a neighbour outside the frame is none."""
    m = np.full((1, 5, 7), 1000, np.uint16)
    m[0, 1, 1], m[0, 1, 5], m[0, 3, 3] = 1050, 1051, 0
    cams, tgt, poses, bx = _identity_camera(5, 7)
    want = np.ones((5, 7), bool)
    want[3, 3] = False                                                          # no measurement
    for y, x in ((2, 3), (4, 3), (3, 2), (3, 4)):                               # next to the hole
        want[y, x] = False
    for y, x in ((0, 5), (2, 5), (1, 4), (1, 6)):                               # next to the jump of 51
        want[y, x] = False
    cell, _ = DR.samples_host(m, cams, tgt, poses, bx, 1, 1, 65535, 1, 50)
    assert (cell[0] >= 0).tolist() == want.tolist()
    assert cell[0, 1, 1] >= 0 and cell[0, 1, 5] >= 0 and cell[0, 0, 1] >= 0 and cell[0, 1, 0] >= 0
    # the restatement above states the same rule
    status = restate64(m, cams, tgt, poses, bx, 1, 1, 65535, 1, 50)[0]
    assert np.array_equal(status >= 0, cell >= 0)
    # edge off: only the hole is dropped; threshold 1000: only a 0 neighbour is a jump
    assert int((DR.samples_host(m, cams, tgt, poses, bx, 1)[0] < 0).sum()) == 1
    assert int((DR.samples_host(m, cams, tgt, poses, bx, 1, 1, 65535, 1, 1000)[0] < 0).sum()) == 5
    # a 3x3 map, every pixel on the border: the corners have two neighbours, none outside the frame is read
    m3 = np.uint16([[[1000, 1049, 1000], [1000, 1000, 1000], [953, 1000, 0]]])
    cams, tgt, poses, bx = _identity_camera(3, 3)
    cell, _ = DR.samples_host(m3, cams, tgt, poses, bx, 1, 1, 65535, 1, 50)
    # 1049 keeps 1000s around it (49000 < 50000); 953 next to 1000: 47000 < 47650 kept, and 1000 next to 953 kept; next to 0: dropped
    assert (cell[0] >= 0).tolist() == [[True, True, True], [True, True, False], [True, False, False]]


def test_nothing_that_is_not_finite_reaches_the_cast():
    depth, cams, tgt, poses = DR.case(1, 5, 7, 'fisheye')
    poses = poses.copy()
    poses[0, 9] = np.float32(3e38)
    bx = DR.box(-2.0, 2.0, 2)
    cell, q = DR.samples_host(depth, cams, tgt, poses, bx, 2)
    assert (cell < 0).all() and (cell == -2).any() and not q.any()
    poses[0, 0], poses[0, 9] = np.float32(3e38), 0.0                            # inf - inf along the way: a NaN drops
    cell, q = DR.samples_host(np.full_like(depth, 65535), cams, tgt, poses, bx, 2)
    assert (cell < 0).all() and not q.any()


def test_the_point_of_a_cell():
    """lo + ((sum + 0.5 count) / count) / inv_step through the accumulation: one sample gives the middle of its step."""
    m = np.uint16([[[1000]]])
    cams, tgt, poses, bx = _identity_camera(1, 1)
    pts, counts, info = DR.cloud_host(m, cams, tgt, poses, bx, 1)
    cell, q = DR.samples_host(m, cams, tgt, poses, bx, 1)
    assert info.tolist() == [1, 1, 0] and counts.tolist() == [1]
    want = np.float64(bx[:3]) + (q[0, 0, 0] + 0.5) / np.float64(bx[3])
    assert np.array_equal(pts[0], want.astype(np.float32))
