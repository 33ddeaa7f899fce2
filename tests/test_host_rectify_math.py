"""CPU tests of the arithmetic of the per-frame rectification: the per-frame part of csrc/lens_math.h built for the host with g++
(tests/host_rectify_math.cpp, through tests/rectify_ref.py) against an fp64 numpy restatement of the two maps written here, and
dataset.common_pinhole / dataset.rectify_zoom / ops.lens_table / ops.lens_target.

Bounds, all derived, and those of tests/test_host_lens_math.py:
  * coordinates: delta = 64 * 2^-23 * max(H, W) px -- 64 roundings of the largest coordinate.  The fisheye chain is about 45 fp32
    operations, two divisions and a square root among them, all rounded correctly, and an arctangent within 8 * 2^-24 of its value;
  * bytes: 0.5 + 510 * delta around the unrounded fp64 bilinear value, for every byte;
  * direction of the map: 1 + (60 + 50) * (2 pi m / 16)^2 / 8 levels, see test_the_fisheye_map_runs_from_the_pinhole_frame_into_the_distorted_one;
  * the arctangent alone: see test_the_arctangent_of_the_header."""
import numpy as np
import pytest

import lens_ref as LR
import rectify_ref as RF
from dbw_amd import dataset as DS
from dbw_amd import ops

MODELS = (RF.RADTAN, RF.FISHEYE)
CASES = [(H, W, model, k) for (H, W) in RF.SHAPES for model in MODELS for k in range(3)]


def theta_d64(th, k):
    t2 = th * th
    return th * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))


def source64(H, W, intr, dist, model, tgt, zoom, i=None, j=None):
    """The fp64 restatement: source index coordinates (u, v) in the frame of the camera (intr, dist, model) of the pixels (i, j) (the whole
    frame by default; fractional allowed) of the pinhole tgt = (fx0, fy0, cx0, cy0) zoomed by `zoom`."""
    fx, fy, cx, cy = intr
    fx0, fy0, cx0, cy0 = tgt
    if i is None:
        i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    x, y = (j + 0.5 - cx0) / (zoom * fx0), (i + 0.5 - cy0) / (zoom * fy0)
    if model == RF.FISHEYE:
        r = np.hypot(x, y)
        safe = np.where(r == 0, 1.0, r)
        s = np.where(r == 0, 1.0, theta_d64(np.arctan(safe), dist) / safe)
        xd, yd = x * s, y * s
    else:
        k1, k2, k3, k4, p1, p2 = dist
        r2 = x * x + y * y
        d = 1 + r2 * (k1 + r2 * (k2 + r2 * (k3 + r2 * k4)))
        xd, yd = x * d + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * d + 2 * p2 * x * y + p1 * (r2 + 2 * y * y)
    return xd * fx + cx - 0.5, yd * fy + cy - 0.5


def bilinear64(frame, u, v):
    """The sampling rule in fp64, unrounded: frame (H,W,3), u, v (H,W) -> (H,W,3) float64."""
    H, W, _ = frame.shape
    u, v = np.clip(u, 0, W - 1), np.clip(v, 0, H - 1)
    x0, y0 = np.minimum(u.astype(np.int64), W - 2), np.minimum(v.astype(np.int64), H - 2)
    wx, wy = (u - x0)[..., None], (v - y0)[..., None]
    f = frame.astype(np.float64)
    a = f[y0, x0] + (f[y0, x0 + 1] - f[y0, x0]) * wx
    b = f[y0 + 1, x0] + (f[y0 + 1, x0 + 1] - f[y0 + 1, x0]) * wx
    return a + (b - a) * wy


def _scene(H, W, model, k):
    """The four cameras with one coefficient set, their median target and the zoom of the crop."""
    cams, dist = RF.cameras(H, W), RF.coeff_sets(model)[k]
    intrs = [cams[c] for c in RF.CAMERA_NAMES]
    tgt = RF.median_target(H, W)
    return intrs, dist, tgt, DS.rectify_zoom(H, W, intrs, [dist] * 4, [model] * 4, tgt)


def test_the_arctangent_of_the_header():
    """Relative error against numpy's fp64 arctan, bound 8 eps with eps = 2^-24 (a rounding moves a value by at most eps of it).  The
    worst branch is the middle one, a = (t - 1) / (t + 1) with |a| <= tan(pi/8) = 0.414 and a result of at least pi/8 = 0.393: three
    roundings in a (3 eps |a| = 1.25 eps, passed on with a slope of at most 1), five in the correction term q z a of at most 0.057 |a|
    (0.12 eps), the polynomial's own truncation (below 0.14 eps, measured here in fp64), the sum with a (0.39 eps), the constant pi/4 in
    fp32 (0.79 eps) and the last sum (eps of the result): 2.7 eps / 0.393 + eps < 8 eps.  The other branches have one rounding or none in
    a and stay below half of that."""
    a = np.linspace(-0.4142136, 0.4142136, 200001)
    z = a * a
    q = ((8.05374449538e-2 * z - 1.38776856032e-1) * z + 1.99777106478e-1) * z - 3.33329491539e-1
    assert np.abs(q * z * a + a - np.arctan(a)).max() < 0.14 * 2.0 ** -24
    t = np.concatenate([np.linspace(0, 4, 200001), np.float32([0.0, 1e-30, 1e-6, 0.41421354, 0.41421357, 2.4142134, 2.4142137, 1.0, 50.0, 1e6, 1e30])])
    t = t.astype(np.float32)
    got, want = RF.atan_host(t).astype(np.float64), np.arctan(t.astype(np.float64))
    worst = float((np.abs(got - want) / np.maximum(want, 1e-300)).max() / 2.0 ** -24)
    print(f'lens_atan: {worst:.3f} eps of relative error at the worst of {t.size} arguments (bound 8)')
    assert worst <= 8.0
    assert RF.atan_host(np.float32([0.0]))[0] == 0.0 and np.isnan(RF.atan_host(np.float32([np.nan]))[0])


@pytest.mark.parametrize('H,W,model,k', CASES)
def test_the_header_against_the_fp64_restatement(H, W, model, k):
    intrs, dist, tgt, zoom = _scene(H, W, model, k)
    delta = 64 * 2.0 ** -23 * max(H, W)
    rows = RF.table(intrs, [dist] * 4, [model] * 4)
    src = LR.frames(4, H, W, seed=k)
    for z in (zoom, 1.0):
        t32 = RF.target(tgt, z)
        got = RF.rectify_host(src, rows, t32)
        for n, name in enumerate(RF.CAMERA_NAMES):
            u64, v64 = source64(H, W, intrs[n], dist, model, tgt, z)
            u32, v32 = RF.source_host(H, W, rows[n], t32)
            eu, ev = float(np.abs(u32 - u64).max()), float(np.abs(v32 - v64).max())
            eb = float(np.abs(got[n].astype(np.float64) - bilinear64(src[n], u64, v64)).max())
            print(f'{H}x{W} model {model} set {k} camera {name} zoom {z:.4f}: |du| {eu:.3g}, |dv| {ev:.3g} px = {max(eu, ev) / (2.0 ** -23 * max(H, W)):.2f} '
                  f'roundings (bound 64); bytes {eb:.6f} levels (bound {0.5 + 510 * delta:.6f})')
            assert eu <= delta and ev <= delta
            assert eb <= 0.5 + 510 * delta
        # the dataset's fp64 map is this restatement
        i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
        ud, vd = DS.lens_source(H, W, intrs[2], dist, z, i, j, model=model, target=tgt)
        u64, v64 = source64(H, W, intrs[2], dist, model, tgt, z)
        assert np.abs(ud - u64).max() < 1e-9 and np.abs(vd - v64).max() < 1e-9
    # the binding's arrays are the checker's
    assert np.array_equal(ops.lens_table(intrs, [dist] * 4, [model] * 4).numpy(), rows)
    assert np.array_equal(ops.lens_target(tgt, zoom).numpy(), RF.target(tgt, zoom))


def test_the_cases_mask_something_and_crop_without_a_refusal():
    """What the shared cases are chosen for, in fp64, for the fisheye sets: the crop needs a zoom (between 1.13 and 1.16 at 24x32) and is
    never refused; at zoom 1 camera C cannot fill 11-14 % of the target, so lens='mask' has something to mask, and B, D fill all of it;
    theta_d is monotone over the field of view.  A fills all of it at 24x32.  At 23x37 the target's cy0 = 11.5 lies 0.46 px below A's
    11.04, which leaves v < 0 on part of the top row under the first two sets (15 and 9 of 851 pixels), and the zoom of the second set is
    1.126: there A is held to 98 % and the zoom to (1.12, 1.16)."""
    for H, W in RF.SHAPES:
        for k in range(3):
            intrs, dist, tgt, zoom = _scene(H, W, RF.FISHEYE, k)
            share = {}
            for n, name in enumerate(RF.CAMERA_NAMES):
                u, v = source64(H, W, intrs[n], dist, RF.FISHEYE, tgt, 1.0)
                share[name] = float(((u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)).mean())
            print(f'{H}x{W} fisheye set {k}: zoom {zoom:.4f}, valid at zoom 1 {share}')
            assert 0.86 <= share['C'] <= 0.89 and share['B'] == share['D'] == 1.0
            if (H, W) == (24, 32):
                assert 1.13 <= zoom <= 1.16 and share['A'] == 1.0
            else:
                assert 1.12 <= zoom <= 1.16 and share['A'] >= 0.98
            fx0, fy0, cx0, cy0 = tgt
            th = np.linspace(0, np.arctan(np.hypot(max(cx0, W - cx0) / fx0, max(cy0, H - cy0) / fy0)), 2001)
            assert (np.diff(theta_d64(th, dist)) > 0).all()


@pytest.mark.parametrize('H,W', RF.SHAPES)
@pytest.mark.parametrize('k', range(len(LR.COEFFS)))
def test_equal_radial_tangential_cameras_are_the_shared_map_byte_for_byte(H, W, k):
    intr, dist = LR.intrinsics(H, W), LR.COEFFS[k]
    zoom = DS.lens_zoom(H, W, intr, dist)
    assert DS.rectify_zoom(H, W, [intr] * 4, [dist] * 4, [0] * 4, intr) == zoom
    src = LR.frames(4, H, W, seed=k)
    rows, t32 = RF.table([intr] * 4, [dist] * 4, [RF.RADTAN] * 4), RF.target(intr, zoom)
    assert np.array_equal(RF.rectify_host(src, rows, t32), LR.undistort_host(src, intr, dist, zoom))
    u, v = RF.source_host(H, W, rows[0], t32)
    u0, v0 = LR.source_host(H, W, LR.lens_array(intr, dist, zoom))
    assert np.array_equal(u.view(np.int32), u0.view(np.int32)) and np.array_equal(v.view(np.int32), v0.view(np.int32))


@pytest.mark.parametrize('H,W', RF.SHAPES)
@pytest.mark.parametrize('model', MODELS)
def test_the_pixel_on_the_principal_point_is_the_source_byte_there(H, W, model):
    """Camera D rectified into itself: the output pixel whose centre is the principal point has r2 == 0 and reads the source pixel of the
    same index with both weights 0, whatever the coefficients."""
    D = RF.cameras(H, W)['D']
    i0, j0 = 11, W // 2
    src = LR.frames(2, H, W, seed=3)
    for dist in RF.coeff_sets(model):
        rows, t32 = RF.table([D] * 2, [dist] * 2, [model] * 2), RF.target(D, 1.0)
        u, v = RF.source_host(H, W, rows[0], t32)
        assert u[i0, j0] == j0 and v[i0, j0] == i0
        assert np.array_equal(RF.rectify_host(src, rows, t32)[:, i0, j0], src[:, i0, j0])


def _invert_theta_d(td, k, rounds=60):
    """theta of theta_d by Newton's iteration in fp64."""
    th = td.copy()
    for _ in range(rounds):
        t2 = th * th
        f = theta_d64(th, k) - td
        df = 1 + t2 * (3 * k[0] + t2 * (5 * k[1] + t2 * (7 * k[2] + t2 * 9 * k[3])))
        th = th - f / df
    return th


def _pattern(x_px, y_px):
    return 127.5 + 60 * np.sin(2 * np.pi * x_px / 16) + 50 * np.cos(2 * np.pi * y_px / 16 + 0.3)


def _direction_error(H, W, intr, dist, zoom, header_dist):
    """Largest |rectified byte - pattern| over the frame, the bound and the magnification.  The fisheye frame is painted with `dist`,
    rectified by the header with `header_dist` into the camera's own pinhole zoomed by `zoom`."""
    fx, fy, cx, cy = intr
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    xd, yd = (xs + 0.5 - cx) / fx, (ys + 0.5 - cy) / fy
    td = np.hypot(xd, yd)
    th = _invert_theta_d(td, dist)
    assert np.abs(theta_d64(th, dist) - td).max() < 1e-13 and (th >= 0).all() and th.max() < np.pi / 2       # the inversion's residual
    s = np.where(td == 0, 1.0, np.tan(th) / np.where(td == 0, 1.0, td))
    x, y = xd * s, yd * s
    painted = np.clip(np.floor(_pattern(x * zoom * fx + cx, y * zoom * fy + cy) + 0.5), 0, 255).astype(np.uint8)
    src = np.repeat(painted[None, :, :, None], 3, 3)
    got = RF.rectify_host(src, RF.table([intr], [header_dist], [RF.FISHEYE]), RF.target(intr, zoom))[0, :, :, 0].astype(np.float64)
    want = _pattern(xs + 0.5, ys + 0.5)
    e = 0.5
    jac = np.stack([(np.stack(source64(H, W, intr, dist, RF.FISHEYE, intr, zoom, ys + di, xs + dj))
                     - np.stack(source64(H, W, intr, dist, RF.FISHEYE, intr, zoom, ys - di, xs - dj))) / (2 * e) for di, dj in ((0, e), (e, 0))], -1)
    # m: output pixels per source pixel at the worst, that is 1 / the smallest singular value of the Jacobian of the map (which runs from
    # the output into the source and COMPRESSES towards the border of a fisheye frame: the painted pattern is densest there)
    sv = np.linalg.svd(np.moveaxis(jac, 0, 2), compute_uv=False)
    m = float(1.0 / sv.min())
    return float(np.abs(got - want).max()), 1 + (60 + 50) * (2 * np.pi * m / 16) ** 2 / 8, m, float(sv.max())


@pytest.mark.parametrize('H,W', RF.SHAPES)
@pytest.mark.parametrize('k', range(3))
def test_the_fisheye_map_runs_from_the_pinhole_frame_into_the_distorted_one(H, W, k):
    """The direction test of tests/test_host_lens_math.py restated for the fisheye model on camera A: a fisheye frame of an analytic
    pattern, painted by inverting theta_d(theta) in fp64 per source pixel (Newton, the residual asserted), must come out of the
    rectification as the pattern at the output's pinhole coordinates.  Bound: half a level for each of the two roundings to a byte, plus
    the error of a bilinear cell on a function of amplitude 60 + 50 whose phase advances by at most 2 pi m / 16 per SOURCE pixel.  The
    pattern is defined on the output, so m is the number of output pixels a step of one source pixel covers at the worst: the reciprocal
    of the SMALLEST singular value of the Jacobian of the fp64 map (output -> source), measured by central differences.  A fisheye map
    compresses towards the border (d theta / d r = 1 / (1 + r^2)), so here m is 1.3 to 1.5 where the largest singular value is 1.0: with
    the largest singular value in m's place the formula's own derivation does not hold and these frames miss it by up to 6 % at 23x37
    (3.31 levels against 3.12).  Handing the header -k1 must exceed twice the bound; the all-zero set (k1 = 0: nothing to negate) is out
    of that second property."""
    intr, dist = RF.cameras(H, W)['A'], RF.coeff_sets(RF.FISHEYE)[k]
    zoom = DS.rectify_zoom(H, W, [intr], [dist], [RF.FISHEYE], intr)
    err, bound, m, sv_max = _direction_error(H, W, intr, dist, zoom, dist)
    print(f'{H}x{W} fisheye set {k}: zoom {zoom:.4f}, m {m:.4f} (largest singular value {sv_max:.4f}): error {err:.3f} levels (bound {bound:.3f})')
    assert err <= bound
    if dist[0] != 0:
        flipped = _direction_error(H, W, intr, dist, zoom, (-dist[0],) + dist[1:])[0]
        print(f'  with k1 negated {flipped:.2f} levels (must exceed {2 * bound:.3f})')
        assert flipped > 2 * bound


@pytest.mark.parametrize('H,W', RF.SHAPES)
def test_common_pinhole_and_rectify_zoom(H, W):
    cams = RF.cameras(H, W)
    for c in cams.values():
        assert DS.common_pinhole([c] * 3) == c and DS.common_pinhole([c]) == c
    assert DS.common_pinhole(list(cams.values())) == RF.median_target(H, W)
    i = np.concatenate([np.zeros(W), np.full(W, H - 1.0), np.arange(H), np.arange(H)])
    j = np.concatenate([np.arange(W), np.arange(W), np.zeros(H), np.full(H, W - 1.0)])

    def inside(intrs, dist, model, tgt, s):
        for intr in intrs:
            u, v = source64(H, W, intr, dist, model, tgt, s, i, j)
            if not bool(np.all((u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1))):
                return False
        return True

    for model in MODELS:
        for k in range(3):
            intrs, dist, tgt, s = _scene(H, W, model, k)
            assert 1 < s < 2 and inside(intrs, dist, model, tgt, s) and not inside(intrs, dist, model, tgt, s * (1 - 1e-3)), (model, k, s)
    # camera B alone, into itself: a fisheye frame of these sets covers more than its pinhole
    for dist in RF.coeff_sets(RF.FISHEYE):
        assert DS.rectify_zoom(H, W, [cams['B']], [dist], [RF.FISHEYE], cams['B']) == 1.0
    # a narrow source under a wide target: a zoom of 2 does not suffice, and the message names the way out
    with pytest.raises(ValueError, match="zoom of 2.*lens='mask'"):
        DS.rectify_zoom(H, W, [(3.0 * W, 3.0 * W, 0.5 * W, 0.5 * H)], [(0.0,) * 6], [RF.RADTAN], cams['B'])
    with pytest.raises(ValueError):
        DS.lens_source(H, W, cams['A'], (0.0,) * 6, 1.0, i, j, model=2)


def test_lens_table_and_lens_target_refuse_what_the_library_would():
    A = RF.cameras(24, 32)['A']
    assert ops.lens_table([], [], []).shape == (0, 16) and ops.lens_table([A], [(0.0,) * 6], [1]).dtype.is_floating_point
    with pytest.raises(ValueError):
        ops.lens_table([A], [(0.0,) * 6], [2])
    with pytest.raises(ValueError):
        ops.lens_table([A, A], [(0.0,) * 6], [0, 0])
    with pytest.raises(ValueError):
        ops.lens_table([(0.0,) + A[1:]], [(0.0,) * 6], [0])
    with pytest.raises(ValueError):
        ops.lens_target(A[:3])
    with pytest.raises(ValueError):
        ops.lens_target(A, 0.0)


def test_the_entry_points_validate_before_any_launch():
    """The device pointers are non-null and never dereferenced: each call must fail validation, on the host (no GPU here)."""
    import ctypes
    from dbw_amd import _lib
    lib = _lib.load()
    good, tgt = RF.five_frames(24, 32, RF.FISHEYE, RF.coeff_sets(RF.FISHEYE)[0])
    base, n = 1 << 20, 5 * 24 * 32 * 3

    def rc(rows=good, target=tgt, src=base, out=1 << 24, N=5, H=24, W=32):
        rows, target = np.ascontiguousarray(rows, np.float32), np.ascontiguousarray(target, np.float32)
        return lib.dbw_lens_rectify_u8(src, N, H, W, rows.ctypes.data, target.ctypes.data, out, None)

    def rc_valid(rows=good, target=tgt, out=1 << 24, N=5, H=24, W=32):
        rows, target = np.ascontiguousarray(rows, np.float32), np.ascontiguousarray(target, np.float32)
        return lib.dbw_lens_rectify_valid_u8(N, H, W, rows.ctypes.data, target.ctypes.data, out, None)

    assert rc(src=None) == -1 and b'null pointer' in lib.dbw_last_error()
    assert rc(out=None) == -1 and b'null pointer' in lib.dbw_last_error()
    assert rc_valid(out=None) == -1 and b'null pointer' in lib.dbw_last_error()
    assert rc(N=0) == -1 and b'N below 1' in lib.dbw_last_error()
    assert rc_valid(N=0) == -1 and b'N below 1' in lib.dbw_last_error()
    for over in (dict(H=1), dict(W=1)):
        assert rc(**over) == -1 and b'below 2 x 2' in lib.dbw_last_error(), over
    assert rc_valid(H=0) == -1 and b'bad size' in lib.dbw_last_error()
    for out in (base, base + n - 1, base - n + 1):
        assert rc(out=out) == -1 and b'overlap' in lib.dbw_last_error(), out
    for f in (rc, rc_valid):
        for col in (0, 4, 10, 15):
            bad = good.copy()
            bad[4, col] = np.nan
            assert f(rows=bad) == -1 and b'not finite' in lib.dbw_last_error(), col
        bad = good.copy()
        bad[0, 0] = 2.0
        assert f(rows=bad) == -1 and b'model id' in lib.dbw_last_error()
        bad = good.copy()
        bad[3, 2] = 0.0
        assert f(rows=bad) == -1 and b'focal length' in lib.dbw_last_error()
        bad = good.copy()
        bad[3, 1] = -4.0
        assert f(rows=bad) == -1 and b'focal length' in lib.dbw_last_error()
        bad_t = tgt.copy()
        bad_t[1] = np.inf
        assert f(target=bad_t) == -1 and b'not finite' in lib.dbw_last_error()
        bad_t = tgt.copy()
        bad_t[3] = 0.0
        assert f(target=bad_t) == -1 and b'not positive' in lib.dbw_last_error()
    import torch
    with pytest.raises(RuntimeError, match='GPU'):
        ops.rectify_u8(torch.zeros(5, 24, 32, 3, dtype=torch.uint8), torch.from_numpy(good), torch.from_numpy(tgt))
    with pytest.raises(RuntimeError, match='GPU'):
        ops.rectify_valid_u8(24, 32, torch.from_numpy(good), torch.from_numpy(tgt), device='cpu')
    assert _lib.LENS_RECT_N_PARAMS == RF.N_PARAMS == 16
