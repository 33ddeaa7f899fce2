"""CPU tests of the lens rectification's arithmetic: csrc/lens_math.h built for the host with g++ (tests/host_lens_math.cpp, through
tests/lens_ref.py) against an fp64 numpy restatement of the map written here, and dataset.lens_zoom.

Bounds, all derived:
  * coordinates: delta = 64 * 2^-23 * max(H, W) px -- 64 roundings of the largest coordinate, for a chain of about 40 fp32 operations
    (2.8e-4 px at 37 px);
  * bytes: 0.5 + 510 * delta around the unrounded fp64 bilinear value -- half a level for the rounding, and a bilinear value moves by at
    most 255 per pixel of coordinate error on each axis.  Every byte is held to it, no share is left out;
  * direction of the map: 1 + (60 + 50) * (2 pi m / 16)^2 / 8 levels, see test_the_map_runs_from_the_pinhole_frame_into_the_distorted_one."""
import numpy as np
import pytest
import torch

import lens_ref as LR
from dbw_amd import dataset as DS
from dbw_amd import ops

CASES = [(H, W, k) for (H, W) in LR.SHAPES for k in range(len(LR.COEFFS))]


def distort64(x, y, dist):
    """OpenCV's radial-tangential model on normalised coordinates, fp64."""
    k1, k2, k3, k4, p1, p2 = dist
    r2 = x * x + y * y
    d = 1 + r2 * (k1 + r2 * (k2 + r2 * (k3 + r2 * k4)))
    return x * d + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * d + 2 * p2 * x * y + p1 * (r2 + 2 * y * y)


def source64(H, W, intr, dist, zoom, i=None, j=None):
    """The fp64 restatement: source index coordinates (u, v) of the output pixels (i, j) (the whole frame by default; fractional allowed)."""
    fx, fy, cx, cy = intr
    if i is None:
        i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    x, y = (j + 0.5 - cx) / (zoom * fx), (i + 0.5 - cy) / (zoom * fy)
    xd, yd = distort64(x, y, dist)
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


def _case(H, W, k):
    intr, dist = LR.intrinsics(H, W), LR.COEFFS[k]
    return intr, dist, DS.lens_zoom(H, W, intr, dist)


@pytest.mark.parametrize('H,W,k', CASES)
def test_the_header_against_the_fp64_restatement(H, W, k):
    intr, dist, zoom = _case(H, W, k)
    delta = 64 * 2.0 ** -23 * max(H, W)
    u64, v64 = source64(H, W, intr, dist, zoom)
    u32, v32 = LR.source_host(H, W, LR.lens_array(intr, dist, zoom))
    eu, ev = float(np.abs(u32 - u64).max()), float(np.abs(v32 - v64).max())
    print(f'{H}x{W} set {k}: zoom {zoom:.6f}, |du| {eu:.3g}, |dv| {ev:.3g} px (bound {delta:.3g})')
    assert eu <= delta and ev <= delta
    src = LR.frames(3, H, W)
    got = LR.undistort_host(src, intr, dist, zoom)
    assert got.shape == src.shape and got.dtype == np.uint8
    want = np.stack([bilinear64(f, u64, v64) for f in src])
    eb = float(np.abs(got.astype(np.float64) - want).max())
    print(f'  bytes: {eb:.6f} levels from the fp64 value (bound {0.5 + 510 * delta:.6f})')
    assert eb <= 0.5 + 510 * delta
    # the binding's array is the checker's
    assert np.array_equal(ops.lens_params(intr, dist, zoom).numpy(), LR.lens_array(intr, dist, zoom))


def test_swapped_tangential_coefficients_are_seen_by_the_coordinate_bound():
    H, W = LR.SHAPES[1]
    intr, dist = LR.intrinsics(H, W), LR.COEFFS[0]
    swapped = dist[:4] + (dist[5], dist[4])
    u64, v64 = source64(H, W, intr, dist, 1.0)
    u32, v32 = LR.source_host(H, W, LR.lens_array(intr, swapped, 1.0))
    assert max(np.abs(u32 - u64).max(), np.abs(v32 - v64).max()) > 64 * 2.0 ** -23 * max(H, W)


@pytest.mark.parametrize('H,W', LR.SHAPES)
def test_no_distortion_and_no_zoom_is_the_identity(H, W):
    src = LR.frames(3, H, W, seed=1)
    assert np.array_equal(LR.undistort_host(src, LR.intrinsics(H, W), (0.0,) * 6, 1.0), src)


def _undistort64(xd, yd, dist, rounds=100):
    """The inverse of distort64 by fixed-point iteration."""
    k1, k2, k3, k4, p1, p2 = dist
    x, y = xd.copy(), yd.copy()
    for _ in range(rounds):
        r2 = x * x + y * y
        d = 1 + r2 * (k1 + r2 * (k2 + r2 * (k3 + r2 * k4)))
        x, y = (xd - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) / d, (yd - (2 * p2 * x * y + p1 * (r2 + 2 * y * y))) / d
    return x, y


def _pattern(x_px, y_px):
    return 127.5 + 60 * np.sin(2 * np.pi * x_px / 16) + 50 * np.cos(2 * np.pi * y_px / 16 + 0.3)


def _direction_error(H, W, intr, dist, zoom, header_dist):
    """Largest |rectified byte - pattern| over the frame, and the bound.  The distorted frame is painted with `dist`, rectified by the
    header with `header_dist`."""
    fx, fy, cx, cy = intr
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    xd, yd = (xs + 0.5 - cx) / fx, (ys + 0.5 - cy) / fy
    x, y = _undistort64(xd, yd, dist)
    rx, ry = distort64(x, y, dist)
    assert max(np.abs(rx - xd).max(), np.abs(ry - yd).max()) < 1e-12              # the inversion's residual
    painted = np.clip(np.floor(_pattern(x * zoom * fx + cx, y * zoom * fy + cy) + 0.5), 0, 255).astype(np.uint8)
    src = np.repeat(painted[None, :, :, None], 3, 3)
    got = LR.undistort_host(src, intr, header_dist, zoom)[0, :, :, 0].astype(np.float64)
    want = _pattern(xs + 0.5, ys + 0.5)
    # m: the largest local magnification of the fp64 map, by central differences of half a pixel
    e = 0.5
    jac = np.stack([(np.stack(source64(H, W, intr, dist, zoom, ys + di, xs + dj)) - np.stack(source64(H, W, intr, dist, zoom, ys - di, xs - dj))) / (2 * e)
                    for di, dj in ((0, e), (e, 0))], -1)                           # (2: u v, H, W, 2: d/dj d/di)
    sv = np.linalg.svd(np.moveaxis(jac, 0, 2), compute_uv=False)                   # (H, W, 2) singular values
    m = float(sv.max())
    return float(np.abs(got - want).max()), 1 + (60 + 50) * (2 * np.pi * m / 16) ** 2 / 8, m


@pytest.mark.parametrize('H,W,k', CASES)
def test_the_map_runs_from_the_pinhole_frame_into_the_distorted_one(H, W, k):
    """A distorted frame of an analytic pattern, painted by inverting the distortion in fp64 per source pixel, must come out of the
    rectification as the pattern at the output's pinhole coordinates.  Bound: half a level for each of the two roundings to a byte, plus
    the error of a bilinear cell on a function of amplitude 60 + 50 whose phase advances by at most 2 pi m / 16 per source pixel,
    (60 + 50) (2 pi m / 16)^2 / 8; m is the largest local magnification of the fp64 map anywhere in the frame (the largest singular value
    of its Jacobian), measured by central differences.
    This test FAILS when the sign of k1 is flipped in the header's map (asserted below by handing the header the flipped coefficient:
    the error then is an order of magnitude above the bound); swapped tangential coefficients are too small to show in this property at
    these values of p1, p2, the fp64 coordinate comparison above catches them."""
    intr, dist, zoom = _case(H, W, k)
    err, bound, m = _direction_error(H, W, intr, dist, zoom, dist)
    flipped, _, _ = _direction_error(H, W, intr, dist, zoom, (-dist[0],) + dist[1:])
    print(f'{H}x{W} set {k}: zoom {zoom:.4f}, m {m:.4f}: error {err:.3f} levels (bound {bound:.3f}); with k1 flipped {flipped:.1f}')
    assert err <= bound
    assert flipped > 2 * bound


@pytest.mark.parametrize('H,W', LR.SHAPES)
def test_lens_zoom(H, W):
    intr = LR.intrinsics(H, W)
    i = np.concatenate([np.zeros(W), np.full(W, H - 1.0), np.arange(H), np.arange(H)])
    j = np.concatenate([np.arange(W), np.arange(W), np.zeros(H), np.full(H, W - 1.0)])

    def inside(dist, s):
        u, v = source64(H, W, intr, dist, s, i, j)
        return bool(np.all((u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)))

    assert DS.lens_zoom(H, W, intr, LR.COEFFS[1]) == 1.0 and inside(LR.COEFFS[1], 1.0)
    for k, (lo, hi) in ((0, (1.055, 1.063)), (2, (1.032, 1.036))):
        s = DS.lens_zoom(H, W, intr, LR.COEFFS[k])
        print(f'{H}x{W} set {k}: zoom {s:.6f}')
        assert lo - 5e-4 <= s <= hi + 5e-4                                         # (the figures of the numpy model, to their last digit)
        assert inside(LR.COEFFS[k], s) and not inside(LR.COEFFS[k], s * (1 - 1e-3))
    # k1 = 3: a zoom of 2 does not suffice on a wide lens (fx = fy = 0.4 W: the corner's radius stays at 0.7 and the radial factor above
    # 2) and is refused; on the narrower test camera (corner radius 0.35 at a zoom of 2, factor 1.4) a zoom below 2 still exists
    k1_3 = (3.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError, match='zoom of 2'):
        DS.lens_zoom(H, W, (0.4 * W, 0.4 * W) + intr[2:], k1_3)
    s = DS.lens_zoom(H, W, intr, k1_3)
    assert 1 < s < 2 and inside(k1_3, s) and not inside(k1_3, s * (1 - 1e-3))
