"""Checker side of the per-frame rectification: the per-frame part of csrc/lens_math.h built for the host with g++
(tests/host_rectify_math.cpp) behind the arguments of ops.rectify_u8, and the cases the tests share.  Used by
tests/test_host_rectify_math.py (against an fp64 restatement written there), tests/test_rectify_scene_host.py and
tests/test_gpu_rectify.py (as the yardstick of the kernel)."""
import ctypes

import numpy as np
import torch

import lens_ref as LR
from host_build import host_lib

SHAPES = LR.SHAPES
RADTAN, FISHEYE = 0, 1
N_PARAMS = 16
FISHEYE_COEFFS = [(0.05, -0.01, 0.002, 0.0), (-0.04, 0.006, -0.001, 0.0002), (0.0, 0.0, 0.0, 0.0)]       # (k1, k2, k3, k4)
CAMERA_NAMES = ('A', 'B', 'C', 'D')


def cameras(H, W):
    """{'A'..'D': (fx, fy, cx, cy)}: A the test camera of lens_ref, B and C other focal lengths and principal points, D A's focal lengths
    with the principal point on a pixel centre (the r2 == 0 case)."""
    return {'A': (0.9 * W, 0.92 * W, 0.51 * W, 0.48 * H), 'B': (0.8 * W, 0.83 * W, 0.5 * W, 0.5 * H), 'C': (1.0 * W, 1.0 * W, 0.47 * W, 0.53 * H),
            'D': (0.9 * W, 0.92 * W, W // 2 + 0.5, 11.5)}


def coeff_sets(model):
    """The (k1, k2, k3, k4, p1, p2) sets of a model."""
    return [tuple(k) + (0.0, 0.0) for k in FISHEYE_COEFFS] if model == FISHEYE else list(LR.COEFFS)


def table(intrs, dists, models):
    """The (N,16) fp32 `cams` table of dbw_lens_rectify_u8, written out by hand."""
    t = np.zeros((len(intrs), N_PARAMS), np.float64)
    for n, (intr, dist, model) in enumerate(zip(intrs, dists, models)):
        t[n, 0], t[n, 1:5], t[n, 5:11] = model, intr, dist
    return t.astype(np.float32)


def target(intr0, zoom=1.0):
    """The 4 floats [cx0, cy0, 1/(zoom fx0), 1/(zoom fy0)], the reciprocals in fp64 and rounded once."""
    fx, fy, cx, cy = [float(v) for v in intr0]
    return np.array([cx, cy, 1.0 / (zoom * fx), 1.0 / (zoom * fy)], dtype=np.float64).astype(np.float32)


def median_target(H, W):
    """The pinhole of the four cameras: the median of each component (dataset.common_pinhole, restated)."""
    return tuple(float(v) for v in np.median(np.array(list(cameras(H, W).values()), np.float64), axis=0))


def lib():
    return host_lib('rectify_math')


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def atan_host(t):
    t = np.ascontiguousarray(t, dtype=np.float32)
    out = np.zeros_like(t)
    assert lib().host_lens_atan(t.size, _p(t), _p(out)) == 0
    return out


def source_host(H, W, row, tgt):
    """(u, v), (H,W) fp32 each: the source index coordinates of every output pixel for one row of the table, not clamped."""
    row, tgt = np.ascontiguousarray(row, dtype=np.float32), np.ascontiguousarray(tgt, dtype=np.float32)
    u, v = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    assert lib().host_lens_rect_source(H, W, _p(row), _p(tgt), _p(u), _p(v)) == 0
    return u, v


def rectify_host(src, rows, tgt):
    """ops.rectify_u8 on the CPU through the host build: src (N,H,W,3) uint8, numpy or CPU tensor -> the same kind."""
    a = np.ascontiguousarray(src.numpy() if torch.is_tensor(src) else src)
    assert a.dtype == np.uint8 and a.ndim == 4 and a.shape[3] == 3
    N, H, W, _ = a.shape
    rows = np.ascontiguousarray(rows.numpy() if torch.is_tensor(rows) else rows, dtype=np.float32)
    tgt = np.ascontiguousarray(tgt.numpy() if torch.is_tensor(tgt) else tgt, dtype=np.float32)
    assert rows.shape == (N, N_PARAMS) and tgt.shape == (4,)
    out = np.zeros_like(a)
    assert lib().host_lens_rectify_u8(_p(a), N, H, W, _p(rows), _p(tgt), _p(out)) == 0
    return torch.from_numpy(out) if torch.is_tensor(src) else out


def valid_host(H, W, rows, tgt):
    """ops.rectify_valid_u8 on the CPU: (N,H,W) uint8 numpy."""
    rows = np.ascontiguousarray(rows.numpy() if torch.is_tensor(rows) else rows, dtype=np.float32)
    tgt = np.ascontiguousarray(tgt.numpy() if torch.is_tensor(tgt) else tgt, dtype=np.float32)
    out = np.zeros((rows.shape[0], H, W), np.uint8)
    assert lib().host_lens_rectify_valid_u8(rows.shape[0], H, W, _p(rows), _p(tgt), _p(out)) == 0
    return out


def write_fisheye_capture(root, tag, n=6, H=24, W=32, **kw):
    """custom_fixture.write_capture of an OPENCV_FISHEYE capture whose frames cycle through the cameras A, B, C, D, the fifth frame with a
    k1 of its own -> (frames (n,H,W,3) uint8, intrs (n,4), dists (n,6), models (n,)) as the loader should read them."""
    from custom_fixture import write_capture
    cams, k = cameras(H, W), FISHEYE_COEFFS[0]
    per_frame, intrs, dists = {}, [], []
    for i in range(n):
        c = cams[CAMERA_NAMES[i % 4]]
        per_frame[i] = dict(zip(('fl_x', 'fl_y', 'cx', 'cy'), c))
        d = k + (0.0, 0.0)
        if i == 4:
            per_frame[i]['k1'] = -0.04
            d = (-0.04,) + d[1:]
        intrs.append(c)
        dists.append(d)
    frames, _ = write_capture(root, tag, n=n, H=H, W=W, dist=k + (0.0, 0.0), camera_model='OPENCV_FISHEYE', per_frame=per_frame, **kw)
    return frames, np.array(intrs, np.float64), np.array(dists, np.float64), np.full(n, FISHEYE, np.int64)


def five_frames(H, W, model, dist, zoom=1.0):
    """The chunk of the GPU tests: 5 frames taken by A, B, C, D, A with one coefficient set -> (rows (5,16), target (4,)) with the median
    target of the four cameras."""
    cams = cameras(H, W)
    intrs = [cams[c] for c in ('A', 'B', 'C', 'D', 'A')]
    return table(intrs, [dist] * 5, [model] * 5), target(median_target(H, W), zoom)
