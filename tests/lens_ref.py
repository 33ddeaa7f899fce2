"""Checker side of the lens rectification: csrc/lens_math.h built for the host with g++ (tests/host_lens_math.cpp) behind the arguments of
ops.undistort_u8, and the cases the tests share.  Used by tests/test_host_lens_math.py (against an fp64 restatement written there),
tests/test_custom_scene_host.py and tests/test_gpu_lens.py (as the yardstick of the kernel)."""
import ctypes

import numpy as np
import torch

from host_build import host_lib

SHAPES = [(24, 32), (23, 37)]                                   # (H, W): the second with an odd width and row bases off the dword grid
COEFFS = [(0.12, 0.02, 0.0, 0.0, 0.003, -0.002),                # (k1, k2, k3, k4, p1, p2)
          (-0.25, 0.05, 0.0, 0.0, 0.004, 0.003),
          (0.08, -0.01, 0.002, 0.0005, -0.002, 0.001)]


def intrinsics(H, W):
    """(fx, fy, cx, cy) of the test camera."""
    return (0.9 * W, 0.92 * W, 0.51 * W, 0.48 * H)


def lens_array(intr, dist, zoom=1.0):
    """The 12 floats of dbw_images_undistort_u8: [fx, fy, cx, cy, 1/(zoom fx), 1/(zoom fy), k1, k2, k3, k4, p1, p2], the reciprocals in fp64
    and rounded once."""
    fx, fy, cx, cy = [float(v) for v in intr]
    return np.array([fx, fy, cx, cy, 1.0 / (zoom * fx), 1.0 / (zoom * fy)] + [float(v) for v in dist], dtype=np.float64).astype(np.float32)


def frames(N, H, W, seed=0):
    """(N,H,W,3) uint8: noise, with a corner of extremes."""
    rng = np.random.RandomState(seed + 7 * H + W)
    a = rng.randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    a[:, : H // 4, : W // 4] = rng.randint(0, 2, (N, H // 4, W // 4, 3)).astype(np.uint8) * 255
    return a


def lib():
    return host_lib('lens_math')


def source_host(H, W, lens):
    """(u, v), (H,W) fp32 each: the source index coordinates of every output pixel from the host build of the header, not clamped."""
    lens = np.ascontiguousarray(lens, dtype=np.float32)
    u, v = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    assert lib().host_lens_source(H, W, ctypes.c_void_p(lens.ctypes.data), ctypes.c_void_p(u.ctypes.data), ctypes.c_void_p(v.ctypes.data)) == 0
    return u, v


def undistort_host(src, intr, dist, zoom=1.0):
    """ops.undistort_u8 on the CPU through the host build of lens_math.h: src (N,H,W,3) uint8, numpy or CPU tensor -> the same kind."""
    a = np.ascontiguousarray(src.numpy() if torch.is_tensor(src) else src)
    assert a.dtype == np.uint8 and a.ndim == 4 and a.shape[3] == 3
    N, H, W, _ = a.shape
    lens = lens_array(intr, dist, zoom)
    out = np.zeros_like(a)
    assert lib().host_images_undistort_u8(ctypes.c_void_p(a.ctypes.data), N, H, W, ctypes.c_void_p(lens.ctypes.data), ctypes.c_void_p(out.ctypes.data)) == 0
    return torch.from_numpy(out) if torch.is_tensor(src) else out
