"""Checker side of the depth cloud: csrc/depth_math.h built for the host with g++ (tests/host_depth_math.cpp) behind the arguments of
ops.depth_cloud, with the integer accumulation and the emit in cell order written out in C++, and the cases the tests share.  Used by
tests/test_host_depth_math.py (against an fp64 restatement written there), tests/test_depth_cloud_host.py (as the yardstick of the numpy
path) and tests/test_gpu_depth_cloud.py (as the yardstick of the kernel)."""
import ctypes

import numpy as np

import lens_ref as LR
import rectify_ref as RF
from host_build import host_lib

KINDS = ('pinhole', 'radtan', 'fisheye')
SUB = 1024
UNIT = 1e-3                                                     # world units per depth step of the cases
GROUP = 16                                                      # csrc/depth_cloud.hip: DEPTH_GROUP, the frames of one launch
SHAPES = [(1, 1), (2, 2), (5, 7), (24, 32), (37, 67)]


def lib():
    return host_lib('depth_math')


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def box(lo, hi, G):
    """[lo_x, lo_y, lo_z, inv_step] fp32 of the cube [lo, hi]^3, inv_step = G * 1024 / (hi - lo) in fp64, rounded once."""
    return np.array([lo, lo, lo, G * float(SUB) / (float(hi) - float(lo))], dtype=np.float64).astype(np.float32)


def _args(depth, cams, target, poses, bx):
    depth = np.ascontiguousarray(depth, dtype=np.uint16)
    N = depth.shape[0]
    cams, target = np.ascontiguousarray(cams, dtype=np.float32), np.ascontiguousarray(target, dtype=np.float32)
    poses, bx = np.ascontiguousarray(poses, dtype=np.float32).reshape(N, 12), np.ascontiguousarray(bx, dtype=np.float32)
    assert depth.ndim == 3 and cams.shape == (N, 16) and target.shape == (4,) and bx.shape == (4,)
    return depth, cams, target, poses, bx


def samples_host(depth, cams, target, poses, bx, G, d_min=1, d_max=65535, stride=1, permille=0):
    """Every selected pixel through depth_sample of the header: cell (N,Hs,Ws) int32 (-1 dropped, -2 outside the box), q (N,Hs,Ws,3) int32."""
    depth, cams, target, poses, bx = _args(depth, cams, target, poses, bx)
    N, H, W = depth.shape
    Hs, Ws = -(-H // stride), -(-W // stride)
    cell, q = np.zeros((N, Hs, Ws), np.int32), np.zeros((N, Hs, Ws, 3), np.int32)
    assert lib().host_depth_samples(_p(depth), N, H, W, _p(cams), _p(target), _p(poses), _p(bx), G, d_min, d_max, stride, permille, _p(cell), _p(q)) == 0
    return cell, q


def cloud_host(depth, cams, target, poses, bx, G, d_min=1, d_max=65535, stride=1, permille=0, min_count=1):
    """dbw_lens_depth_cloud through the host build: (points (M,3) fp32, counts (M,) int32, info [M, accumulated, outside] int64)."""
    depth, cams, target, poses, bx = _args(depth, cams, target, poses, bx)
    N, H, W = depth.shape
    cc, cs = np.zeros(G ** 3, np.uint32), np.zeros((G ** 3, 3), np.uint64)
    points, counts, info = np.zeros((G ** 3, 3), np.float32), np.zeros(G ** 3, np.int32), np.zeros(3, np.int64)
    fn = lib().host_depth_cloud
    fn.restype = ctypes.c_longlong
    M = fn(_p(depth), N, H, W, _p(cams), _p(target), _p(poses), _p(bx), G, d_min, d_max, stride, permille, min_count, _p(cc), _p(cs), _p(points),
           _p(counts), _p(info))
    assert M == info[0]
    return points[:M].copy(), counts[:M].copy(), info


def intrinsics(H, W, n):
    """(fx, fy, cx, cy) of frame n: four cameras in turn; at 1x1 and 2x2 they still look through the middle of the frame."""
    f = max(W, 2.0)
    return [(0.9 * f, 0.92 * f, 0.51 * W, 0.48 * H), (0.8 * f, 0.83 * f, 0.5 * W, 0.5 * H), (1.0 * f, 1.0 * f, 0.47 * W, 0.53 * H),
            (0.9 * f, 0.92 * f, W // 2 + 0.5, H // 2 + 0.5)][n % 4]


def target_of(H, W):
    f = max(W, 2.0)
    return RF.target((0.8731 * f, 0.9017 * f, 0.4983 * W, 0.5071 * H))     # (no ratio to a camera's numbers that puts a whole row or column on a tie)


def coeffs(kind, n):
    if kind == 'pinhole':
        return (0.0,) * 6
    return LR.COEFFS[n % 3] if kind == 'radtan' else tuple(RF.FISHEYE_COEFFS[n % 3]) + (0.0, 0.0)


def look_at(eye, at=(0.0, 0.0, 0.0)):
    """(3,3) camera-to-world rotation of a camera at `eye` looking at `at`: columns x right, y down, z forward; world up is +z."""
    eye, at = np.asarray(eye, np.float64), np.asarray(at, np.float64)
    z = (at - eye) / np.linalg.norm(at - eye)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]))
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], 1)


def case(N, H, W, kind, seed=0, unit=UNIT, scale=1.0):
    """A chunk of N frames: cameras on a ring of radius 2.5 at height 1.2 looking at the origin, depths of 1.5 .. 3.5 world units that vary
    smoothly with a step edge across the frame and a few holes (0) -> (depth (N,H,W) uint16, cams (N,16), target (4,), poses (N,12)).
    scale: the whole scene, cameras and depth unit, shrunk about the origin (the depth steps stay what they are)."""
    rng = np.random.RandomState(seed + 131 * N + 7 * H + W)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    depth, intrs, dists, poses = [], [], [], []
    for n in range(N):
        a = 2 * np.pi * (n + rng.rand() * 0.5) / N
        eye = np.array([2.5 * np.cos(a), 2.5 * np.sin(a), 1.2])
        R = look_at(eye, rng.randn(3) * 0.1)
        d = 2.2 + 0.4 * np.sin(0.3 * ii + n) * np.cos(0.23 * jj) + 0.9 * (jj > W * (0.35 + 0.3 * rng.rand())) + rng.rand(H, W) * 0.004
        d = np.round(d / unit)
        d[rng.rand(H, W) < 0.03] = 0
        depth.append(d.astype(np.uint16))
        intrs.append(intrinsics(H, W, n))
        dists.append(coeffs(kind, n))
        poses.append(np.concatenate([(R * (unit * scale)).reshape(9), eye * scale]))
    models = [RF.FISHEYE if kind == 'fisheye' else RF.RADTAN] * N
    return np.stack(depth), RF.table(intrs, dists, models), target_of(H, W), np.array(poses, np.float64).astype(np.float32)


# the GPU list (tests/test_gpu_depth_cloud.py) and the numpy path's (tests/test_depth_cloud_host.py): N crosses the frames of a launch at 17
# and twice at 33; every shape, kind, G, stride, edge and min_count of the issue appears, not their full product
CASES = [dict(N=N, H=H, W=W, kind=KINDS[(k + a) % 3], G=(1, 2, 8, 64)[(k + a) % 4], stride=(1, 3)[(k + a // 2) % 2], permille=(0, 50)[(k + a) % 2],
              min_count=(1, 3)[(a + k // 2) % 2])
         for a, N in enumerate((1, 3, GROUP + 1, 33)) for k, (H, W) in enumerate(SHAPES)]
CASES += [dict(N=3, H=24, W=32, kind=kind, G=G, stride=stride, permille=permille, min_count=min_count)
          for kind, G, stride, permille, min_count in (('pinhole', 64, 1, 50, 1), ('radtan', 8, 3, 0, 3), ('fisheye', 2, 1, 50, 3), ('fisheye', 64, 3, 50, 1),
                                                       ('radtan', 1, 1, 0, 1), ('pinhole', 8, 1, 0, 3))]


def case_id(c):
    return '{N}x{H}x{W}-{kind}-G{G}-s{stride}-e{permille}-m{min_count}'.format(**c)
