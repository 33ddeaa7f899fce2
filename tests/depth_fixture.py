"""A synthetic capture with depth maps in the layout dataset.CustomScene(cloud='depth') reads, for tests/test_depth_cloud_host.py and
tests/test_gpu_depth_cloud.py: the ground plane z = 0 and two boxes standing on it, seen by 6 cameras on a ring, written with
custom_fixture.write_capture (noise images: the cloud does not read them) and then given one 16-bit PNG per frame whose depth is ray-cast
analytically in fp64 and quantised to the depth unit, `depth_file_path` on the frames and `depth_unit_scale_factor` at the top level.
A lens is cast through by inverting the radial-tangential model with an fp64 fixed-point iteration."""
import json
import os

import numpy as np
from PIL import Image

import lens_ref as LR
from custom_fixture import write_capture

UNIT = 1e-3                                                     # metres per depth step: 1 mm
BOXES = [((-1.2, -0.8, 0.0), (-0.2, 0.2, 0.9)), ((0.5, 0.1, 0.0), (1.3, 1.1, 0.6))]      # (lo, hi) in metres, standing on z = 0
MILD = (0.04, -0.008, 0.0, 0.0, 0.001, -0.0007)                 # (k1, k2, k3, k4, p1, p2): a mild radial-tangential lens


def cameras_gl(n=6, radius=4.0, height=2.5):
    """(n,4,4) OpenGL camera-to-world matrices (x right, y up, z backwards) on a ring, looking at a point just above the ground."""
    out = []
    for k in range(n):
        a = 2 * np.pi * (k + 0.3) / n
        eye = np.array([radius * np.cos(a), radius * np.sin(a), height + 0.2 * np.sin(3 * a)])
        fwd = np.array([0.1 * np.cos(2 * a), 0.1 * np.sin(a), 0.3]) - eye
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
        right /= np.linalg.norm(right)
        M = np.eye(4)
        M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = right, np.cross(right, fwd), -fwd, eye
        out.append(M)
    return np.stack(out)


def undistort64(xd, yd, dist, n_iter=60):
    """The pinhole coordinates (x, y) whose radial-tangential image is (xd, yd): the fixed point of x = (xd - tangential(x, y)) / radial(x, y)."""
    k1, k2, k3, k4, p1, p2 = dist
    x, y = xd.copy(), yd.copy()
    for _ in range(n_iter):
        r2 = x * x + y * y
        d = 1 + r2 * (k1 + r2 * (k2 + r2 * (k3 + r2 * k4)))
        x, y = (xd - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) / d, (yd - (2 * p2 * x * y + p1 * (r2 + 2 * y * y))) / d
    return x, y


def _slab(o, d, lo, hi):
    """the entry distance of the rays o + t d into the box [lo, hi] (inf where they miss), arrays (..., 3)"""
    with np.errstate(divide='ignore', invalid='ignore'):
        t0, t1 = (np.asarray(lo) - o) / d, (np.asarray(hi) - o) / d
    near, far = np.nanmax(np.minimum(t0, t1), -1), np.nanmin(np.maximum(t0, t1), -1)
    return np.where((near <= far) & (near > 0), near, np.inf)


def cast(c2w, intr, dist, H, W, unit=UNIT):
    """The depth map (H,W) uint16 of one camera: the z-depth along the optical axis of the first surface on the ray through every pixel
    centre, in steps of `unit` (0: nothing hit, or farther than 65535 steps), and the same in fp64 metres (inf)."""
    fx, fy, cx, cy = intr
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    x, y = undistort64((j + 0.5 - cx) / fx, (i + 0.5 - cy) / fy, dist)
    d = np.stack([x, -y, -np.ones_like(x)], -1) @ c2w[:3, :3].T                 # per unit of z-depth
    o = c2w[:3, 3]
    with np.errstate(divide='ignore'):
        t = np.where(d[..., 2] < 0, -o[2] / d[..., 2], np.inf)
    for lo, hi in BOXES:
        t = np.minimum(t, _slab(o, d, lo, hi))
    steps = np.round(t / unit)
    return np.where(np.isfinite(t) & (steps <= 65535), steps, 0).astype(np.uint16), t


def surface_distance(p):
    """The distance in metres of points (n,3) of the file's frame to the nearest surface: the plane z = 0 or a box's faces."""
    p = np.asarray(p, np.float64)
    best = np.abs(p[:, 2])
    for lo, hi in BOXES:
        lo, hi = np.asarray(lo), np.asarray(hi)
        out = np.linalg.norm(np.maximum(np.maximum(lo - p, p - hi), 0.0), axis=1)               # outside the solid: to the solid
        inside = np.minimum(p - lo, hi - p).min(1)                                               # inside: to the nearest face
        best = np.minimum(best, np.where(inside > 0, inside, out))
    return best


def write_depth_capture(root, tag, dist=(0.0,) * 6, H=24, W=32, depth_size=(48, 64), n=6, unit=UNIT, unit_in_file=True, skip=(), **kw):
    """The capture with its depth maps -> (depth (n,Hd,Wd) uint16, the fp64 z-depths in metres, the camera-to-world matrices).  The images
    are H x W, the depth maps depth_size; skip: frames left without a depth map."""
    c2w = cameras_gl(n)
    per_frame = {k: {'transform_matrix': c2w[k].tolist()} for k in range(n)}
    write_capture(root, tag, n=n, H=H, W=W, dist=dist, per_frame=per_frame, **kw)
    folder = os.path.join(str(root), 'custom', tag)
    os.makedirs(os.path.join(folder, 'depth'), exist_ok=True)
    Hd, Wd = depth_size
    fx, fy, cx, cy = LR.intrinsics(H, W)
    intr = (fx * Wd / W, fy * Hd / H, cx * Wd / W, cy * Hd / H)
    with open(os.path.join(folder, 'transforms.json')) as f:
        meta = json.load(f)
    depth, metres = [], []
    for k in range(n):
        d, t = cast(c2w[k], intr, dist, Hd, Wd, unit)
        depth.append(d)
        metres.append(t)
        if k in skip:
            continue
        rel = f'depth/frame_{k + 1:05d}.png'
        Image.fromarray(d).save(os.path.join(folder, rel))
        meta['frames'][k]['depth_file_path'] = rel
    if unit_in_file:
        meta['depth_unit_scale_factor'] = unit
    with open(os.path.join(folder, 'transforms.json'), 'w') as f:
        json.dump(meta, f)
    return np.stack(depth), np.stack(metres), c2w
