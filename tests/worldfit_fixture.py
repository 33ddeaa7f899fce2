"""Seeded synthetic captures for the world-frame tests (tests/test_worldfit_host.py, tests/test_gpu_worldfit.py): a noisy ground plane, a box
of object points standing on it, a wall distractor, far clutter and a wobbling ring of cameras, all under a random similarity, with the
truth the estimator is held to; small plane clouds for the device-vs-host tests; a writer for the CustomScene layout."""
import json
import os

import numpy as np

GROUND_NOISE = 0.004
N_CAPTURES = 8


def _rotation(rng):
    Q, _ = np.linalg.qr(rng.randn(3, 3))
    if np.linalg.det(Q) < 0:
        Q[:, 0] *= -1
    return Q


def capture(seed, n_cams=24, similarity=True):
    """-> dict(points (N,3) fp32, cam2world (V,4,4) fp64 OpenGL, n (3,), d, foot (3,), scale): the plane n . p = d is the true ground, n
    towards the cameras; foot is the centre of the box's footprint.  Canonical frame before the similarity: ground y = 0, box 0.5 x 0.3 x
    0.4 at the origin, wall x = 1.7, cameras on a ring of radius 2 about 25 degrees up."""
    rng = np.random.RandomState(1000 + seed)
    g = np.stack([rng.uniform(-1.5, 1.5, 3300), rng.randn(3300) * GROUND_NOISE, rng.uniform(-1.5, 1.5, 3300)], 1)
    half = np.array([0.25, 0.15, 0.2])
    box = rng.uniform(-1, 1, (1200, 3))
    face = rng.randint(0, 3, 1200)
    box[np.arange(1200), face] = np.where(face == 1, 1.0, np.sign(box[np.arange(1200), face]))      # on the five faces a camera can see
    box = box * half + np.array([0.0, 0.15 + 3 * GROUND_NOISE, 0.0])
    wall = np.stack([1.7 + rng.randn(1200) * GROUND_NOISE, rng.uniform(0, 1.2, 1200), rng.uniform(-1.5, 1.5, 1200)], 1)
    far = rng.randn(300, 3)
    far = far / np.linalg.norm(far, axis=1, keepdims=True) * rng.uniform(3, 6, (300, 1))
    pts = np.concatenate([g, box, wall, far])
    pts = pts[rng.permutation(len(pts))]
    az = np.arange(n_cams) * (2 * np.pi / n_cams) + rng.uniform(0, 1)
    el = np.radians(25) + 0.15 * np.sin(3 * az)
    C = 2.0 * np.stack([np.cos(el) * np.sin(az), np.sin(el), np.cos(el) * np.cos(az)], 1) * (1 + 0.05 * rng.randn(n_cams, 1))
    target = np.array([0.0, 0.15, 0.0]) + 0.03 * rng.randn(n_cams, 3)
    c2w = np.tile(np.eye(4), (n_cams, 1, 1))
    for i in range(n_cams):
        z = C[i] - target[i]
        z /= np.linalg.norm(z)
        upw = np.array([0.0, 1.0, 0.0]) + 0.05 * rng.randn(3)
        x = np.cross(upw, z)
        x /= np.linalg.norm(x)
        c2w[i, :3, :3] = np.stack([x, np.cross(z, x), z], 1)
        c2w[i, :3, 3] = C[i]
    n, d, foot, s = np.array([0.0, 1.0, 0.0]), 0.0, np.zeros(3), 1.0
    if similarity:
        Q, s, t = _rotation(rng), float(rng.uniform(0.5, 2.0)), rng.randn(3)
        pts = s * pts @ Q.T + t
        c2w[:, :3, :3] = Q @ c2w[:, :3, :3]
        c2w[:, :3, 3] = s * c2w[:, :3, 3] @ Q.T + t
        n = Q @ n
        foot = s * Q @ foot + t
        d = float(n @ foot)
    return dict(points=pts.astype(np.float32), cam2world=c2w, n=n, d=d, foot=foot, scale=s)


def errors(frame, cap):
    """(angle between the normals in degrees, |offset error| / r0, |foot error| / r0) of a WorldFrame against the capture's truth"""
    n, d = frame.plane
    ang = float(np.degrees(np.arccos(np.clip(n @ cap['n'], -1, 1))))
    return ang, abs(d - cap['d']) / frame.r0, float(np.linalg.norm(frame.c - cap['foot'])) / frame.r0


def single_wall(seed=0):
    """a capture whose cloud is an exact wall x = 1.7 alone (every triple's normal is the x axis, at 90 degrees from the cameras' up): no
    plane under the cameras"""
    cap = capture(seed, similarity=False)
    rng = np.random.RandomState(seed)
    cap['points'] = np.stack([np.full(500, 1.7), rng.uniform(0, 1.2, 500), rng.uniform(-1.5, 1.5, 500)], 1).astype(np.float32)
    return cap


def plane_cloud(N, seed):
    """-> (points (N,3) fp32, cams (5,3) fp32, up (3,) fp32): 60 % of the points on a tilted plane with noise, the rest in a blob; cameras
    above the plane.  N >= 3."""
    rng = np.random.RandomState(seed)
    k = max(3, int(0.6 * N)) if N > 3 else 3
    xy = rng.uniform(-1, 1, (N, 2))
    z = np.where(np.arange(N) < k, 0.2 * xy[:, 0] - 0.1 * xy[:, 1] + 0.05 + 0.004 * rng.randn(N), rng.uniform(-0.5, 1.0, N))
    pts = np.concatenate([xy, z[:, None]], 1)[rng.permutation(N)].astype(np.float32)
    cams = (np.array([0.0, 0.0, 1.5]) + 0.3 * rng.randn(5, 3)).astype(np.float32)
    return pts, cams, np.array([0.0, 0.0, 1.0], np.float32)


def write_capture(root, tag, cap, n_frames=6, H=16, W=24, with_points=True):
    """The capture in the layout dataset.CustomScene reads: transforms.json (pinhole intrinsics, the first n_frames cameras spread over the
    ring), images/frame_XXXXX.png of noise, and a binary points.ply.  -> the indices of the cameras written."""
    from PIL import Image
    folder = os.path.join(str(root), 'custom', tag)
    os.makedirs(os.path.join(folder, 'images'), exist_ok=True)
    rng = np.random.RandomState(5)
    ids = np.linspace(0, len(cap['cam2world']) - 1, n_frames).astype(int).tolist()
    meta = {'fl_x': 1.2 * W, 'fl_y': 1.2 * W, 'cx': W / 2, 'cy': H / 2, 'w': W, 'h': H, 'camera_model': 'PINHOLE', 'frames': []}
    for k, i in enumerate(ids):
        rel = f'images/frame_{k + 1:05d}.png'
        Image.fromarray(rng.randint(0, 256, (H, W, 3)).astype(np.uint8), 'RGB').save(os.path.join(folder, rel))
        meta['frames'].append({'file_path': rel, 'transform_matrix': cap['cam2world'][i].tolist()})
    with open(os.path.join(folder, 'transforms.json'), 'w') as f:
        json.dump(meta, f)
    if with_points:
        p = np.ascontiguousarray(cap['points'], dtype='<f4')
        with open(os.path.join(folder, 'points.ply'), 'wb') as f:
            f.write(b'ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n' % len(p))
            f.write(p.tobytes())
    return ids
