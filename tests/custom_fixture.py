"""A synthetic capture in the layout dataset.CustomScene reads, for tests/test_custom_scene_host.py and tests/test_gpu_lens.py:
<root>/custom/<tag>/transforms.json (top-level intrinsics of the test camera of tests/lens_ref.py, OpenGL camera-to-world matrices) next
to images/frame_XXXXX.png, optionally a dataparser_transforms.json and an ascii points.ply."""
import json
import os

import numpy as np
from PIL import Image

import lens_ref as LR


def cameras_to_world(n, seed=3):
    """(n,4,4) OpenGL camera-to-world matrices (x right, y up, z backwards): cameras around a point away from the origin, roughly upright."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        Q, _ = np.linalg.qr(rng.randn(3, 3) * 0.35 + np.eye(3))
        Q = Q * np.sign(np.diag(Q))[None]                       # near the identity ...
        if np.linalg.det(Q) < 0:
            Q[:, 2] *= -1
        tilt = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], dtype=np.float64)       # ... with the cameras' up axis along the world's -z, say
        M = np.eye(4)
        M[:3, :3] = tilt @ Q
        M[:3, 3] = np.array([2.0, -1.0, 5.0]) + rng.randn(3) * 1.5
        out.append(M)
    return np.stack(out)


def write_capture(root, tag, n=6, H=24, W=32, dist=LR.COEFFS[0], seed=0, camera_model='OPENCV', with_extension=True, dataparser=None,
                  with_points=False, per_frame=None, frame_size=None):
    """Writes the capture and returns (the raw frames (n,H,W,3) uint8 in file order, the camera-to-world matrices (n,4,4)).  dist: the six
    coefficients (k3, k4 are written only where they are not 0: absent means 0).  with_extension=False leaves the suffix off file_path.
    dataparser: (transform 3x4, scale).  per_frame: {frame index: {key: value}} merged into the frames.  frame_size: {frame index: (H, W)}
    of files written at another size."""
    folder = os.path.join(str(root), 'custom', tag)
    os.makedirs(os.path.join(folder, 'images'), exist_ok=True)
    frames = LR.frames(n, H, W, seed=seed)
    c2w = cameras_to_world(n, seed=seed + 3)
    fx, fy, cx, cy = LR.intrinsics(H, W)
    meta = {'fl_x': fx, 'fl_y': fy, 'cx': cx, 'cy': cy, 'w': W, 'h': H, 'frames': []}
    if camera_model is not None:
        meta['camera_model'] = camera_model
    for name, v in zip(('k1', 'k2', 'k3', 'k4', 'p1', 'p2'), dist):
        if v != 0 or name in ('k1', 'k2', 'p1', 'p2'):
            meta[name] = v
    for i in range(n):
        rel = f'images/frame_{i + 1:05d}.png'
        a = frames[i]
        if frame_size and i in frame_size:
            a = np.zeros(tuple(frame_size[i]) + (3,), np.uint8)
        Image.fromarray(a, 'RGB').save(os.path.join(folder, rel))
        frame = {'file_path': rel if with_extension else rel[:-4], 'transform_matrix': c2w[i].tolist()}
        frame.update((per_frame or {}).get(i, {}))
        meta['frames'].append(frame)
    with open(os.path.join(folder, 'transforms.json'), 'w') as f:
        json.dump(meta, f)
    if dataparser is not None:
        with open(os.path.join(folder, 'dataparser_transforms.json'), 'w') as f:
            json.dump({'transform': np.asarray(dataparser[0]).tolist(), 'scale': float(dataparser[1])}, f)
    if with_points:
        pts = np.random.RandomState(seed + 1).randn(30, 3) + np.array([2.0, -1.0, 5.0])
        with open(os.path.join(folder, 'points.ply'), 'w') as f:
            f.write('ply\nformat ascii 1.0\nelement vertex 30\nproperty float x\nproperty float y\nproperty float z\nend_header\n')
            for p in pts:
                f.write('%r %r %r\n' % (float(np.float32(p[0])), float(np.float32(p[1])), float(np.float32(p[2]))))
    return frames, c2w
