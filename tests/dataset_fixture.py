"""A synthetic scene directory in the layout the reference's datasets read (src/dataset/dtu.py, bmvs.py), for tests/test_dataset_host.py and
tests/test_gpu_ingest.py: <root>/<DTU|BlendedMVS>/<tag>/image/*.png, cameras.npz next to image/ in the IDR layout, and for DTU an ascii
Points/stl/stlNNN_total.ply."""
import os

import numpy as np
from PIL import Image

SCALE = np.diag([350.0, 350.0, 350.0, 1.0])
SCALE[:3, 3] = [10.0, -25.0, 600.0]                             # scale_mat: normalised frame -> world (mm)


def projection_matrices(n_views, H, W, seed=3):
    """world_mat_i (4,4): pinhole cameras on a sphere of 900 mm around the scene's centre, looking at it.  (H, W): the size the matrices
    refer to -- the dataset's raw_img_size, whatever the size of the files (the loaders take it from the class, dtu.py:44)."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n_views):
        Q, _ = np.linalg.qr(rng.randn(3, 3))
        R_w2c = Q * np.sign(np.linalg.det(Q))
        C = SCALE[:3, 3] + R_w2c.T @ np.array([0.0, 0.0, -900.0]) + rng.randn(3) * 30
        Kcv = np.array([[1.8 * W, 0.0, 0.51 * W], [0.0, 1.8 * W, 0.52 * H], [0.0, 0.0, 1.0]])
        Wm = np.eye(4)
        Wm[:3] = Kcv @ np.concatenate([R_w2c, (-R_w2c @ C)[:, None]], 1)
        out.append(Wm)
    return out


def write_scene(root, folder, tag, n_views=6, H=24, W=32, with_points=True, seed=0):
    """Writes the scene and returns the raw frames, (H,W,3) uint8 each, in the order of the sorted file names.  The files are written out
    of order and one sits in a sub-directory; a file with another extension is ignored by the loaders."""
    rng = np.random.RandomState(seed)
    img_dir = os.path.join(str(root), folder, tag, 'image')
    os.makedirs(os.path.join(img_dir, 'sub'), exist_ok=True)
    names = [f'{i:06d}.png' for i in range(n_views - 1)] + [os.path.join('sub', '000000.png')]     # 'sub/...' sorts behind the digits
    frames = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in names]
    for i in reversed(range(n_views)):
        Image.fromarray(frames[i], 'RGB').save(os.path.join(img_dir, names[i]))
    with open(os.path.join(img_dir, 'notes.txt'), 'w') as f:
        f.write('not an image\n')
    arrays = {}
    raw = (1200, 1600) if folder == 'DTU' else (576, 768)
    for i, Wm in enumerate(projection_matrices(n_views, *raw)):
        arrays[f'world_mat_{i}'], arrays[f'scale_mat_{i}'] = Wm, SCALE
        arrays[f'world_mat_inv_{i}'] = np.linalg.inv(Wm)
    np.savez(os.path.join(str(root), folder, tag, 'cameras.npz'), **arrays)
    if with_points and folder == 'DTU':
        pts = np.random.RandomState(seed + 1).randn(40, 3) * 100 + SCALE[:3, 3]
        d = os.path.join(str(root), 'DTU', 'Points', 'stl')
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, 'stl{}_total.ply'.format(tag.replace('scan', '').zfill(3))), 'w') as f:
            f.write('ply\nformat ascii 1.0\nelement vertex 40\nproperty float x\nproperty float y\nproperty float z\nend_header\n')
            for p in pts:
                f.write('%r %r %r\n' % (float(np.float32(p[0])), float(np.float32(p[1])), float(np.float32(p[2]))))
    return frames
