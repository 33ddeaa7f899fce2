"""Scene ingest: a DTU / BlendedMVS scene directory, or a capture of one's own with a transforms.json (CustomScene), on disk -> the
resident `views` dict Trainer(cfg, model, views) consumes, the (inp, labels) loaders the evaluations walk, and the reference's YAML configs.  Restates src/dataset/dtu.py, src/dataset/bmvs.py,
src/dataset/__init__.py and utils.load_yaml of the reference.

The reference resizes every image on the host, per item, with Compose([Resize(img_size), ToTensor()]) on a PIL image.  Here each file is
decoded once on the host (PIL), the raw uint8 frames are stacked in pinned memory and uploaded in chunks -- 3 bytes per raw pixel --, and
the targets of the whole chunk are made on the device in one launch of ops.resample_u8, which reproduces Pillow's resample and ToTensor bit
for bit (csrc/resample_math.h).  The frames stay resident; `keep_raw` keeps the raw stack too, so another img_size needs no second decode."""
from copy import deepcopy
from pathlib import Path

import numpy as np
import torch

from . import ops
from .cameras import load_idr_cameras

IMG_EXTENSIONS = ['jpeg', 'jpg', 'JPG', 'png', 'ppm', 'JPEG']              # utils/image.py:18
N_LABEL_POINTS = int(1e5)                                                   # dtu.py:66


# ---- configs (utils/__init__.py:47-86) ----------------------------------------------------------------------------------------------------
def update_recursive(dict1, dict2):
    """dict1 updated in place with the entries of dict2, dictionaries merged key by key."""
    for k, v in dict2.items():
        if k not in dict1:
            dict1[k] = dict()
        if isinstance(v, dict):
            update_recursive(dict1[k], v)
        else:
            dict1[k] = v


def load_config(path, default_path=None):
    """The reference's load_yaml: the defaults -- default_path, or the `default.yml` next to `path` where there is one -- updated
    recursively with the file itself."""
    import yaml
    path = Path(path)
    if not path.exists():
        raise FileNotFoundError(f'{path.absolute()} does not exist')
    with open(path) as fp:
        cfg_s = yaml.load(fp, Loader=yaml.FullLoader)
    cfg = {}
    if default_path is not None:
        if not Path(default_path).exists():
            raise FileNotFoundError(f'{Path(default_path).absolute()} does not exist')
        with open(default_path) as fp:
            cfg = yaml.load(fp, Loader=yaml.FullLoader)
    elif (path.parent / 'default.yml').exists():
        with open(path.parent / 'default.yml') as fp:
            cfg = yaml.load(fp, Loader=yaml.FullLoader)
    update_recursive(cfg, cfg_s or {})
    return cfg


# ---- files ------------------------------------------------------------------------------------------------------------------------------------
def get_files_from(dir_path, valid_extensions=IMG_EXTENSIONS, recursive=True, sort=True):
    """utils/__init__.py:32-44: the files under dir_path with one of the extensions, as absolute paths, sorted as paths sort."""
    path = Path(dir_path)
    if not path.exists():
        raise FileNotFoundError(f'{path.absolute()} does not exist')
    files = [f.absolute() for f in path.glob('**/*' if recursive else '*') if f.is_file()]
    exts = ['.{}'.format(e) if not e.startswith('.') else e for e in valid_extensions]
    files = [f for f in files if f.suffix in exts]
    return sorted(files) if sort else files


def decode_mask(path, size):
    """One mask file -> (H,W) uint8, 255 where Image.open(f).convert('L') is not zero and 0 elsewhere; size (H,W): the frame's, which the
    mask must have."""
    from PIL import Image
    with Image.open(path) as im:
        a = np.array(im.convert('L'))
    if a.shape != tuple(size):
        raise ValueError(f'{path}: a mask of {a.shape}, its frame is {tuple(size)}')
    return np.where(a != 0, 255, 0).astype(np.uint8)


def decode_rgb(path):
    """One image file -> (H,W,3) uint8, as Image.open(f).convert('RGB') reads it (dtu.py:63)."""
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert('RGB'))


class ImageStore:
    """The decoded frames of one scene directory, resident on one device: (N,3,H,W) fp32 targets of one img_size, filled file by file the
    first time a view is asked for, and optionally the raw (N,Hraw,Wraw,3) uint8 stack.  The three splits of a scene share one store.
    prepare: a callable from the uploaded (n,Hraw,Wraw,3) uint8 chunk on the device to a chunk of the same kind, applied before the
    resize (a custom scene's lens rectification); the raw stack keeps what came off disk.
    Validity masks: mask_files -- one entry per frame, a file or None (all valid) -- and / or valid -- one (Hraw,Wraw) uint8
    map of 0 / 255 for every frame, or a callable from the device to it (a lens map: ops.lens_valid_u8) -- make the store keep
    masks (N,1,h,w) fp32 of 0 / 1 beside the targets.  A decoded mask (decode_mask: 0 / 255) is expanded to 3 channels, goes through
    mask_prepare (default: prepare, the frames' own warp), is ANDed with valid and resized by the kernel that resizes the frames
    (ops.resample_u8, out='u8'); a training pixel is valid where that byte is 255, that is where its whole footprint is valid.  The
    existing kernels do the warp and the resize: three identical channels on a once-per-scene pass are accepted for that.
    per_frame=True (a scene whose frames have a camera each): prepare and mask_prepare are called with the chunk AND the file
    indices of its frames, prepare(raw, ids), and valid is one map per frame, (N,Hraw,Wraw) or a callable from the device to that."""

    def __init__(self, files, img_size, chunk=16, prepare=None, mask_files=None, mask_prepare=None, valid=None, per_frame=False):
        self.files, self.img_size, self.chunk, self.prepare = list(files), tuple(img_size), chunk, prepare
        self.per_frame = bool(per_frame)
        self.mask_files = None if mask_files is None else list(mask_files)
        if self.mask_files is not None and len(self.mask_files) != len(self.files):
            raise ValueError(f'{len(self.mask_files)} masks for {len(self.files)} frames')
        self.mask_prepare = prepare if mask_prepare is None else mask_prepare
        self.valid, self.has_masks = valid, mask_files is not None or valid is not None
        self.masks = None
        self.device = self.imgs = self.raw = None
        self.have, self.have_raw = np.zeros(len(self.files), bool), np.zeros(len(self.files), bool)

    def get(self, device, ids, keep_raw=False, chunk=None):
        device = torch.device(device)
        if self.device is not None and self.device != device:
            raise RuntimeError(f'the frames of this scene are resident on {self.device}: one store serves one device')
        ids = [int(i) for i in ids]
        todo = sorted(set(i for i in ids if not self.have[i] or (keep_raw and not self.have_raw[i])))
        chunk = chunk or self.chunk
        pinned, events = [None, None], [None, None]
        for b, c0 in enumerate(range(0, len(todo), chunk)):
            part = todo[c0:c0 + chunk]
            first = decode_rgb(self.files[part[0]])
            if self.device is None:
                self.device, self.raw_size = device, first.shape[:2]
                self.imgs = torch.empty(len(self.files), 3, *self.img_size, dtype=torch.float32, device=device)
                if self.has_masks:
                    self.masks = torch.empty(len(self.files), 1, *self.img_size, dtype=torch.float32, device=device)
                    if callable(self.valid):
                        self.valid = self.valid(device)
                    if self.valid is not None:
                        self.valid = torch.as_tensor(self.valid, dtype=torch.uint8).to(device)
                        want = ((len(self.files),) if self.per_frame else ()) + tuple(self.raw_size)
                        if tuple(self.valid.shape) != want:
                            raise ValueError(f'valid: {tuple(self.valid.shape)}, the frames are {want}')
            if keep_raw and self.raw is None:
                self.raw = torch.empty(len(self.files), *self.raw_size, 3, dtype=torch.uint8, device=device)
            slot = b % 2                                         # two staging buffers: the next chunk is decoded while this one is copied
            if pinned[slot] is None:
                pinned[slot] = torch.empty(chunk, *self.raw_size, 3, dtype=torch.uint8)
                if device.type == 'cuda':
                    pinned[slot] = pinned[slot].pin_memory()
            elif events[slot] is not None:
                events[slot].synchronize()
            buf = pinned[slot][:len(part)]
            for j, i in enumerate(part):
                a = first if j == 0 else decode_rgb(self.files[i])
                if a.shape[:2] != self.raw_size:
                    raise ValueError(f'{self.files[i]}: {a.shape[:2]}, the other frames of the scene are {self.raw_size}')
                buf[j] = torch.from_numpy(a)
            raw = buf.to(device, non_blocking=True)
            if device.type == 'cuda':
                events[slot] = torch.cuda.Event()
                events[slot].record(torch.cuda.current_stream(device))
            idx = torch.as_tensor(part, device=device)
            self.imgs[idx] = ops.resample_u8(self._warp(self.prepare, raw, part), self.img_size, out='f32')
            if self.has_masks:
                self.masks[idx] = self._masks_of(part, device)
            if self.raw is not None:
                self.raw[idx] = raw
                self.have_raw[part] = True
            self.have[part] = True
        idx = torch.as_tensor(ids, dtype=torch.long, device=device)
        return self.imgs[idx], (self.raw[idx] if keep_raw else None)

    def _warp(self, prepare, chunk, part):
        if prepare is None:
            return chunk
        return prepare(chunk, part) if self.per_frame else prepare(chunk)

    def _masks_of(self, part, device):
        """(n,1,h,w) fp32 masks of the frames `part` (file indices), made on the device as the class docstring says."""
        H, W = self.raw_size
        m = torch.full((len(part), H, W, 3), 255, dtype=torch.uint8)
        if self.mask_files is not None:
            for j, i in enumerate(part):
                if self.mask_files[i] is not None:
                    m[j] = torch.from_numpy(decode_mask(self.mask_files[i], (H, W)))[:, :, None]
        m = m.to(device)
        m = self._warp(self.mask_prepare, m, part)
        if self.valid is not None:
            m = m & (self.valid[torch.as_tensor(part, device=device)][:, :, :, None] if self.per_frame else self.valid[None, :, :, None])
        small = ops.resample_u8(m.contiguous(), self.img_size, out='u8')
        return (small[..., 0] == 255).to(torch.float32)[:, None]

    def get_masks(self, ids):
        """masks (V,1,h,w) of the file indices `ids`, after get() has made them."""
        return self.masks[torch.as_tensor([int(i) for i in ids], dtype=torch.long, device=self.device)]


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------------
class _Scene:
    """What the two dataset kinds share (dtu.py / bmvs.py): files, cameras, view ids, resident views and loaders."""
    name, folder, raw_img_size, n_channels = None, None, None, 3

    def __init__(self, root, tag, img_size, split, view_ids=None, store=None, masks=False):
        self.split, self.tag = split, tag
        self.data_path = Path(root) / self.folder / tag / 'image'
        self.input_files = get_files_from(self.data_path, IMG_EXTENSIONS, recursive=True, sort=True)
        self.img_size = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)
        N = len(self.input_files)
        self.view_ids = self._split_ids(N, list(range(N)) if view_ids is None else list(deepcopy(view_ids)))
        cams = load_idr_cameras(self.data_path.parent / 'cameras.npz', self.raw_img_size, n_views=N)
        self.K, self.R, self.T, self.scale_mat = cams['K'], cams['R'], cams['T'], cams['scale_mat']
        self.pc_gt = torch.zeros(1, 3)
        # masks=True: the IDR layout's <tag>/mask/* beside image/, in sorted order, one per image
        self.mask_files = None
        if masks:
            self.mask_files = get_files_from(self.data_path.parent / 'mask', IMG_EXTENSIONS, recursive=True, sort=True)
            if len(self.mask_files) != N:
                raise ValueError(f"{self.data_path.parent / 'mask'}: {len(self.mask_files)} masks for {N} images")
        if store is not None and ([str(f) for f in store.files] != [str(f) for f in self.input_files] or store.img_size != self.img_size
                                  or store.has_masks != bool(masks)):
            raise ValueError('store: made for other files, another img_size or other masks')
        self.store = store if store is not None else ImageStore(self.input_files, self.img_size, mask_files=self.mask_files)

    def _split_ids(self, N, view_ids):
        return view_ids

    def __len__(self):
        return len(self.view_ids)

    def ids(self):
        """The file index of every item of this split, in its order."""
        return self.view_ids[:len(self)]

    def views(self, device, keep_raw=False, chunk=None):
        """{'imgs' (V,3,H,W) fp32, 'K' (V,4,4), 'R' (V,3,3), 'T' (V,3)} of this split, in its order, resident on `device`; with keep_raw
        also 'raw' (V,Hraw,Wraw,3) uint8; for a scene with validity masks also 'masks' (V,1,H,W) fp32 of 0 / 1."""
        ids = self.ids()
        imgs, raw = self.store.get(device, ids, keep_raw=keep_raw, chunk=chunk)
        out = {'imgs': imgs, 'K': self.K[ids].to(device), 'R': self.R[ids].to(device), 'T': self.T[ids].to(device)}
        if self.store.has_masks:
            out['masks'] = self.store.get_masks(ids)
        if keep_raw:
            out['raw'] = raw
        return out

    def loader(self, batch_size, device):
        return SceneLoader(self, batch_size, device)


class SceneLoader:
    """A re-walkable iterable of (inp, labels) over a scene's views in the split's order, batch_size at a time, like the reference's
    DataLoader without shuffling (src/dataset/__init__.py:23): inp = {'imgs','K','R','T'} on the device, labels = {'points' (B,P,3)}, for
    every view its own draw of at most 1e5 ground-truth points (dtu.py:66-68).  `batch_size` and `dataset` as a DataLoader has them."""

    def __init__(self, scene, batch_size, device):
        self.dataset, self.batch_size, self.device = scene, int(batch_size), device

    def __len__(self):
        return -(-len(self.dataset) // self.batch_size)

    def __iter__(self):
        views = self.dataset.views(self.device)
        pc = self.dataset.pc_gt
        for a in range(0, len(self.dataset), self.batch_size):
            inp = {k: v[a:a + self.batch_size] for k, v in views.items()}
            B = inp['imgs'].shape[0]
            points = torch.stack([pc[torch.randperm(len(pc))[:N_LABEL_POINTS]] for _ in range(B)])
            yield inp, {'points': points}


class DTUScene(_Scene):
    """src/dataset/dtu.py: <root>/DTU/<tag>/image/*, <root>/DTU/<tag>/cameras.npz, <root>/DTU/Points/stl/stlNNN_total.ply.  The test split
    takes every view; val and test are shuffled under the seed len(split + tag).  pc_gt: the ground-truth points in the normalised frame
    (a (1,3) zero tensor where the scan's file is absent), scale_mat: the matrix back to the DTU frame."""
    name, folder, raw_img_size = 'dtu', 'DTU', (1200, 1600)

    def __init__(self, root, tag, img_size, split, view_ids=None, store=None, masks=False):
        super().__init__(root, tag, img_size, split, view_ids=view_ids, store=store, masks=masks)
        ply = self.data_path.parent.parent / 'Points' / 'stl' / 'stl{}_total.ply'.format(tag.replace('scan', '').zfill(3))
        if ply.exists():
            from .eval3d import read_ply_points
            points = torch.from_numpy(np.asarray(read_ply_points(ply))).float()
            scale_inv = self.scale_mat.inverse()
            self.pc_gt = points @ scale_inv[:3, :3] + scale_inv[:3, 3]           # dtu.py:49-50

    def _split_ids(self, N, view_ids):
        ids = list(range(N)) if self.split == 'test' else view_ids
        if self.split != 'train':
            np.random.RandomState(len(self.split + self.tag)).shuffle(ids)      # use_seed(len(split + tag)): np.random.seed, then shuffle
        return ids


class BMVSScene(_Scene):
    """src/dataset/bmvs.py: <root>/BlendedMVS/<tag>/image/*, cameras.npz next to image/.  No shuffling; val holds the first 5 views, test
    the first 10."""
    name, folder, raw_img_size = 'bmvs', 'BlendedMVS', (576, 768)

    def __len__(self):
        n = len(self.view_ids)
        return n if self.split == 'train' else min(5 if self.split == 'val' else 10, n)


# ---- custom scenes: a transforms.json capture ----------------------------------------------------------------------------------------------
LENS_COEFFS = ('k1', 'k2', 'k3', 'k4', 'p1', 'p2')
CAMERA_KEYS = ('fl_x', 'fl_y', 'cx', 'cy', 'w', 'h') + LENS_COEFFS
TRAIN_SPLIT_FRACTION = 0.9                                                  # Nerfstudio's default split of a capture


def lens_source(H, W, intr, dist, zoom, i, j, model=0, target=None):
    """The map of csrc/lens_math.h in fp64: the source INDEX coordinates (u, v) of the output pixels (i, j) (arrays) of an H x W frame
    rectified with the focal lengths zoom * (fx, fy).  intr = (fx, fy, cx, cy), dist = (k1, k2, k3, k4, p1, p2).  model: 0 OpenCV's
    radial-tangential lens, 1 its fisheye lens (k1..k4; p1, p2 are not read).  target = (fx0, fy0, cx0, cy0): the pinhole camera the
    output pixels belong to, zoomed by `zoom` (a scene of per-frame cameras: common_pinhole); None: the source's own."""
    fx, fy, cx, cy = [float(v) for v in intr]
    k1, k2, k3, k4, p1, p2 = [float(v) for v in dist]
    fx0, fy0, cx0, cy0 = (fx, fy, cx, cy) if target is None else [float(v) for v in target]
    x = (np.asarray(j, np.float64) + 0.5 - cx0) / (zoom * fx0)
    y = (np.asarray(i, np.float64) + 0.5 - cy0) / (zoom * fy0)
    r2 = x * x + y * y
    if model == 1:
        r = np.sqrt(r2)
        th = np.arctan(r)
        t2 = th * th
        td = th * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
        s = np.where(r2 == 0, 1.0, td / np.where(r2 == 0, 1.0, r))
        return x * s * fx + cx - 0.5, y * s * fy + cy - 0.5
    if model != 0:
        raise ValueError(f'model: 0 (radial-tangential) or 1 (fisheye), got {model!r}')
    d = 1 + r2 * (k1 + r2 * (k2 + r2 * (k3 + r2 * k4)))
    xd = x * d + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * d + 2 * p2 * x * y + p1 * (r2 + 2 * y * y)
    return xd * fx + cx - 0.5, yd * fy + cy - 0.5


def lens_zoom(H, W, intr, dist):
    """The smallest zoom s >= 1 at which every border pixel centre of the rectified H x W frame reads inside the source frame
    (0 <= u <= W - 1, 0 <= v <= H - 1): no black or smeared border reaches the loss, which has no mask.  1.0 where that holds at s = 1;
    otherwise [1, 2] is bisected 40 times and the upper end returned.  ValueError where s = 2 does not suffice."""
    i, j = _border(H, W)

    def inside(s):
        u, v = lens_source(H, W, intr, dist, s, i, j)
        return bool(np.all((u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)))           # (False for a NaN)

    return _smallest_zoom(inside, f'lens_zoom: the border of a {H}x{W} frame leaves the source even at a zoom of 2 (intr={tuple(intr)}, '
                                  f'dist={tuple(dist)})')


def _border(H, W):
    """(i, j) of the border pixels of an H x W frame."""
    i = np.concatenate([np.zeros(W), np.full(W, H - 1), np.arange(H), np.arange(H)])
    j = np.concatenate([np.arange(W), np.arange(W), np.zeros(H), np.full(H, W - 1)])
    return i, j


def _smallest_zoom(inside, refusal):
    """The bisection of lens_zoom and rectify_zoom: 1.0 where inside(1.0), ValueError(refusal) where not inside(2.0)."""
    if inside(1.0):
        return 1.0
    if not inside(2.0):
        raise ValueError(refusal)
    lo, hi = 1.0, 2.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if inside(mid):
            hi = mid
        else:
            lo = mid
    return hi


def common_pinhole(intrs):
    """The pinhole camera (fx0, fy0, cx0, cy0) that the frames of a capture with per-frame intrinsics (N,4) are rectified into, before any
    zoom: the median of each component over the frames.  Equal cameras give exactly the camera they share; one odd frame (a refocus, a
    second body of a rig) does not move it."""
    intrs = np.asarray(intrs, dtype=np.float64).reshape(-1, 4)
    if len(intrs) == 0:
        raise ValueError('common_pinhole: no cameras')
    return tuple(float(v) for v in np.median(intrs, axis=0))


def rectify_zoom(H, W, intrs, dists, models, target):
    """lens_zoom for per-frame cameras: the smallest s >= 1 at which every border pixel centre of the H x W frame of the pinhole `target`
    (fx0, fy0, cx0, cy0), zoomed by s, reads inside the source frame of EVERY camera (intrs (N,4), dists (N,6), models (N,)).  The same
    bisection; ValueError where s = 2 does not suffice."""
    i, j = _border(H, W)
    cams = sorted(set((tuple(float(v) for v in a), tuple(float(v) for v in d), int(m)) for a, d, m in zip(intrs, dists, models)))

    def inside(s):
        for intr, dist, model in cams:
            u, v = lens_source(H, W, intr, dist, s, i, j, model=model, target=target)
            if not bool(np.all((u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1))):
                return False
        return True

    return _smallest_zoom(inside, f'rectify_zoom: the border of a {H}x{W} frame of the common camera {tuple(target)} leaves the source of one '
                                  f"of the {len(cams)} distinct cameras even at a zoom of 2: lens='mask' rectifies without a zoom and masks "
                                  'what a frame cannot fill')


def _rotation_to_z(up):
    """The Rodrigues rotation that takes the unit vector `up` to (0, 0, 1): the identity where they coincide, a half turn about an axis
    orthogonal to `up` where they are opposite."""
    z = np.array([0.0, 0.0, 1.0])
    v, c = np.cross(up, z), float(up @ z)
    if c > 1 - 1e-12:
        return np.eye(3)
    if c < -1 + 1e-12:
        a = np.cross(up, np.eye(3)[int(np.argmin(np.abs(up)))])
        a /= np.linalg.norm(a)
        return 2 * np.outer(a, a) - np.eye(3)
    vx = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + vx + vx @ vx * ((1 - c) / float(v @ v))


def normalize_poses(c2w, method='poses'):
    """(N,4,4) camera-to-world matrices -> (the normalised ones, F): F (4,4) is the similarity from the file's frame to the normalised
    one, the rigid part applied to the whole matrices and the scale to their translations.  'poses' is Nerfstudio's default recipe: the
    mean camera up goes to +z, the mean camera position to the origin, the largest |coordinate| of a camera position to 1.  'none': the
    identity."""
    c2w = np.array(c2w, dtype=np.float64)
    F = np.eye(4)
    if method == 'none':
        return c2w, F
    if method != 'poses':
        raise ValueError(f"normalize: 'poses' or 'none', got {method!r}")
    up = c2w[:, :3, 1].mean(0)
    rot = _rotation_to_z(up / np.linalg.norm(up))
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = rot, -rot @ c2w[:, :3, 3].mean(0)
    c2w = M @ c2w
    scale = 1.0 / float(np.abs(c2w[:, :3, 3]).max())
    c2w[:, :3, 3] *= scale
    F = np.diag([scale, scale, scale, 1.0]) @ M
    return c2w, F


CLOUD_KEYS = ('source', 'unit', 'range', 'grid', 'bound', 'stride', 'edge', 'min_count')
CLOUD_DEFAULTS = {'unit': None, 'range': (0.1, 10.0), 'grid': 128, 'bound': 2.0, 'stride': 1, 'edge': 0.05, 'min_count': 2}


def cloud_options(cloud):
    """The `cloud` argument of CustomScene -> None for 'file' (the capture's .ply), else the options of the depth cloud with their
    defaults filled in: 'depth', or a mapping of CLOUD_KEYS {source: depth, unit, range, grid, bound, stride, edge, min_count}.
    unit: metres per depth step (None: the file's depth_unit_scale_factor, else 1e-3); range: (near, far) in metres; grid: cells per axis;
    bound: the half-size of the cube around the origin of the normalised frame that is gridded.  The default bound of 2.0 is a design
    choice, not a measured value: the cameras are normalised into [-1, 1]^3, and what lies more than one rig extent outside them is not
    what the plane and block fits are after.  stride: every stride-th depth row and column; edge: the relative depth jump to a
    4-neighbour above which a sample counts as a mixed pixel and is dropped (0: off); min_count: samples a cell needs to give a point."""
    from collections.abc import Mapping
    if isinstance(cloud, str) and cloud == 'file':
        return None
    if isinstance(cloud, str) and cloud == 'depth':
        cloud = {}
    elif isinstance(cloud, Mapping):
        bad = [k for k in cloud if k not in CLOUD_KEYS]
        if bad:
            raise ValueError(f"cloud: '{bad[0]}' is not one of {', '.join(CLOUD_KEYS)}")
        source = cloud.get('source', 'depth')
        if source == 'file':
            return None
        if source != 'depth':
            raise ValueError(f"cloud.source: 'file' or 'depth', got {source!r}")
    else:
        raise ValueError(f"cloud: 'file', 'depth' or a mapping of {', '.join(CLOUD_KEYS)}, got {cloud!r}")
    o = dict(CLOUD_DEFAULTS)
    o.update({k: v for k, v in cloud.items() if k != 'source'})
    o['range'] = tuple(float(v) for v in o['range'])
    if len(o['range']) != 2 or not 0 < o['range'][0] < o['range'][1]:
        raise ValueError(f"cloud.range: (near, far) in metres with 0 < near < far, got {o['range']}")
    if o['unit'] is not None and not float(o['unit']) > 0:
        raise ValueError(f"cloud.unit: metres per depth step, positive; got {o['unit']}")
    if not float(o['bound']) > 0:
        raise ValueError(f"cloud.bound: positive, got {o['bound']}")
    return o


def read_depth_png(path):
    """A 16-bit single-channel PNG -> (H,W) uint16."""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.ndim != 2 or a.dtype.kind not in 'iu' or int(a.min()) < 0 or int(a.max()) > 65535:
        raise ValueError(f'{path}: a single-channel 16-bit PNG is expected, got an array of {a.dtype} {a.shape}')
    return a.astype(np.uint16)


class CustomScene(_Scene):
    """A capture of one's own: <root>/custom/<tag>/transforms.json -- top-level fl_x, fl_y, cx, cy, w, h, optional k1..k4, p1, p2 and
    camera_model (OPENCV or PINHOLE; a PINHOLE file's coefficients are not read), and per frame a file_path relative to the json and an
    OpenGL camera-to-world transform_matrix -- as ns-process-data, instant-ngp exporters and COLMAP converters write it.  Restates
    src/dataset/nerfstudio.py:35-77 without the `nerfstudio` package, and rectifies the frames on the device (ops.undistort_u8, zoomed so
    that every pixel is valid: lens_zoom) where the reference trains a pinhole renderer on the distorted ones; undistort=False is the
    reference's behaviour.  The train split holds ceil(0.9 N) frames spread evenly, test the others (shuffled under the seed len(tag)),
    val none.  scale_mat: the normalised frame back to the file's; pc_gt: the points of `ply_file_path` or points.ply, normalised.
    masks=True reads each frame's `mask_path` (relative to the json, as Nerfstudio's exporters write it; a frame without one is all
    valid) into views()['masks']; lens='mask' rectifies at zoom 1 and masks what reads outside the source frame (ops.lens_valid_u8)
    instead of cropping it away with lens_zoom ('crop'), and never raises lens_zoom's ValueError.
    cameras='per_frame'  reads fl_x, fl_y, cx, cy, k1..k4, p1, p2 frame by frame (the frame's own value where it has one,
    else the top level's; w, h must still agree) and accepts camera_model OPENCV_FISHEYE: every frame is warped from its own camera into
    ONE pinhole (ops.rectify_u8) -- intr = common_pinhole(intrs), zoomed by rectify_zoom under 'crop'; under lens='mask' at zoom 1 with
    a validity map per frame --, so K stays one matrix.  intrs (N,4), dists (N,6), models (N,) keep the frames' cameras; dist is what they
    share, None where they differ.  'shared', the default, refuses both kinds of capture.
    cloud: where cloud(), world_frame and block_init take their points from.  'file', the default: the .ply above.
    'depth', or a mapping (cloud_options has the keys and defaults): from the capture's depth maps -- each frame's `depth_file_path`
    (relative to the json, a 16-bit PNG in steps of `depth_unit_scale_factor` metres, of one size that may differ from the images'; a frame
    without one contributes nothing), every sample unprojected through the TRUE lens of its frame (also under undistort=False and under
    cameras='shared') and its normalised pose, and reduced to one point per cell of a grid (ops.depth_cloud on a device, ops.depth_cloud_host
    without one: the same bytes).  Every frame with a depth map contributes, whichever split it is in.  pc_gt stays the .ply: a depth
    cloud is no ground truth."""
    name, folder = 'custom', 'custom'

    def __init__(self, root, tag, split, downscale_factor=1, img_size=None, undistort=True, normalize='poses', view_ids=None, store=None,
                 masks=False, lens='crop', cameras='shared', cloud='file'):
        import json
        if cameras not in ('shared', 'per_frame'):
            raise ValueError(f"cameras: 'shared' or 'per_frame', got {cameras!r}")
        self.cloud_options = cloud_options(cloud)
        per_frame = cameras == 'per_frame'
        self.cameras = cameras
        self.split, self.tag = split, tag
        self.data_path = Path(root) / self.folder / tag
        path = self.data_path / 'transforms.json'
        if not path.exists():
            raise FileNotFoundError(f'{path.absolute()} does not exist')
        with open(path) as fp:
            meta = json.load(fp)
        frames = meta.get('frames') or []
        if not frames:
            raise ValueError(f'{path}: no frames')
        model = meta.get('camera_model')
        if per_frame and model not in (None, 'OPENCV', 'OPENCV_FISHEYE', 'PINHOLE'):
            raise NotImplementedError(f"{path}: camera_model '{model}' is not supported (OPENCV, OPENCV_FISHEYE and PINHOLE are)")
        if not per_frame and model not in (None, 'OPENCV', 'PINHOLE'):
            hint = " (OPENCV_FISHEYE is under cameras='per_frame')" if model == 'OPENCV_FISHEYE' else ''
            raise NotImplementedError(f"{path}: camera_model '{model}' is not supported (OPENCV and PINHOLE are){hint}")
        cam, each = {}, {}
        for k in CAMERA_KEYS:
            given = [f[k] for f in frames if k in f]
            if per_frame and k not in ('w', 'h'):
                # the frame's own value where it has one, else the top level's; a coefficient nobody gives is 0
                if k not in meta and len(given) != len(frames) and k not in LENS_COEFFS:
                    raise ValueError(f"{path}: '{k}' is neither given at the top level nor on every frame")
                each[k] = [float(f[k]) if k in f else float(meta.get(k, 0.0)) for f in frames]
                continue
            if k in meta:
                cam[k] = meta[k]
            elif len(given) == len(frames):
                cam[k] = given[0]
            elif given or k not in LENS_COEFFS:
                raise ValueError(f"{path}: '{k}' is neither given at the top level nor on every frame")
            else:
                cam[k] = 0.0
            if any(float(v) != float(cam[k]) for v in given):
                raise NotImplementedError(f"{path}: per-frame intrinsics differ ('{k}'): the model keeps one K for all views"
                                          + ('' if k in ('w', 'h') else " (cameras='per_frame' rectifies every frame into one K)"))
        h, w = int(cam['h']), int(cam['w'])
        self.raw_img_size = (h, w)
        if per_frame:
            # a camera per frame; intr is the pinhole they are all rectified into, dist what they share (None where they do not)
            self.intrs = np.array([each[k] for k in ('fl_x', 'fl_y', 'cx', 'cy')], dtype=np.float64).T
            self.dists = np.array([each[k] for k in LENS_COEFFS], dtype=np.float64).T * (0.0 if model == 'PINHOLE' else 1.0)
            self.models = np.full(len(frames), ops.LENS_MODELS[model or 'OPENCV'], dtype=np.int64)
            self.intr = common_pinhole(self.intrs)
            differ = bool((self.intrs != self.intrs[0]).any() or (self.dists != self.dists[0]).any())
            self.dist = None if (self.dists != self.dists[0]).any() else tuple(float(v) for v in self.dists[0])
        else:
            self.intr = tuple(float(cam[k]) for k in ('fl_x', 'fl_y', 'cx', 'cy'))
            self.dist = tuple(0.0 if model == 'PINHOLE' else float(cam[k]) for k in LENS_COEFFS)

        self.input_files = [self._frame_file(path.parent, f['file_path']) for f in frames]
        from PIL import Image
        for f in self.input_files:
            with Image.open(f) as im:
                if im.size != (w, h):
                    raise ValueError(f"{f}: {im.size[::-1]}, transforms.json says {(h, w)}")
        if img_size is not None:
            self.img_size = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)
        else:
            self.img_size = tuple(round(x / downscale_factor) for x in self.raw_img_size)           # nerfstudio.py:55

        N = len(frames)
        n_train = int(np.ceil(TRAIN_SPLIT_FRACTION * N))
        train = np.linspace(0, N - 1, n_train).astype(int).tolist()
        if split == 'train':
            self.view_ids = train if view_ids is None else list(deepcopy(view_ids))
        elif split == 'test':
            self.view_ids = [i for i in range(N) if i not in set(train)]
            np.random.RandomState(len(tag)).shuffle(self.view_ids)                                  # nerfstudio.py:46-48
        else:
            self.view_ids = []

        if lens not in ('crop', 'mask'):
            raise ValueError(f"lens: 'crop' or 'mask', got {lens!r}")
        if per_frame:
            if differ and not undistort:
                raise ValueError(f"{path}: undistort=False with per-frame cameras that differ: there is no single K to train on")
            # a fisheye frame is no pinhole frame even with every coefficient at 0
            rectify = bool(undistort) and bool(differ or (self.models != 0).any() or (self.dists != 0).any())
            lens_mask = rectify and lens == 'mask'
            self.zoom = rectify_zoom(h, w, self.intrs, self.dists, self.models, self.intr) if (rectify and not lens_mask) else 1.0
            table, target = ops.lens_table(self.intrs, self.dists, self.models), ops.lens_target(self.intr, self.zoom)
            self.prepare = (lambda raw, ids: ops.rectify_u8(raw, table[list(ids)], target)) if rectify else None
            valid = (lambda device: ops.rectify_valid_u8(h, w, table, target, device=device)) if lens_mask else None
        else:
            rectify = bool(undistort) and any(c != 0 for c in self.dist)
            lens_mask = rectify and lens == 'mask'
            self.zoom = lens_zoom(h, w, self.intr, self.dist) if (rectify and not lens_mask) else 1.0
            intr, dist, zoom = self.intr, self.dist, self.zoom
            self.prepare = (lambda raw: ops.undistort_u8(raw, intr, dist, zoom)) if rectify else None
            valid = (lambda device: ops.lens_valid_u8(h, w, intr, dist, 1.0, device=device)) if lens_mask else None
        self.mask_files = None
        if masks:
            self.mask_files = [self._frame_file(path.parent, f['mask_path']) if f.get('mask_path') else None for f in frames]
        has_masks = self.mask_files is not None or valid is not None

        c2w = np.stack([np.asarray(f['transform_matrix'], dtype=np.float64)[:4, :4] for f in frames])
        if c2w.shape[1] == 3:
            c2w = np.concatenate([c2w, np.tile(np.array([[[0.0, 0.0, 0.0, 1.0]]]), (N, 1, 1))], 1)
        parser = path.parent / 'dataparser_transforms.json'
        if parser.exists():
            with open(parser) as fp:
                dp = json.load(fp)
            M = np.eye(4)
            M[:3, :4] = np.asarray(dp['transform'], dtype=np.float64)[:3, :4]
            scale = float(dp.get('scale', 1.0))
            c2w = M @ c2w
            c2w[:, :3, 3] *= scale
            F = np.diag([scale, scale, scale, 1.0]) @ M
        else:
            c2w, F = normalize_poses(c2w, normalize)
        self.cam2world = torch.from_numpy(c2w).float()
        self.scale_mat = torch.from_numpy(np.linalg.inv(F)).float()

        # nerfstudio.py:59-77
        wh = np.array([w, h], dtype=np.float64)
        scale = wh.min() / 2.0
        p0 = -(np.array(self.intr[2:]) - wh / 2.0) / scale
        focal = self.zoom * np.array(self.intr[:2]) / scale
        K = np.array([[focal[0], 0, p0[0], 0], [0, focal[1], p0[1], 0], [0, 0, 0, 1], [0, 0, 1, 0]])
        self.K = torch.from_numpy(K).float().expand(N, -1, -1)
        w2c = np.linalg.inv(c2w)
        flip = np.array([-1.0, 1.0, -1.0])
        self.R = torch.from_numpy(w2c[:, :3, :3].transpose(0, 2, 1) * flip).float()
        self.T = torch.from_numpy(w2c[:, :3, 3] * flip).float()

        self.pc_gt = torch.zeros(1, 3)
        ply = path.parent / meta['ply_file_path'] if meta.get('ply_file_path') else path.parent / 'points.ply'
        self.ply_file = ply if ply.exists() else None
        if ply.exists():
            from .eval3d import read_ply_points
            points = np.asarray(read_ply_points(ply), dtype=np.float64)
            self.pc_gt = torch.from_numpy(points @ F[:3, :3].T + F[:3, 3]).float()

        self.cloud_info, self._clouds, self._depth = None, {}, None
        self.rays_info, self._rays = None, {}
        if self.cloud_options is not None:
            self._depth = self._depth_setup(path, meta, frames, c2w, F, (h, w))

        if store is not None and ([str(f) for f in store.files] != [str(f) for f in self.input_files] or store.img_size != self.img_size
                                  or (store.prepare is None) != (self.prepare is None) or store.has_masks != has_masks
                                  or store.per_frame != per_frame):
            raise ValueError('store: made for other files, another img_size, another lens treatment (or another `cameras` mode) or other masks')
        self.store = store if store is not None else ImageStore(self.input_files, self.img_size, prepare=self.prepare,
                                                                mask_files=self.mask_files, valid=valid, per_frame=per_frame)

    def world_frame(self, device=None, T_range=(1, 1, 1), **kw):
        """worldfit.estimate_world_frame on this capture's cloud and cameras (both in the normalised frame R, T live in) -> WorldFrame: the
        R_world, T_world and S_world of model.mesh.  device: where the plane fit runs (a cuda device: the HIP kernel).  ValueError for a
        capture without a cloud."""
        from .worldfit import estimate_world_frame
        if self._depth is None and self.ply_file is None:
            raise ValueError(f"'{self.tag}': no point cloud (ply_file_path of transforms.json, or points.ply next to it): the world frame is "
                             'fitted to the cloud, there is no fit without one')
        return estimate_world_frame(self.cloud(device), self.cam2world, T_range=T_range, **kw)

    def block_init(self, model, device=None, **kw):
        """model.init_blocks_from_points on this capture's cloud (in the normalised frame R, T live in): the blocks of `model` start at the
        clusters of the cloud -> worldfit.BlockInit.  device: where the clustering runs (a cuda device: the HIP kernel).  ValueError for a
        capture without a cloud."""
        if self._depth is None and self.ply_file is None:
            raise ValueError(f"'{self.tag}': no point cloud (ply_file_path of transforms.json, or points.ply next to it): the blocks are "
                             'fitted to the cloud, there is no fit without one')
        return model.init_blocks_from_points(self.cloud(device), **kw)

    def cloud(self, device=None):
        """The points the fits use, (M,3) float32 in the normalised frame R, T live in, on `device` (None: the CPU): the .ply's under
        cloud='file' (ValueError without one), the depth cloud under cloud='depth' -- built on first use, by the HIP kernel for a cuda
        device and in numpy otherwise, and kept per device.  cloud_info then holds {points, samples, outside, frames}: the cells that gave a
        point, the depth samples accumulated, those that fell outside the cube, and the frames with a depth map."""
        if self._depth is None:
            if self.ply_file is None:
                raise ValueError(f"'{self.tag}': no point cloud (ply_file_path of transforms.json, or points.ply next to it)")
            return self.pc_gt if device is None else self.pc_gt.to(device)
        dev = None if device is None else torch.device(device)
        host = dev is None or dev.type == 'cpu'
        key = 'cpu' if host else str(dev)
        if key not in self._clouds:
            D = self._depth
            depth = np.stack([read_depth_png(f) for f in D['files']])
            args = (depth, D['cams'], D['target'], D['poses'], D['lo'], D['hi'])
            kw = {k: D[k] for k in ('grid', 'd_range', 'stride', 'edge', 'min_count')}
            if host:
                pts, _, info = ops.depth_cloud_host(*args, return_info=True, **kw)
                pts = torch.from_numpy(pts)
            else:
                pts, _, info = ops.depth_cloud(*args, device=dev, return_info=True, **kw)
            self._clouds[key] = pts
            self.cloud_info = {'points': info[0], 'samples': info[1], 'outside': info[2], 'frames': len(D['files'])}
        pts = self._clouds[key]
        return pts if device is None else pts.to(device)

    def rays(self, device=None):
        """The capture's depth rays for the free-space term, in the normalised frame R, T live in, on `device` (None: the CPU)
        -> (ends (Nr,3) float32, frame (Nr,) int32, origins (Nf,3) float32): ray j runs from origins[frame[j]], the centre of the camera of the
        j-th ray's depth map (the pose rows' t), to ends[j], the measured surface point -- every depth sample that cloud() would take before
        its cube, with the same range, stride and edge rule (ops.depth_rays on a cuda device, ops.depth_rays_host otherwise; the valid
        records compacted once, order kept).  Built on first use and kept per device; rays_info then holds {rays, samples, frames}.  The
        rays use the capture's poses as loaded.  ValueError for a scene without cloud='depth': a .ply carries no visibility."""
        if self._depth is None:
            raise ValueError(f"'{self.tag}': no depth rays (dataset.cloud: depth, with a depth_file_path on the frames of transforms.json): a "
                             'point cloud from a file does not say where it was seen from')
        dev = None if device is None else torch.device(device)
        host = dev is None or dev.type == 'cpu'
        key = 'cpu' if host else str(dev)
        if key not in self._rays:
            D = self._depth
            depth = np.stack([read_depth_png(f) for f in D['files']])
            args = (depth, D['cams'], D['target'], D['poses'])
            kw = {k: D[k] for k in ('d_range', 'stride', 'edge')}
            rec = torch.from_numpy(ops.depth_rays_host(*args, **kw)) if host else ops.depth_rays(*args, device=dev, **kw)
            ends, frame = ops.depth_rays_compact(rec)
            origins = torch.from_numpy(np.ascontiguousarray(D['poses'][:, 9:12])).to(ends.device)
            self._rays[key] = (ends, frame, origins)
            self.rays_info = {'rays': int(ends.shape[0]), 'samples': int(rec.numel() // 4), 'frames': len(D['files'])}
        out = self._rays[key]
        return out if device is None else tuple(t.to(device) for t in out)

    def release_rays(self, device=None):
        """Drop the copy of rays() kept for `device` (None: every copy): a caller that has taken what it needs -- the model thins the rays to
        its own buffers -- gives the memory back; rays() builds them again when asked."""
        if device is None:
            self._rays.clear()
        else:
            dev = torch.device(device)
            self._rays.pop('cpu' if dev.type == 'cpu' else str(dev), None)

    def _depth_setup(self, path, meta, frames, c2w, F, size):
        """What cloud() hands ops.depth_cloud: the depth files and, per frame that has one, the camera row at the depth maps' resolution
        and the pose row [A, t] -- A = R_c2w . diag(1, -1, -1) * (unit * scale of F): the camera point (x right, y down, z forward, in
        depth steps) through the OpenGL axes (x, -y, -z) of the normalised cam2world --, the common target at zoom 1, the cube and the
        rules.  The intrinsics scale by (Wd / W, Hd / H): with pixel centres at +0.5 that is exact."""
        from PIL import Image
        o = self.cloud_options
        ids = [n for n, f in enumerate(frames) if f.get('depth_file_path')]
        if not ids:
            raise ValueError(f"{path}: cloud='depth', but no frame has a depth_file_path")
        files = [self._frame_file(path.parent, frames[n]['depth_file_path']) for n in ids]
        sizes = set()
        for f in files:
            with Image.open(f) as im:
                sizes.add(im.size)
        if len(sizes) != 1:
            raise ValueError(f'{path}: the depth maps must share one size, got {sorted(s[::-1] for s in sizes)}')
        Wd, Hd = sizes.pop()
        zoom = np.array([Wd / size[1], Hd / size[0]] * 2)
        if self.cameras == 'per_frame':
            intrs, dists, models = self.intrs[ids], self.dists[ids], self.models[ids]
        else:
            intrs, dists, models = np.tile(np.array(self.intr), (len(ids), 1)), np.tile(np.array(self.dist), (len(ids), 1)), np.zeros(len(ids), np.int64)
        unit = float(o['unit'] if o['unit'] is not None else meta.get('depth_unit_scale_factor', 1e-3))
        if not unit > 0:
            raise ValueError(f'{path}: depth_unit_scale_factor must be positive, got {unit}')
        scale = float(abs(np.linalg.det(F[:3, :3])) ** (1.0 / 3.0))
        poses = np.stack([np.concatenate([(c2w[n, :3, :3] * np.array([1.0, -1.0, -1.0]) * (unit * scale)).reshape(9), c2w[n, :3, 3]]) for n in ids])
        d_min, d_max = max(1, int(np.ceil(o['range'][0] / unit - 1e-9))), min(65535, int(np.floor(o['range'][1] / unit + 1e-9)))
        if d_min > d_max:
            raise ValueError(f"{path}: cloud.range {o['range']} m holds no 16-bit depth step of {unit} m")
        return {'files': files, 'frames': ids, 'size': (Hd, Wd), 'unit': unit, 'cams': ops.lens_table(intrs * zoom, dists, models),
                'target': ops.lens_target(np.array(self.intr) * zoom, 1.0), 'poses': poses.astype(np.float32), 'lo': -float(o['bound']),
                'hi': float(o['bound']), 'grid': int(o['grid']), 'd_range': (d_min, d_max), 'stride': int(o['stride']), 'edge': float(o['edge']),
                'min_count': int(o['min_count'])}

    @staticmethod
    def _frame_file(folder, file_path):
        f = folder / file_path
        if f.suffix == '':
            found = [g for g in (f.with_name(f.name + '.' + e) for e in IMG_EXTENSIONS) if g.exists()]
            if not found:
                raise FileNotFoundError(f"{f.absolute()}: no file with one of the extensions {IMG_EXTENSIONS}")
            return found[0].absolute()
        if not f.exists():
            raise FileNotFoundError(f'{f.absolute()} does not exist')
        return f.absolute()


def get_scene_class(name):
    if name == 'nerfstudio':
        raise NotImplementedError("dataset 'nerfstudio': the reference reads these scenes through the `nerfstudio` package, which is not "
                                  'installed here; DTU and BlendedMVS scenes are supported')
    return {'dtu': DTUScene, 'bmvs': BMVSScene, 'custom': CustomScene}[name]


def create_train_val_test(cfg, root, device=None):
    """src/dataset/__init__.py:9-26: the train, val and test scenes of cfg['dataset'] = {name, tag, img_size[, view_ids]} under `root`.
    The three share one ImageStore: every file is decoded and resized once.  With a device the training views are made resident now."""
    kwargs = deepcopy(cfg['dataset'])
    cls = get_scene_class(kwargs.pop('name'))
    kwargs.pop('on_disk', None)                                  # (the reference's switch for keeping the tensors in host memory: always resident here)
    train = cls(root, split='train', **deepcopy(kwargs))
    val = cls(root, split='val', store=train.store, **deepcopy(kwargs))
    test = cls(root, split='test', store=train.store, **deepcopy(kwargs))
    if device is not None:
        train.views(device)
    bs = cfg.get('training', {}).get('batch_size')
    print(f"Dataset '{cls.name}' init: kwargs={kwargs}, n_train={len(train)}, n_val={len(val)}, n_test={len(test)}, bs={bs}")
    return train, val, test
