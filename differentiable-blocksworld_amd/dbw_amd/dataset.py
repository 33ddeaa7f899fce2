"""Scene ingest: a DTU / BlendedMVS scene directory on disk -> the resident `views` dict Trainer(cfg, model, views) consumes, the
(inp, labels) loaders the evaluations walk, and the reference's YAML configs.  Restates src/dataset/dtu.py, src/dataset/bmvs.py,
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


def decode_rgb(path):
    """One image file -> (H,W,3) uint8, as Image.open(f).convert('RGB') reads it (dtu.py:63)."""
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert('RGB'))


class ImageStore:
    """The decoded frames of one scene directory, resident on one device: (N,3,H,W) fp32 targets of one img_size, filled file by file the
    first time a view is asked for, and optionally the raw (N,Hraw,Wraw,3) uint8 stack.  The three splits of a scene share one store."""

    def __init__(self, files, img_size, chunk=16):
        self.files, self.img_size, self.chunk = list(files), tuple(img_size), chunk
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
            self.imgs[idx] = ops.resample_u8(raw, self.img_size, out='f32')
            if self.raw is not None:
                self.raw[idx] = raw
                self.have_raw[part] = True
            self.have[part] = True
        idx = torch.as_tensor(ids, dtype=torch.long, device=device)
        return self.imgs[idx], (self.raw[idx] if keep_raw else None)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------------
class _Scene:
    """What the two dataset kinds share (dtu.py / bmvs.py): files, cameras, view ids, resident views and loaders."""
    name, folder, raw_img_size, n_channels = None, None, None, 3

    def __init__(self, root, tag, img_size, split, view_ids=None, store=None):
        self.split, self.tag = split, tag
        self.data_path = Path(root) / self.folder / tag / 'image'
        self.input_files = get_files_from(self.data_path, IMG_EXTENSIONS, recursive=True, sort=True)
        self.img_size = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)
        N = len(self.input_files)
        self.view_ids = self._split_ids(N, list(range(N)) if view_ids is None else list(deepcopy(view_ids)))
        cams = load_idr_cameras(self.data_path.parent / 'cameras.npz', self.raw_img_size, n_views=N)
        self.K, self.R, self.T, self.scale_mat = cams['K'], cams['R'], cams['T'], cams['scale_mat']
        self.pc_gt = torch.zeros(1, 3)
        if store is not None and ([str(f) for f in store.files] != [str(f) for f in self.input_files] or store.img_size != self.img_size):
            raise ValueError('store: made for other files or another img_size')
        self.store = store if store is not None else ImageStore(self.input_files, self.img_size)

    def _split_ids(self, N, view_ids):
        return view_ids

    def __len__(self):
        return len(self.view_ids)

    def ids(self):
        """The file index of every item of this split, in its order."""
        return self.view_ids[:len(self)]

    def views(self, device, keep_raw=False, chunk=None):
        """{'imgs' (V,3,H,W) fp32, 'K' (V,4,4), 'R' (V,3,3), 'T' (V,3)} of this split, in its order, resident on `device`; with keep_raw
        also 'raw' (V,Hraw,Wraw,3) uint8."""
        ids = self.ids()
        imgs, raw = self.store.get(device, ids, keep_raw=keep_raw, chunk=chunk)
        out = {'imgs': imgs, 'K': self.K[ids].to(device), 'R': self.R[ids].to(device), 'T': self.T[ids].to(device)}
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

    def __init__(self, root, tag, img_size, split, view_ids=None, store=None):
        super().__init__(root, tag, img_size, split, view_ids=view_ids, store=store)
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


def get_scene_class(name):
    if name == 'nerfstudio':
        raise NotImplementedError("dataset 'nerfstudio': the reference reads these scenes through the `nerfstudio` package, which is not "
                                  'installed here; DTU and BlendedMVS scenes are supported')
    return {'dtu': DTUScene, 'bmvs': BMVSScene}[name]


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
