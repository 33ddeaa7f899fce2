"""Checker side of the image ingest: csrc/resample_math.h built for the host with g++ (tests/host_resample_math.cpp) behind the arguments
of ops.resample_u8, a double-precision numpy restatement of its coefficient tables, and the reference's transform restated with PIL and
torch.  Used by tests/test_host_resample_math.py (against Pillow's bytes), tests/test_dataset_host.py (as the stand-in for the kernel)
and tests/test_gpu_ingest.py (as the yardstick of the kernel)."""
import ctypes
import math
import os

import numpy as np
import torch

from host_build import host_lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'resample_pil.npz')

# (Hin, Win) -> (Hout, Wout) of tests/golden/resample_pil.npz, by tag (tests/golden/make_resample_golden.py writes them)
SHAPES = {
    'identity': ((576, 768), (576, 768)),
    'half': ((540, 960), (270, 480)),
    'stripes': ((37, 53), (9, 13)),
    'odd': ((40, 64), (13, 17)),
    'up': ((16, 24), (40, 50)),
    'x_only': ((23, 31), (23, 8)),
    'y_only': ((23, 31), (7, 31)),
    'zeros': ((37, 53), (9, 13)),
    'ones': ((37, 53), (9, 13)),
    'checker': ((40, 64), (13, 17)),
    'ratio4': ((48, 64), (12, 16)),
    'tiles': ((150, 260), (37, 65)),
    'tall': ((400, 8), (3, 8)),
}


def make_input(tag):
    """The seeded input image of a fixture tag, (Hin, Win, 3) uint8 (the fixture keeps only Pillow's outputs)."""
    (H, W), _ = SHAPES[tag]
    if tag == 'zeros':
        return np.zeros((H, W, 3), np.uint8)
    if tag == 'ones':
        return np.full((H, W, 3), 255, np.uint8)
    if tag == 'stripes':                                        # alternating 0 / 255 rows
        return np.repeat(((np.arange(H) % 2) * 255).astype(np.uint8)[:, None, None], W, 1).repeat(3, 2)
    if tag == 'checker':
        return np.repeat((((np.arange(H)[:, None] + np.arange(W)[None]) % 2) * 255).astype(np.uint8)[:, :, None], 3, 2)
    rng = np.random.RandomState(sum(ord(c) for c in tag))
    if H * W > 100000:                                          # the two large ones: ramps (a small fixture) around a patch of noise
        y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(3), indexing='ij')
        a = ((x * 3 + y * 5 + c * 40) % 256).astype(np.uint8)
        a[100:196, 200:328] = rng.randint(0, 256, (96, 128, 3)).astype(np.uint8)
        return a
    a = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    a[: H // 4, : W // 4] = rng.randint(0, 2, (H // 4, W // 4, 3)).astype(np.uint8) * 255      # a corner of extremes
    return a


def lib():
    return host_lib('resample_math')


def table_host(in_size, out_size):
    """(out_size, ksize + 2) int32 rows [xmin, n, k...] from the host build of the header."""
    ksize = lib().host_resample_table(in_size, out_size, None, ctypes.c_longlong(0))
    assert ksize > 0
    t = np.zeros((out_size, ksize + 2), np.int32)
    assert lib().host_resample_table(in_size, out_size, ctypes.c_void_p(t.ctypes.data), ctypes.c_longlong(t.size)) == ksize
    return t


def table_numpy(in_size, out_size):
    """The same rows restated in numpy float64 from the text of Pillow's algorithm."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support, ss = fs, 1.0 / fs
    ksize = int(math.ceil(support)) * 2 + 1
    t = np.zeros((out_size, ksize + 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        x = np.arange(n, dtype=np.float64)
        tt = np.abs((x + xmin - center + 0.5) * ss)
        w = np.where(tt < 1.0, 1.0 - tt, 0.0)
        w = w / w.sum()
        t[xx, 0], t[xx, 1] = xmin, n
        t[xx, 2:2 + n] = (w * float(1 << 22) + 0.5).astype(np.int64)
    return t


def resample_host(src, size, out='f32'):
    """ops.resample_u8 on the CPU through the host build of resample_math.h: src (N,Hin,Win,3) uint8 CPU tensor."""
    if src.is_cuda or src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] != 3:
        raise RuntimeError('src: an (N,Hin,Win,3) uint8 CPU tensor')
    src = src.contiguous()
    N, Hin, Win, _ = src.shape
    Hout, Wout = size
    f32 = torch.empty(N, 3, Hout, Wout) if out in ('f32', 'both') else None
    u8 = torch.empty(N, Hout, Wout, 3, dtype=torch.uint8) if out in ('u8', 'both') else None
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    assert lib().host_images_resample_u8(p(src), N, Hin, Win, Hout, Wout, p(f32), p(u8)) == 0
    return {'f32': f32, 'u8': u8, 'both': (f32, u8)}[out]


def pil_resize(a, size):
    """Resize(size) of torchvision on a PIL image: Pillow's BILINEAR.  a (Hin,Win,3) uint8 numpy, size (Hout,Wout) -> (Hout,Wout,3) uint8."""
    from PIL import Image
    return np.array(Image.fromarray(a, 'RGB').resize((size[1], size[0]), Image.BILINEAR))


def to_tensor(a):
    """ToTensor of torchvision on an (H,W,3) uint8 array: (3,H,W) fp32 in [0, 1]."""
    return torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1).contiguous().float().div(255)
