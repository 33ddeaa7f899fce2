"""Checker side of the image scores: csrc/score_math.h built for the host with g++ (tests/host_score_math.cpp) behind the arguments of
ops.image_scores, the 2-D 11 x 11 definition of SSIM evaluated in fp64 (the arbiter), and the inputs both test files score.  Used by
tests/test_host_score_math.py (against the reference's golden map and the arbiter) and by tests/test_gpu_monitor.py (as the yardstick of
the kernel)."""
import ctypes
import os
import subprocess

import numpy as np
import torch
import torch.nn.functional as F

from host_build import host_lib

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'differentiable-blocksworld_amd', 'csrc')
SRCS = [os.path.join(HERE, 'host_score_math.cpp'), os.path.join(CSRC, 'score_math.h'), os.path.join(CSRC, 'raster_math.h')]
NOISE_SHAPES = [(11, 11), (12, 16), (23, 37), (37, 70)]
RENDER_SHAPE = (48, 64)
_CACHE = {}


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in SRCS)


def lib():
    return host_lib('score_math')


def sanitized_program():
    """tests/_build/host_score_math_san: the same file as a program of its own (-DSCORE_MATH_MAIN) under -fsanitize=address,undefined."""
    out = os.path.join(HERE, '_build')
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, 'host_score_math_san')
    if _stale(exe):
        subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                               '-DSCORE_MATH_MAIN', SRCS[0], '-o', exe])
    return exe


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def image_scores_host(a, b, padding=False):
    """dbw_image_scores on the CPU through the host build: (N,3,H,W) CPU tensors -> (out (N,2) fp64 [sum (a-b)^2, sum ssim], map (N,3,H',W'))."""
    a, b = a.detach().cpu().float().contiguous(), b.detach().cpu().float().contiguous()
    N, _, H, W = a.shape
    Hp, Wp = (H, W) if padding else (H - 10, W - 10)
    m = torch.empty(N, 3, max(Hp, 0), max(Wp, 0))
    out = torch.empty(N, 2, dtype=torch.float64)
    rc = lib().host_image_scores(_p(a), _p(b), N, H, W, int(padding), _p(m), _p(out))
    if rc != 0:
        raise ValueError(f'host_image_scores refused N={N}, H={H}, W={W}, padding={padding}')
    return out, m


def window_host():
    w = torch.empty(11)
    lib().host_ssim_window(_p(w))
    return w


def ssim_map_fp64(a, b, padding=False):
    """The arbiter: the reference's definition (loss.py:124-156) with its 2-D 11 x 11 window (the outer product of the fp32 weights), every
    operation in fp64."""
    x = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-x * x / (2.0 * 1.5 * 1.5))
    g = (g / g.sum()).float().double()
    w2 = (g[:, None] * g[None, :]).view(1, 1, 11, 11).expand(3, 1, 11, 11)
    a, b, pad = a.double(), b.double(), 5 if padding else 0

    def blur(t):
        return F.conv2d(t, w2, padding=pad, groups=3)
    mu1, mu2 = blur(a), blur(b)
    s11, s22, s12 = blur(a * a) - mu1 * mu1, blur(b * b) - mu2 * mu2, blur(a * b) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))


def noise_pair(H, W, N=1):
    g = torch.Generator().manual_seed(1000 * H + W)
    return torch.rand(N, 3, H, W, generator=g), torch.rand(N, 3, H, W, generator=g)


def render_like_pair(H=48, W=64, N=1):
    """Piecewise-constant regions, the second image's vertical edge shifted by two pixels, 0.002 of noise on both: what a render against
    its target looks like, and the hard case of E[x^2] - mu^2 in fp32 (flat regions cancel down to C2 = 9e-4)."""
    g = torch.Generator().manual_seed(77)
    a, b = torch.empty(N, 3, H, W), torch.empty(N, 3, H, W)
    for n in range(N):
        lv = torch.rand(4, 3, generator=g)
        for t, ex in ((a, W // 2), (b, W // 2 + 2)):
            t[n, :, :H // 3, :ex], t[n, :, :H // 3, ex:] = lv[0].view(3, 1, 1), lv[1].view(3, 1, 1)
            t[n, :, H // 3:, :ex], t[n, :, H // 3:, ex:] = lv[2].view(3, 1, 1), lv[3].view(3, 1, 1)
    a = a + 0.002 * torch.randn(a.shape, generator=g)
    b = b + 0.002 * torch.randn(b.shape, generator=g)
    return a.clamp(0, 1), b.clamp(0, 1)


def case(name, N=1):
    """name: 'noise_HxW' or 'render' -> dict(a, b, and per padding p in (0, 1): host_out{p}, host_map{p}), made once and shared."""
    key = (name, N)
    if key not in _CACHE:
        if name == 'render':
            a, b = render_like_pair(*RENDER_SHAPE, N=N)
        else:
            H, W = [int(v) for v in name.split('_')[1].split('x')]
            a, b = noise_pair(H, W, N)
        c = dict(a=a, b=b)
        for p in (0, 1):
            c[f'host_out{p}'], c[f'host_map{p}'] = image_scores_host(a, b, bool(p))
        _CACHE[key] = c
    return _CACHE[key]
