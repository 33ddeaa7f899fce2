"""Checker side of the SSIM term (ops.ssim_term, csrc/ssim_term.hip): the arithmetic of csrc/score_math.h built for the host with g++
(tests/host_ssim_term.cpp), the float64 oracles, the inputs and the bar that tests/test_host_ssim_term.py (CPU) and
tests/test_gpu_ssim_term.py hold value and gradient to.

The bar (the same for the host build and the kernel): on every input the error against float64 may be at most 4 x the error that torch's own
fp32 evaluation of the same formula (metrics.ssim_map(padding=True) under autograd) leaves against the same float64 values -- the factor
covers another order of the same fp32 operations (rows first, other rounding order) -- with a floor of a few fp32 roundings at the
natural scale where torch happens to be exact: 1e-6 relative on the value, 1e-6 * max(max|g64|, 1/M) on the gradient."""
import ctypes
import os
import subprocess

import numpy as np
import torch
import torch.nn.functional as F

from dbw_amd import metrics
from host_build import host_lib

HERE = os.path.dirname(os.path.abspath(__file__))
# the kernel's tile is 16 x 32: an image smaller than the window; exactly one tile (N = 2: the plane index); one pixel into the next tile
# both ways; ragged with W % 4 != 0 (element loads); a tile with all eight neighbours with W % 4 == 0 (16-byte loads)
SHAPES = [(1, 5, 7), (2, 16, 32), (1, 17, 33), (2, 19, 37), (1, 48, 96)]
KINDS = ['noise', 'equal', 'black']
BLOCKS = ('blocks', (2, 19, 37))                     # the constant-block pair of tests/golden/ssim_term.npz, rec == target on image 0
CASES = [(k, s) for s in SHAPES for k in KINDS] + [BLOCKS]
BLOCKS_SEED = 1937
_CACHE = {}


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def term_host(a, b, with_grad=True):
    """dbw_monitor_ssim_term on the CPU through the host build: (N,3,H,W) CPU tensors -> (value: python float of the fp64, grad or None,
    SSIM map)."""
    a, b = a.detach().cpu().float().contiguous(), b.detach().cpu().float().contiguous()
    N, _, H, W = a.shape
    grad, m = (torch.empty_like(b) if with_grad else None), torch.empty_like(b)
    value = torch.full((1,), -1.0, dtype=torch.float64)
    rc = host_lib('ssim_term').host_ssim_term(_p(a), _p(b), N, H, W, _p(grad), _p(m), _p(value))
    if rc != 0:
        raise ValueError(f'host_ssim_term refused N={N}, H={H}, W={W}')
    return value.item(), grad, m


def sanitized_program():
    """tests/_build/host_ssim_term_san: the same file as a program of its own (-DSSIM_TERM_MAIN) under -fsanitize=address,undefined."""
    out = os.path.join(HERE, '_build')
    os.makedirs(out, exist_ok=True)
    src, exe = os.path.join(HERE, 'host_ssim_term.cpp'), os.path.join(out, 'host_ssim_term_san')
    hdr = os.path.join(HERE, '..', 'differentiable-blocksworld_amd', 'csrc', 'score_math.h')
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in (src, hdr)):
        subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                               '-DSSIM_TERM_MAIN', src, '-o', exe])
    return exe


def _value_grad(fn, a, b):
    b = b.clone().requires_grad_(True)
    v = fn(a, b)
    g, = torch.autograd.grad(v, b)
    return v.detach(), g


def term_torch(a, b, dtype):
    """(1 - metrics.ssim_map(a, b, padding=True)).mean() and its autograd gradient in b, evaluated in `dtype` on the CPU."""
    return _value_grad(lambda x, y: (1 - metrics.ssim_map(x, y, padding=True)).mean(), a.detach().cpu().to(dtype), b.detach().cpu().to(dtype))


def term_fp64_2d(a, b):
    """The reference's definition (loss.py:124-156, padding=True, then the mean) with its 2-D 11 x 11 window -- the outer product of the
    fp32 weights --, every operation in float64, and its autograd gradient in b."""
    g = metrics.gaussian_window().double()
    w2 = (g[:, None] * g[None, :]).view(1, 1, 11, 11).expand(3, 1, 11, 11)

    def f(x, y):
        def blur(t):
            return F.conv2d(t, w2, padding=5, groups=3)
        mu1, mu2 = blur(x), blur(y)
        s11, s22, s12 = blur(x * x) - mu1 * mu1, blur(y * y) - mu2 * mu2, blur(x * y) - mu1 * mu2
        c1, c2 = 0.01 ** 2, 0.03 ** 2
        return (1 - ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))).mean()
    return _value_grad(f, a.detach().cpu().double(), b.detach().cpu().double())


def block_pair(N, H, W, seed, equal_first=False):
    """Constant blocks: four flat regions per image and channel, the second image's vertical edge two pixels further right and its levels a
    little off -- no noise, so that every window inside a region is flat (the hard case of E[x^2] - mu^2 and of the derivative maps, which
    grow to 1 / C2 there).  equal_first: rec == target on image 0."""
    g = torch.Generator().manual_seed(seed)
    a, b = torch.empty(N, 3, H, W), torch.empty(N, 3, H, W)
    for n in range(N):
        lv = torch.rand(4, 3, generator=g)
        lw = (lv + 0.05 * (torch.rand(4, 3, generator=g) - 0.5)).clamp(0, 1)
        for t, l, ex in ((a, lv, W // 2), (b, lw, W // 2 + 2)):
            t[n, :, :H // 3, :ex], t[n, :, :H // 3, ex:] = l[0].view(3, 1, 1), l[1].view(3, 1, 1)
            t[n, :, H // 3:, :ex], t[n, :, H // 3:, ex:] = l[2].view(3, 1, 1), l[3].view(3, 1, 1)
    if equal_first:
        b[0] = a[0]
    return a, b


def pair(kind, shape):
    N, H, W = shape
    g = torch.Generator().manual_seed(100000 * len(kind) + 1000 * H + W)
    if kind == 'noise':
        return torch.rand(N, 3, H, W, generator=g), torch.rand(N, 3, H, W, generator=g)
    if kind == 'blocks':
        return block_pair(N, H, W, BLOCKS_SEED, equal_first=True)
    if kind == 'equal':                              # rec == target: the minimum of the term, value 0 and gradient 0
        a = torch.rand(N, 3, H, W, generator=g)
        return a, a.clone()
    if kind == 'black':                              # nearly black: mu^2 and the variances far below C1 and C2
        return 0.004 * torch.rand(N, 3, H, W, generator=g), 0.004 * torch.rand(N, 3, H, W, generator=g)
    raise KeyError(kind)


def case_id(c):
    return f'{c[0]}_{c[1][0]}x3x{c[1][1]}x{c[1][2]}'


def case(kind, shape):
    """dict(a, b, v64, g64: the float64 oracle metrics.ssim_map(padding=True) under autograd; v32, g32: torch's fp32 evaluation of the same;
    tol_v, tol_g: the bar), made once and shared."""
    key = (kind, tuple(shape))
    if key not in _CACHE:
        a, b = pair(kind, shape)
        v64, g64 = term_torch(a, b, torch.float64)
        v32, g32 = term_torch(a, b, torch.float32)
        c = dict(a=a, b=b, v64=v64.item(), g64=g64, v32=v32.item(), g32=g32)
        c.update(bars(c['v64'], g64, v32.double().item(), g32))
        _CACHE[key] = c
    return _CACHE[key]


def bars(v64, g64, v32, g32):
    M = g64.numel()
    ev, eg = abs(v32 - v64), (g32.double() - g64).abs().max().item()
    return dict(torch_err_v=ev, torch_err_g=eg, tol_v=max(4 * ev, 1e-6 * abs(v64)), tol_g=max(4 * eg, 1e-6 * max(g64.abs().max().item(), 1.0 / M)))


def check(name, c, value, grad):
    """Prints both errors of one case and holds value (a float, from the fp64 the code returns) and gradient to the bar of `c`."""
    ev = abs(value - c['v64'])
    eg = (grad.detach().cpu().double() - c['g64']).abs().max().item()
    gmax = c['g64'].abs().max().item()
    print(f"{name}: value err {ev:.3e} (torch fp32 {c['torch_err_v']:.3e}, bar {c['tol_v']:.3e}, value {c['v64']:.6f}); "
          f"grad err {eg:.3e} (torch fp32 {c['torch_err_g']:.3e}, bar {c['tol_g']:.3e}, max|g| {gmax:.3e})")
    assert ev <= c['tol_v'], f'{name}: value error {ev:.3e} above {c["tol_v"]:.3e}'
    assert eg <= c['tol_g'], f'{name}: gradient error {eg:.3e} above {c["tol_g"]:.3e}'


def fixture_pairs(golden_dir):
    """[(name, a, b, the reference's value, its gradient)] of tests/golden/ssim_term.npz (the first pair's images are those of ssim.npz)."""
    g, pin = np.load(os.path.join(golden_dir, 'ssim_term.npz')), np.load(os.path.join(golden_dir, 'ssim.npz'))
    t = torch.from_numpy
    return [('ssim.npz', t(pin['img1']), t(pin['img2']), float(g['value']), t(g['grad'])),
            ('blocks', t(g['blocks_a']), t(g['blocks_b']), float(g['blocks_value']), t(g['blocks_grad']))]


def fixture_check(name, a, b, ref_v, ref_g, value, grad):
    """|ours - reference| <= (the reference's own fp32 error against float64) + (the bar of ssim_term_ref on this input)."""
    v64, g64 = term_fp64_2d(a, b)
    v32, g32 = term_torch(a, b, torch.float32)
    bar = bars(v64.item(), g64, v32.double().item(), g32)
    ref_ev, ref_eg = abs(ref_v - v64.item()), (ref_g.double() - g64).abs().max().item()
    ev, eg = abs(value - ref_v), (grad.detach().cpu().double() - ref_g.double()).abs().max().item()
    print(f'{name}: value {ev:.3e} from the reference (its own error {ref_ev:.3e}), gradient {eg:.3e} (its own error {ref_eg:.3e}, '
          f'max|g| {ref_g.abs().max().item():.3e})')
    assert ev <= ref_ev + bar['tol_v'] and eg <= ref_eg + bar['tol_g']
