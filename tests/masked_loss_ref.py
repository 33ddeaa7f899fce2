"""Checker side of the masked image terms (csrc/masked_loss.hip, csrc/ssim_term.hip, ops.composite_mse_masked, ops.ssim_term(masks=)): the arithmetic built for
the host with g++ (tests/host_masked_loss.cpp), the float64 oracles, the inputs and the bars that tests/test_host_masked_loss.py (CPU) and
tests/test_gpu_masked_loss.py hold values and gradients to.

SSIM term.  Oracle: s = metrics.ssim_map(a * m, b * m, padding=True); ((1 - s) * m).sum() / (3 * m.sum()) in float64 under autograd.  Bar:
ssim_term_ref.bars with 1 / count in place of 1 / M -- at most 4 x the error of torch's own fp32 evaluation of the same formula against the
same float64 values, floors 1e-6 relative on the value and 1e-6 * max(max|g64|, 1 / count) on the gradient.

Composite.  Oracle: rec = fg_rgb * fg_a + (1 - fg_a) * env_rgb, L = g * w * sum m (rec - img)^2 / count + <x, rec> in float64 under autograd
(x: what another term sends to rec), the gradients in fg and env.  The same kind of bar: 4 x torch's fp32 error, floors 1e-6 relative on
the value and 1e-6 * max|g64| on each gradient; rec to 1e-6 (three fp32 roundings on values in [0, 1])."""
import ctypes
import os
import subprocess

import numpy as np
import torch

import ssim_term_ref as TR
from dbw_amd import metrics
from host_build import host_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = TR.SHAPES
KINDS = TR.KINDS                                     # the images: noise, equal, black
MASKS = ['ones', 'holes', 'fraction', 'ring', 'empty']
CASES = [(k, mk, s) for s in SHAPES for k in KINDS for mk in MASKS]
COMPOSITE_SHAPES = SHAPES + [(3, 40, 100)]           # ... and one with more than one workgroup behind the fixed-order sum
COMPOSITE_CASES = [(mk, s) for s in COMPOSITE_SHAPES for mk in MASKS]
WEIGHT, UPSTREAM = 0.7, 1.3                          # w_rgb and the upstream scalar of the composite cases
_CACHE = {}


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def lib():
    return host_lib('masked_loss')


def mask(kind, shape):
    """(N,1,H,W) fp32 weights in [0, 1]."""
    N, H, W = shape
    g = torch.Generator().manual_seed(7000 * len(kind) + 100 * H + W)
    if kind == 'ones':
        return torch.ones(N, 1, H, W)
    if kind == 'empty':
        return torch.zeros(N, 1, H, W)
    if kind == 'holes':                              # 30 % random zeros plus a rectangle
        m = (torch.rand(N, 1, H, W, generator=g) >= 0.3).float()
        m[:, :, H // 4:H // 2 + 1, W // 3:2 * W // 3 + 1] = 0
        return m
    if kind == 'fraction':                           # uniform weights, some of them exactly 0
        m = torch.rand(N, 1, H, W, generator=g)
        m[torch.rand(N, 1, H, W, generator=g) < 0.2] = 0
        return m
    if kind == 'ring':                               # valid inside an ellipse only: the lens case
        y = (torch.arange(H).float() + 0.5) / H * 2 - 1
        x = (torch.arange(W).float() + 0.5) / W * 2 - 1
        return ((y[:, None] / 0.95) ** 2 + (x[None, :] / 0.9) ** 2 <= 1).float().expand(N, 1, H, W).contiguous()
    raise KeyError(kind)


def count_of(m):
    return 3.0 * float(m.double().sum())


def case_id(c):
    return f'{c[0]}_{c[1]}_{c[2][0]}x3x{c[2][1]}x{c[2][2]}'


# ---- the SSIM term ------------------------------------------------------------------------------------------------------------------------------
def _formula(a, b, m):
    s = metrics.ssim_map(a * m, b * m, padding=True)
    total = ((1 - s) * m).sum()
    cnt = 3 * m.sum()
    return total / cnt if float(cnt) > 0 else total * 0.0


def term_torch(a, b, m, dtype):
    """The formula and its autograd gradient in b, evaluated in `dtype` on the CPU."""
    a, b, m = (t.detach().cpu().to(dtype) for t in (a, b, m))
    b = b.clone().requires_grad_(True)
    v = _formula(a, b, m)
    g, = torch.autograd.grad(v, b)
    return v.detach(), g


def term_host(a, b, m, count=None, with_grad=True):
    """dbw_monitor_masked_ssim_term on the CPU through the host build -> (value: python float of the fp64, grad or None)."""
    a, b, m = (t.detach().cpu().float().contiguous() for t in (a, b, m))
    N, _, H, W = a.shape
    count = count_of(m) if count is None else float(count)
    grad = torch.full_like(b, float('nan')) if with_grad else None
    value = torch.full((1,), -1.0, dtype=torch.float64)
    rc = lib().host_masked_ssim_term(_p(a), _p(b), _p(m), N, H, W, ctypes.c_double(count), _p(grad), _p(value))
    if rc != 0:
        raise ValueError(f'host_masked_ssim_term refused N={N}, H={H}, W={W}')
    return value.item(), grad


def bars(v64, g64, v32, g32, count):
    ev, eg = abs(v32 - v64), (g32.double() - g64).abs().max().item()
    floor = 1.0 / count if count > 0 else 0.0
    return dict(torch_err_v=ev, torch_err_g=eg, tol_v=max(4 * ev, 1e-6 * abs(v64)), tol_g=max(4 * eg, 1e-6 * max(g64.abs().max().item(), floor)))


def case(kind, mkind, shape):
    """dict(a, b, m, count, v64, g64, v32, g32, tol_v, tol_g), made once and shared."""
    key = (kind, mkind, tuple(shape))
    if key not in _CACHE:
        a, b = TR.pair(kind, shape)
        m = mask(mkind, shape)
        v64, g64 = term_torch(a, b, m, torch.float64)
        v32, g32 = term_torch(a, b, m, torch.float32)
        c = dict(a=a, b=b, m=m, count=count_of(m), v64=v64.item(), g64=g64, v32=v32.item(), g32=g32)
        c.update(bars(c['v64'], g64, v32.double().item(), g32, c['count']))
        _CACHE[key] = c
    return _CACHE[key]


def check(name, c, value, grad):
    """Prints both errors of one case and holds value (a float, from the fp64 the code returns) and gradient to the bar of `c`."""
    ev = abs(value - c['v64'])
    eg = (grad.detach().cpu().double() - c['g64']).abs().max().item()
    print(f"{name}: value err {ev:.3e} (torch fp32 {c['torch_err_v']:.3e}, bar {c['tol_v']:.3e}, value {c['v64']:.6f}); "
          f"grad err {eg:.3e} (torch fp32 {c['torch_err_g']:.3e}, bar {c['tol_g']:.3e}, max|g| {c['g64'].abs().max().item():.3e})")
    assert np.isfinite(value) and bool(torch.isfinite(grad).all()), f'{name}: a value that is not finite'
    assert ev <= c['tol_v'], f'{name}: value error {ev:.3e} above {c["tol_v"]:.3e}'
    assert eg <= c['tol_g'], f'{name}: gradient error {eg:.3e} above {c["tol_g"]:.3e}'


def repaint(t, m, seed):
    """t with other finite content wherever m == 0 (junk of both signs, far outside [0, 1])."""
    junk = (torch.rand(t.shape, generator=torch.Generator().manual_seed(seed)) - 0.3) * 7
    return torch.where((m == 0).expand_as(t), junk.to(t.device), t)


# ---- the composite ------------------------------------------------------------------------------------------------------------------------------
def _composite_loss(fg, env, imgs, m, x, scale, upstream):
    rec = fg[:, :3] * fg[:, 3:4] + (1 - fg[:, 3:4]) * env[:, :3]
    value = (m * (rec - imgs) ** 2).sum() * scale
    return rec, value, upstream * value + (0 if x is None else (x * rec).sum())


def composite_torch(c, dtype, with_extra):
    fg, env, imgs, m, x = (c[k].to(dtype) for k in ('fg', 'env', 'imgs', 'm', 'x'))
    fg, env = fg.clone().requires_grad_(True), env.clone().requires_grad_(True)
    rec, value, total = _composite_loss(fg, env, imgs, m, x if with_extra else None, c['scale'], UPSTREAM)
    g_fg, g_env = torch.autograd.grad(total, (fg, env))
    return rec.detach(), value.detach(), g_fg, g_env


def composite_case(mkind, shape):
    """dict(fg, env, imgs, m, x, count, scale, and per with_extra in (False, True): rec64, v64, gfg64, genv64 and the bars)."""
    key = ('composite', mkind, tuple(shape))
    if key not in _CACHE:
        N, H, W = shape
        g = torch.Generator().manual_seed(31 * H + W + len(mkind))
        c = dict(fg=torch.rand(N, 4, H, W, generator=g), env=torch.rand(N, 4, H, W, generator=g), imgs=torch.rand(N, 3, H, W, generator=g),
                 x=torch.randn(N, 3, H, W, generator=g) * 1e-3, m=mask(mkind, shape))
        c['count'] = count_of(c['m'])
        c['scale'] = WEIGHT / c['count'] if c['count'] > 0 else 0.0
        for extra in (False, True):
            rec64, v64, gfg64, genv64 = composite_torch(c, torch.float64, extra)
            rec32, v32, gfg32, genv32 = composite_torch(c, torch.float32, extra)
            tol = lambda a64, a32: max(4 * (a32.double() - a64).abs().max().item(), 1e-6 * a64.abs().max().item())
            c[extra] = dict(rec64=rec64, v64=v64.item(), gfg64=gfg64, genv64=genv64, tol_v=max(4 * abs(v32.double().item() - v64.item()), 1e-6 * abs(v64.item())),
                            tol_gfg=tol(gfg64, gfg32), tol_genv=tol(genv64, genv32))
        _CACHE[key] = c
    return _CACHE[key]


def composite_host(c, with_extra, upstream=UPSTREAM, scale=None):
    """dbw_monitor_masked_composite on the CPU through the host build, forward and backward -> (rec, value float, grad_fg, grad_env)."""
    fg, env, imgs, m = (c[k].float().contiguous() for k in ('fg', 'env', 'imgs', 'm'))
    x = c['x'].float().contiguous() if with_extra else None
    N, _, H, W = fg.shape
    rec, gfg, genv = torch.full_like(imgs, float('nan')), torch.full_like(fg, float('nan')), torch.full_like(env, float('nan'))
    value = torch.full((1,), -1.0, dtype=torch.float64)
    rc = lib().host_masked_composite(_p(fg), _p(env), _p(imgs), _p(m), N, H, W, ctypes.c_double(c['scale'] if scale is None else scale), _p(rec), _p(value),
                                     ctypes.c_float(upstream), _p(x), _p(gfg), _p(genv))
    assert rc == 0
    return rec, value.item(), gfg, genv


def composite_check(name, c, with_extra, rec, value, gfg, genv):
    r = c[with_extra]
    er = (rec.detach().cpu().double() - r['rec64']).abs().max().item()
    ev = abs(value - r['v64'])
    ef, ee = (gfg.detach().cpu().double() - r['gfg64']).abs().max().item(), (genv.detach().cpu().double() - r['genv64']).abs().max().item()
    print(f"{name}: rec err {er:.3e}; value err {ev:.3e} (bar {r['tol_v']:.3e}, value {r['v64']:.6f}); grad_fg err {ef:.3e} (bar {r['tol_gfg']:.3e}), "
          f"grad_env err {ee:.3e} (bar {r['tol_genv']:.3e})")
    assert er <= 1e-6 and ev <= r['tol_v'] and ef <= r['tol_gfg'] and ee <= r['tol_genv'], name


# ---- the lens predicate ---------------------------------------------------------------------------------------------------------------------------
def lens_valid_host(H, W, lens):
    """dbw_lens_valid_u8 on the CPU through the host build: lens (12,) fp32 -> (H,W) uint8."""
    lens = np.ascontiguousarray(lens, dtype=np.float32)
    out = np.full((H, W), 7, np.uint8)
    assert lib().host_lens_valid_u8(H, W, ctypes.c_void_p(lens.ctypes.data), ctypes.c_void_p(out.ctypes.data)) == 0
    return out


def sanitized_program():
    """tests/_build/host_masked_loss_san: the same file as a program of its own (-DMASKED_LOSS_MAIN) under -fsanitize=address,undefined."""
    out = os.path.join(HERE, '_build')
    os.makedirs(out, exist_ok=True)
    src, exe = os.path.join(HERE, 'host_masked_loss.cpp'), os.path.join(out, 'host_masked_loss_san')
    csrc = os.path.join(HERE, '..', 'differentiable-blocksworld_amd', 'csrc')
    deps = [src] + [os.path.join(csrc, h) for h in ('score_math.h', 'loss_math.h', 'lens_math.h', 'raster_math.h')]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in deps):
        subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                               '-DMASKED_LOSS_MAIN', src, '-o', exe])
    return exe
