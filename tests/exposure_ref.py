"""Checker side of the per-view exposure compensation (csrc/exposure_math.h, csrc/exposure_loss.hip, ops.composite_mse_exposure; DESIGN.md
6s): the inputs of the kernel cases, a numpy float64 restatement of the term and of its gradients, and the host build of the arithmetic
(tests/host_exposure_math.cpp), shared by tests/test_host_exposure_math.py (CPU) and tests/test_gpu_exposure.py.

The term of a case: with comp = fg_rgb * fg_a + (1 - fg_a) * env_rgb and the row (g, b) = theta[ids[n]] of view n (zero for an id outside
the table), rec = exp(g) * comp + b, value = scale * sum m (rec - img)^2, L = UPSTREAM * value + <x, rec> (x: what another term sends to
rec).  backward64 returns dL / d fg, dL / d env and, per row of theta, the six sums together with the sums of the terms' magnitudes, which
is what the bound on a reduced sum is stated in."""
import ctypes

import numpy as np
import torch

from host_build import host_lib

SHAPES = [(1, 1, 1), (2, 5, 7), (3, 12, 16), (3, 40, 100)]       # scalar path (twice), vector path, more than one workgroup per view (ragged)
MASKS = ['none', 'random', 'zero_view']
CASES = [(s, m) for s in SHAPES for m in MASKS]
V = 5
WEIGHT, UPSTREAM = 0.7, 1.3
_CACHE = {}


def case_id(c):
    return f'{c[0][0]}x{c[0][1]}x{c[0][2]}_{c[1]}'


def case(shape, mkind):
    """dict(fg, env, imgs, m (None without masks), x, theta (V,6) in +-0.3, ids (N,) int32: a shuffled subset of the V rows, count, scale),
    fp32 torch tensors on the CPU, made once and shared; nobody writes to them."""
    key = (tuple(shape), mkind)
    if key not in _CACHE:
        N, H, W = shape
        g = torch.Generator().manual_seed(1000 * H + 10 * W + len(mkind))
        c = dict(fg=torch.rand(N, 4, H, W, generator=g), env=torch.rand(N, 4, H, W, generator=g), imgs=torch.rand(N, 3, H, W, generator=g),
                 x=torch.randn(N, 3, H, W, generator=g) * 1e-3, theta=(torch.rand(V, 6, generator=g) - 0.5) * 0.6,
                 ids=torch.randperm(V, generator=g)[:N].to(torch.int32))
        m = None
        if mkind != 'none':
            m = torch.rand(N, 1, H, W, generator=g)
            if mkind == 'zero_view':
                m[0] = 0
        c['m'] = m
        c['count'] = float(3 * N * H * W) if m is None else 3.0 * float(m.double().sum())
        c['scale'] = WEIGHT / c['count'] if c['count'] > 0 else 0.0
        _CACHE[key] = c
    return _CACHE[key]


def _np(t):
    return None if t is None else t.detach().cpu().double().numpy()


def rows64(theta, ids):
    """(N,6) float64: the rows of theta of the batch, zero for an id outside the table."""
    theta, ids = np.asarray(theta, dtype=np.float64), np.asarray(ids).astype(np.int64)
    out = np.zeros((len(ids), 6))
    ok = (ids >= 0) & (ids < len(theta))
    out[ok] = theta[ids[ok]]
    return out


def forward64(fg, env, imgs, m, theta, ids, scale):
    """-> (rec (N,3,H,W), value, comp, the per-pixel term m * sum_c (rec - img)^2 (N,H,W)) in float64."""
    fg, env, imgs = (np.asarray(a, dtype=np.float64) for a in (fg, env, imgs))
    a = fg[:, 3:4]
    comp = fg[:, :3] * a + (1 - a) * env[:, :3]
    t = rows64(theta, ids)
    rec = np.exp(t[:, :3])[:, :, None, None] * comp + t[:, 3:, None, None]
    mm = np.ones_like(a) if m is None else np.asarray(m, dtype=np.float64)
    pix = (mm * (rec - imgs) ** 2).sum(1)
    return rec, scale * pix.sum(), comp, pix


def pixel_loss64(fg, env, imgs, m, x, theta, ids, scale, upstream=UPSTREAM):
    """L split by view and pixel, (N,H,W): UPSTREAM * scale * m sum_c (rec - img)^2 + sum_c x rec.  Its sum is L; the pixels are
    independent in fg and env, the views in theta: what the central differences of the tests lean on."""
    rec, _, _, pix = forward64(fg, env, imgs, m, theta, ids, scale)
    return upstream * scale * pix + (0.0 if x is None else (np.asarray(x, dtype=np.float64) * rec).sum(1))


def backward64(fg, env, imgs, m, x, theta, ids, scale, upstream=UPSTREAM):
    """The analytic gradients in float64 -> (grad_fg, grad_env (N,4,H,W), grad_theta (V,6), abs_theta (V,6): per sum, the sum of the
    magnitudes of its terms)."""
    fg, env, imgs = (np.asarray(a, dtype=np.float64) for a in (fg, env, imgs))
    n_rows = len(np.asarray(theta))
    rec, _, comp, _ = forward64(fg, env, imgs, m, theta, ids, scale)
    t = rows64(theta, ids)
    gain = np.exp(t[:, :3])[:, :, None, None]
    mm = 1.0 if m is None else np.asarray(m, dtype=np.float64)
    dp = 2 * scale * upstream * mm * (rec - imgs) + (0.0 if x is None else np.asarray(x, dtype=np.float64))
    d = gain * dp
    a = fg[:, 3:4]
    gfg = np.concatenate([d * a, (d * (fg[:, :3] - env[:, :3])).sum(1, keepdims=True)], 1)
    genv = np.concatenate([d * (1 - a), np.zeros_like(a)], 1)
    terms = np.concatenate([dp * gain * comp, dp], 1)                                # (N,6,H,W)
    gth, ath = np.zeros((n_rows, 6)), np.zeros((n_rows, 6))
    for n, i in enumerate(np.asarray(ids).astype(np.int64)):
        if 0 <= i < n_rows:
            gth[i] += terms[n].sum((1, 2))
            ath[i] += np.abs(terms[n]).sum((1, 2))
    return gfg, genv, gth, ath


def reference(c, with_extra, ids=None):
    """The float64 reference of a case: dict(rec, value, gfg, genv, gth, ath), cached on the case."""
    key = ('ref', with_extra, None if ids is None else tuple(int(i) for i in ids))
    if key not in c:
        ids_ = _np(c['ids']) if ids is None else np.asarray(ids)
        args = (_np(c['fg']), _np(c['env']), _np(c['imgs']), _np(c['m']))
        rec, value, _, _ = forward64(*args, _np(c['theta']), ids_, c['scale'])
        gfg, genv, gth, ath = backward64(*args, _np(c['x']) if with_extra else None, _np(c['theta']), ids_, c['scale'])
        c[key] = dict(rec=rec, value=value, gfg=gfg, genv=genv, gth=gth, ath=ath)
    return c[key]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def host(c, with_extra, theta=None, ids=None, upstream=UPSTREAM, backward=True):
    """dbw_monitor_exposure_composite on the CPU through the host build -> (rec fp32, value float, grad_fg, grad_env fp32, grad_theta
    (V,6) float64 or None)."""
    fg, env, imgs = (c[k].float().contiguous() for k in ('fg', 'env', 'imgs'))
    m = None if c['m'] is None else c['m'].float().contiguous()
    x = c['x'].float().contiguous() if with_extra else None
    theta = (c['theta'] if theta is None else theta).float().contiguous()
    ids = (c['ids'] if ids is None else ids).to(torch.int32).contiguous()
    N, _, H, W = fg.shape
    rec, value = torch.full_like(imgs, float('nan')), torch.full((1,), -1.0, dtype=torch.float64)
    gfg = torch.full_like(fg, float('nan')) if backward else None
    genv = torch.full_like(env, float('nan')) if backward else None
    gth = torch.zeros(theta.shape, dtype=torch.float64) if backward else None
    rc = host_lib('exposure_math').host_exposure_composite(_p(fg), _p(env), _p(imgs), _p(m), _p(theta), _p(ids), N, H, W, theta.shape[0],
                                                           ctypes.c_double(c['scale']), _p(rec), _p(value), ctypes.c_float(upstream), _p(x), _p(gfg),
                                                           _p(genv), _p(gth))
    assert rc == 0
    return rec, value.item(), gfg, genv, gth
