"""The float64 reference of the perceptual head (tests/lpips_head_ref.py) that the kernel tests compare csrc/lpips_head.hip with, checked
on the CPU: its closed-form gradient against float64 autograd of the plain formulation, its convention on an all-zero pixel (where autograd
gives NaN), and its value against the frozen fixture of the whole criterion (tests/golden/lpips_random.npz)."""
import os

import numpy as np
import pytest
import torch

import lpips_ref as L                                   # oracle/ (checker only)
import lpips_head_ref as R


def _case(C, N=3, V=4, h=7, w=9, seed=0):
    g = torch.Generator().manual_seed(seed + C)
    f = torch.relu(torch.randn(N, C, h, w, generator=g, dtype=torch.float64) * 0.5 + 0.1)
    if C < 16:
        f = f + 0.02          # (three channels behind a ReLU are all zero at one pixel in ten: those are the next test's)
    a = R.unit(torch.relu(torch.randn(V, C, h, w, generator=g, dtype=torch.float64) * 0.5 + 0.1))
    wt = torch.rand(C, generator=g, dtype=torch.float64) * 4.0 / C
    wt[::5] = 0.0
    gv = torch.tensor([1.5, -0.7, 0.0], dtype=torch.float64)[:N]
    ids = torch.tensor([3, 0, 3])[:N]
    return f, a, wt, gv, ids


def _autograd(f, a, wt, gv, ids):
    x = f.clone().requires_grad_(True)
    v = R.plain_value(x, a, wt, ids)
    gr, = torch.autograd.grad((v * gv).sum(), x)
    return v.detach(), gr


@pytest.mark.parametrize('with_ids', [False, True])
@pytest.mark.parametrize('C', [3, 64, 128, 512])
def test_closed_form_equals_float64_autograd_of_the_plain_formulation(C, with_ids):
    f, a, wt, gv, ids = _case(C)
    ids = ids if with_ids else None
    assert not bool(R.zero_pixels(f).any())
    v, gr = _autograd(f, a, wt, gv, ids)
    assert float((R.head_value(f, a, wt, ids) - v).abs().max()) <= 1e-12 * float(v.abs().max())
    got = R.head_grad(f, a, wt, gv, ids)
    assert got.shape == f.shape and got.dtype == torch.float64
    assert float((got - gr).abs().max()) <= 1e-12 * float(gr.abs().max())
    assert float(got[2].abs().max()) == 0.0          # (grad_value 0)
    # float32 inputs are read as they are and evaluated in double
    got32 = R.head_grad(f.float(), a.float(), wt.float(), gv.float(), ids)
    assert got32.dtype == torch.float64 and float((got32 - gr).abs().max()) <= 1e-6 * float(gr.abs().max())


@pytest.mark.parametrize('C', [64, 512])
def test_all_zero_pixel_autograd_gives_nan_there_and_the_closed_form_the_r_q_term(C):
    f, a, wt, gv, _ = _case(C)
    spots = [(0, 0, 0), (1, 6, 8), (1, 6, 5)]          # first pixel, last pixel, inside the last group of four
    for n, y, x in spots:
        f[n, :, y, x] = 0.0
    v, gr = _autograd(f, a, wt, gv, None)
    zero = R.zero_pixels(f)
    assert int(zero.sum()) == len(spots)
    nan = torch.isnan(gr)
    assert torch.equal(nan, zero[:, None].expand_as(nan)) and int(nan.sum()) == len(spots) * C          # exactly the C entries of each
    got = R.head_grad(f, a, wt, gv)
    assert bool(torch.isfinite(got).all())
    rest = ~nan
    assert float((got[rest] - gr[rest]).abs().max()) <= 1e-12 * float(gr[rest].abs().max())
    HW = f.shape[2] * f.shape[3]
    for n, y, x in spots:          # r q with f = 0: r = 1 / 1e-10, q = -2 w a
        want = float(gv[n]) / HW * (1.0 / R.EPS) * (-2.0 * wt * a[n, :, y, x])
        assert float((got[n, :, y, x] - want).abs().max()) <= 1e-14 * float(want.abs().max())
        # ~1e10 x the gradient elsewhere: such a pixel has to be compared apart from the rest of its image
        assert float(want.abs().max()) > 1e8 * float(gr[n][rest[n]].abs().max())
    assert torch.isfinite(v).all() and float((R.head_value(f, a, wt) - v).abs().max()) <= 1e-12 * float(v.abs().max())


def test_head_errors_gives_each_pixel_its_own_scale_and_sees_nan():
    f, a, wt, gv, _ = _case(64)
    f, a, wt, gv = f.float(), a.float(), wt.float(), gv.float()
    f[0, :, 0, 0] = 0.0
    a[2] = R.unit(f[2:3].double())[0].float()          # image 2: identical pair
    gv[2] = 2.0
    v, gr = R.head_value(f, a, wt), R.head_grad(f, a, wt, gv)
    e = R.head_errors(v.float(), gr.float(), f, a, wt, gv, identical=(2,))
    assert e['zero_pixels'] == 1 and e['nan_elems'] == 0
    assert 0 < e['value'] < 1e-7 and 0 < e['grad'] < 1e-7 and 0 < e['zero_grad'] < 1e-7          # float32 rounding of the reference itself
    # an error of 1e-3 of ITS pixel on the pixel with the smallest gradient: far below 1e-5 of the image's largest entry, seen all the same
    pix = gr[1].abs().amax(0)
    y, x = divmod(int(pix.argmin()), pix.shape[1])
    bad = gr.clone()
    bad[1, :, y, x] *= 1.0 + 1e-3
    e = R.head_errors(v.float(), bad.float(), f, a, wt, gv, identical=(2,))
    want = 1e-3 * float(pix[y, x] / (pix[y, x] + 1e-2 * pix.max()))
    assert 0.9 * want < e['grad'] < 1.1 * want
    # the zero pixel against its own scale, not the image's
    bad = gr.clone()
    bad[0, :, 0, 0] *= 1.0 + 1e-4
    e = R.head_errors(v.float(), bad.float(), f, a, wt, gv, identical=(2,))
    assert 0.9e-4 < e['zero_grad'] < 1.1e-4 and e['grad'] < 1e-7
    bad = gr.float().clone()
    bad[1, 5, 3, 3] = float('nan')
    e = R.head_errors(v.float(), bad, f, a, wt, gv, identical=(2,))
    assert e['grad'] != e['grad'] and e['nan_elems'] == 1 and not e['grad'] <= 1e-5


def test_sum_of_head_values_over_the_taps_reproduces_the_fixture(golden_dir):
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(golden_dir, 'lpips_random.npz')).items()}
    vgg, lin = L.random_weights(int(g['seed']), torch.float64)
    shift = torch.tensor(L.SHIFT, dtype=torch.float64)[None, :, None, None]
    scale = torch.tensor(L.SCALE, dtype=torch.float64)[None, :, None, None]
    fa = L.vgg16_taps((2 * g['imgs'].double() - 1 - shift) / scale, vgg)
    fb = L.vgg16_taps((2 * g['rec'].double() - 1 - shift) / scale, vgg)
    per = sum(R.head_value(fb[k], R.unit(fa[k]), lin[f'lin{k}.model.1.weight'].view(-1)) for k in range(5))
    assert per.dtype == torch.float64
    assert torch.allclose(per, g['per_sample'].view(-1), rtol=1e-12, atol=0)
