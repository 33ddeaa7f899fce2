"""CPU tests of the arithmetic of the image scores (csrc/score_math.h, the header image_scores_kernel compiles) built for the host with
g++ -ffp-contract=off (tests/host_score_math.cpp):
  * on tests/golden/ssim.npz -- the reference's own SSIMLoss -- the map is within 2e-5 per pixel and the per-image mean within 1e-6, both
    paddings: the bars tests/test_host_logic.py holds metrics.ssim_map to on this fixture.  Measured: 4.59e-6 and 9.43e-8.
  * against the 2-D 11 x 11 definition evaluated in fp64 (score_ref.ssim_map_fp64), on seeded noise pairs and on a render-like pair, the
    error is at most TWICE what metrics.ssim_map (per pixel) and metrics.ssim (per-image mean) leave against the same arbiter on the same
    input.  The factor 2 covers another order of the same fp32 operations; a wrong tap or halo is off by orders more.  torch's side of
    the MEAN is metrics.ssim, the project's per-image mean: an fp32 mean of the fp32 map, so the bar holds that reduction's error too
    (1.8e-9 .. 1.0e-7 on these inputs); the header's side is the fp64 sum of its fp32 map over the count, as the kernel returns it.
    Against the fp64 mean of metrics.ssim_map instead the header meets 2x in 9 of the 10 noise / render cases and misses (23,37) with
    padding, where torch's own error happens to cancel to 9e-11, below what a mean of fp32 values resolves.  Measured, as
    "per pixel / mean", header against torch:
        noise (11,11), (12,16), (23,37), (37,70), the worse padding: 4.2e-7 / 5.8e-9, 6.5e-7 / 5.7e-9, 7.4e-7 / 2.6e-9, 9.9e-7 / 1.3e-9
                                                      against torch's    5.7e-7 / 1.0e-7, 1.2e-6 / 7.6e-8, 1.3e-6 / 1.1e-8, 1.8e-6 / 4.9e-9
        render-like (48,64): 2.1e-4 / 3.6e-7 against torch's 4.1e-4 / 6.1e-7 (flat regions cancel in E[x^2] - mu^2 over C2 = 9e-4)
    (the header's filters are compensated dot products, csrc/score_math.h; (11,11) without padding is ONE window, where the header's
    1.8e-7 stands against torch's 1.2e-7: one fp32 rounding of a value near 0.02 either way)
  * the squared-error sum equals numpy's fp64 sum within 1e-12 relative; identical constant images give a map of exactly 1; H = 10 without
    padding is refused; a program of its own runs the same host code under -fsanitize=address,undefined."""
import subprocess

import numpy as np
import pytest
import torch

import score_ref as SR
from dbw_amd import metrics

CASES = [f'noise_{h}x{w}' for h, w in SR.NOISE_SHAPES] + ['render']


def test_window_is_the_one_of_metrics():
    assert torch.equal(SR.window_host(), metrics.gaussian_window())


def test_golden_fixture(golden_dir):
    import os
    g = np.load(os.path.join(golden_dir, 'ssim.npz'))
    a, b = torch.from_numpy(g['img1']), torch.from_numpy(g['img2'])
    for pad in (0, 1):
        out, m = SR.image_scores_host(a, b, bool(pad))
        assert m.shape == g[f'ssim_map_pad{pad}'].shape
        e_map = np.abs(m.numpy() - g[f'ssim_map_pad{pad}']).max()
        e_mean = np.abs((1 - out[:, 1] / m[0].numel()).numpy() - g[f'one_minus_ssim_pad{pad}']).max()
        print(f'golden, padding {pad}: map {e_map:.3e}, mean {e_mean:.3e}')
        assert e_map < 2e-5 and e_mean < 1e-6


@pytest.mark.parametrize('pad', [0, 1])
@pytest.mark.parametrize('name', CASES)
def test_fp64_arbiter(name, pad):
    c = SR.case(name)
    a, b = c['a'], c['b']
    ref = SR.ssim_map_fp64(a, b, bool(pad))
    ref_mean = ref.flatten(1).mean(1)
    t_map = (metrics.ssim_map(a, b, padding=bool(pad)).double() - ref).abs().max().item()
    t_mean = (metrics.ssim(a, b, padding=bool(pad)).double() - ref_mean).abs().max().item()
    h_map = (c[f'host_map{pad}'].double() - ref).abs().max().item()
    h_mean = (c[f'host_out{pad}'][:, 1] / ref[0].numel() - ref_mean).abs().max().item()
    print(f'{name}, padding {pad}: per pixel {h_map:.3e} (torch {t_map:.3e}), mean {h_mean:.3e} (torch {t_mean:.3e})')
    assert c[f'host_map{pad}'].shape == ref.shape
    assert h_map <= 2 * t_map and h_mean <= 2 * t_mean


@pytest.mark.parametrize('name', CASES)
def test_squared_error_sum(name):
    c = SR.case(name)
    want = ((c['a'].numpy().astype(np.float64) - c['b'].numpy().astype(np.float64)) ** 2).reshape(c['a'].shape[0], -1).sum(1)
    for pad in (0, 1):
        assert np.abs(c[f'host_out{pad}'][:, 0].numpy() / want - 1).max() < 1e-12


def test_constant_images_give_exactly_one():
    for v in (0.0, 0.25, 0.7, 1.0):
        a = torch.full((1, 3, 14, 19), v)
        out, m = SR.image_scores_host(a, a, padding=False)
        assert torch.equal(m, torch.ones_like(m)) and out[0, 0] == 0 and out[0, 1] == m.numel()
    a = torch.full((1, 3, 14, 19), 0.4)
    _, m = SR.image_scores_host(a, a, padding=True)
    assert torch.equal(m, torch.ones_like(m))           # (identical images: numerator and denominator are the same floats at the border too)


def test_refusals():
    a = torch.zeros(1, 3, 10, 16)
    with pytest.raises(ValueError):
        SR.image_scores_host(a, a, padding=False)
    with pytest.raises(ValueError):
        SR.image_scores_host(a.transpose(2, 3), a.transpose(2, 3), padding=False)
    out, m = SR.image_scores_host(a, a, padding=True)
    assert m.shape == (1, 3, 10, 16)


def test_host_code_is_clean_under_the_sanitizers():
    r = subprocess.run([SR.sanitized_program()], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.count(': ok') == 12 and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr
