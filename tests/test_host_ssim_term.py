"""CPU tests of the arithmetic of the SSIM term (csrc/score_math.h: ssim_deriv, ssim_grad_pixel beside the filters of the image scores --
the header ssim_term_kernel compiles) built for the host with g++ -ffp-contract=off (tests/host_ssim_term.cpp), on whole small images:
  * value and gradient against the 2-D 11 x 11 definition evaluated in float64 under torch autograd (ssim_term_ref.term_fp64_2d), on
    every shape and input kind of the GPU test, within the bar of ssim_term_ref: 4 x the error of torch's fp32 evaluation of the same
    input, floors of 1e-6 relative (value) and 1e-6 * max(max|g64|, 1/M) (gradient).  Measured, the worst case of each kind over the five
    shapes (blocks: the fixture's pair), as "value / gradient" error, host build against torch fp32:
        noise   6.1e-9 / 5.1e-9    against  3.8e-8 / 1.0e-8        blocks  2.1e-7 / 5.8e-8   against  4.5e-6 / 1.3e-7
        equal   0 / 0 (exactly)    against  0 / 8.2e-9             black   4.3e-11 / 1.0e-8  against  3.4e-9 / 1.1e-8
    Constant blocks without noise at the other four shapes were tried and are not cases: there the value's error is the rounding of the
    products a*a, b*b, a*b of a constant region, the same for every pixel of the region (about 3e-8 of v^2 against C2 = 9e-4), which
    torch's fp32 evaluation carries too; which of the two lands closer to float64 is chance (host 5e-7 .. 3.9e-6 against torch
    3.8e-7 .. 5.7e-6; at 1x3x48x96 the host's 3.9e-6 stood against a torch error of 3.8e-7).
  * rec == target gives the value 0 and a gradient of exactly 0; S of ssim_deriv is ssim_pixel's bit for bit; the map and the value agree
    with the host build of the image scores (padding = 1);
  * tests/golden/ssim_term.npz -- the reference's own SSIMLoss().mean() and its autograd gradient -- within the reference's own fp32 error
    against float64 plus the bar above; metrics.SSIMTerm on CPU tensors (the torch formula) against the same fixture;
  * a program of its own runs the same host code under -fsanitize=address,undefined."""
import os
import subprocess

import pytest
import torch

import score_ref as SR
import ssim_term_ref as TR
from dbw_amd import metrics

_id = TR.case_id


@pytest.mark.parametrize('kind,shape', TR.CASES, ids=[_id(c) for c in TR.CASES])
def test_value_and_gradient_against_fp64(kind, shape):
    a, b = TR.pair(kind, shape)
    v64, g64 = TR.term_fp64_2d(a, b)
    v32, g32 = TR.term_torch(a, b, torch.float32)
    c = dict(v64=v64.item(), g64=g64, **TR.bars(v64.item(), g64, v32.double().item(), g32))
    value, grad, _ = TR.term_host(a, b)
    TR.check(f'host {_id((kind, shape))}', c, value, grad)
    value0, none, _ = TR.term_host(a, b, with_grad=False)
    assert none is None and value0 == value


@pytest.mark.parametrize('shape', TR.SHAPES, ids=[f'{n}x3x{h}x{w}' for n, h, w in TR.SHAPES])
def test_identical_images_are_the_minimum(shape):
    a, b = TR.pair('equal', shape)
    value, grad, m = TR.term_host(a, b)
    assert value == 0.0 and torch.equal(m, torch.ones_like(m)) and not grad.any()


def test_map_and_value_are_those_of_the_image_scores():
    a, b = TR.pair('noise', (2, 19, 37))
    value, _, m = TR.term_host(a, b)
    out, m_scores = SR.image_scores_host(a, b, padding=True)
    assert torch.equal(m, m_scores)                                   # ssim_deriv's S is ssim_pixel's, bit for bit
    assert abs(value - (1 - out[:, 1].sum().item() / m.numel())) < 1e-6     # (the term forms 1 - S in fp64 from the statistics)
    lib = TR.host_lib('ssim_term')
    stats = torch.rand(1000, 5, generator=torch.Generator().manual_seed(3))
    assert all(lib.host_ssim_deriv_matches_pixel(TR._p(row)) == 1 for row in stats)


def test_golden_fixture_host_build(golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, 'ssim_term.npz')) < 200 * 1024
    for name, a, b, ref_v, ref_g in TR.fixture_pairs(golden_dir):
        value, grad, _ = TR.term_host(a, b)
        TR.fixture_check(f'host, {name}', a, b, ref_v, ref_g, value, grad)
        if name == 'blocks':
            assert all(torch.equal(x, y) for x, y in zip((a, b), TR.pair(*TR.BLOCKS)))
            assert torch.equal(a[0], b[0]) and not ref_g[0].abs().max() > 1e-6 and not grad[0].any()


def test_golden_fixture_module_on_cpu(golden_dir):
    term = metrics.SSIMTerm()
    assert not list(term.parameters()) and not hasattr(term, 'cache_targets') and not hasattr(term, 'target_cache')
    for name, a, b, ref_v, ref_g in TR.fixture_pairs(golden_dir):
        rec = b.clone().requires_grad_(True)
        v = term(a, rec)
        assert v.dim() == 0 and v.dtype == torch.float32
        v.backward()
        TR.fixture_check(f'SSIMTerm on the CPU, {name}', a, b, ref_v, ref_g, v.item(), rec.grad)


def test_host_code_is_clean_under_the_sanitizers():
    r = subprocess.run([TR.sanitized_program()], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.count(': ok') == len(TR.SHAPES) and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr
