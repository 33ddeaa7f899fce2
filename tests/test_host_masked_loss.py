"""CPU tests of the masked image terms: the arithmetic csrc/masked_loss.hip and csrc/ssim_term.hip compile -- csrc/loss_math.h:
masked_composite_pixel, csrc/score_math.h under a mask -- and the predicate of dbw_lens_valid_u8 (csrc/lens_math.h: lens_valid), built for
the host by g++ (tests/host_masked_loss.cpp) and held to float64 (tests/masked_loss_ref.py has oracles, inputs and bars).

SSIM term: the five shapes of ssim_term_ref.SHAPES x {noise, equal, black} x the masks {ones, holes, fraction, ring, empty}.  Properties on
the host build: overwriting rec and imgs where m = 0 changes no bit of value or gradient; the gradient is exactly 0 there; an empty mask
gives 0 and 0; a mask of ones gives the plain host term's gradient (and value) bit for bit.  Composite: the same masks on the same shapes
and on 3x40x100, with and without a gradient sent to rec.  The same file runs once as a program of its own under
-fsanitize=address,undefined.  Lens predicate: against dataset.lens_source in float64 on lens_ref.COEFFS x lens_ref.SHAPES at zoom 1."""
import subprocess

import numpy as np
import pytest
import torch

import lens_ref as LR
import masked_loss_ref as MR
import ssim_term_ref as TR
from dbw_amd import dataset, metrics, ops

IDS = [MR.case_id(c) for c in MR.CASES]


@pytest.mark.parametrize('kind,mkind,shape', MR.CASES, ids=IDS)
def test_ssim_term_against_fp64(kind, mkind, shape):
    c = MR.case(kind, mkind, shape)
    value, grad = MR.term_host(c['a'], c['b'], c['m'])
    MR.check(f'host {MR.case_id((kind, mkind, shape))}', c, value, grad)
    value0, none = MR.term_host(c['a'], c['b'], c['m'], with_grad=False)
    assert none is None and value0 == value
    invalid = (c['m'] == 0).expand_as(grad)
    assert not grad[invalid].any()                                                     # exactly 0 where m = 0
    # what rec and imgs hold where m = 0 reaches nothing
    value_r, grad_r = MR.term_host(MR.repaint(c['a'], c['m'], 1), MR.repaint(c['b'], c['m'], 2), c['m'])
    assert value_r == value and torch.equal(grad_r, grad)
    if mkind == 'empty':
        assert value == 0.0 and c['count'] == 0.0 and not grad.any()
    if mkind == 'ones':                                                                # every product by 1.0f is exact: the plain term
        plain_v, plain_g, _ = TR.term_host(c['a'], c['b'])
        assert c['count'] == c['a'].numel() and value == plain_v and torch.equal(grad, plain_g)
    if kind == 'equal':
        assert value == 0.0 and not grad.any()


def test_the_oracle_has_the_properties_the_definition_claims():
    """The float64 formula itself, on the largest shape: independent of invalid content to the bit, zero gradient on invalid pixels, the
    plain term for a mask of ones."""
    c = MR.case('noise', 'holes', (1, 48, 96))
    v, g = MR.term_torch(MR.repaint(c['a'], c['m'], 3), MR.repaint(c['b'], c['m'], 4), c['m'], torch.float64)
    assert v.item() == c['v64'] and torch.equal(g, c['g64']) and not g[(c['m'] == 0).expand_as(g)].any()
    o = MR.case('noise', 'ones', (1, 48, 96))
    plain = TR.case('noise', (1, 48, 96))
    assert abs(o['v64'] - plain['v64']) < 1e-15 and (o['g64'] - plain['g64']).abs().max().item() < 1e-18


@pytest.mark.parametrize('mkind,shape', MR.COMPOSITE_CASES, ids=[f'{m}_{s[0]}x{s[1]}x{s[2]}' for m, s in MR.COMPOSITE_CASES])
def test_composite_against_fp64(mkind, shape):
    c = MR.composite_case(mkind, shape)
    for extra in (False, True):
        rec, value, gfg, genv = MR.composite_host(c, extra)
        MR.composite_check(f'host composite {mkind} {shape} extra={extra}', c, extra, rec, value, gfg, genv)
        assert bool(torch.isfinite(gfg).all()) and bool(torch.isfinite(genv).all()) and not genv[:, 3].any()
    # without a gradient sent to rec, an invalid pixel sends none to the layers; its target reaches nothing
    rec, value, gfg, genv = MR.composite_host(c, False)
    invalid = (c['m'] == 0)
    assert not gfg[invalid.expand_as(gfg)].any() and not genv[invalid.expand_as(genv)].any()
    c2 = dict(c, imgs=MR.repaint(c['imgs'], c['m'], 5))
    rec2, value2, gfg2, genv2 = MR.composite_host(c2, True)
    rec1, value1, gfg1, genv1 = MR.composite_host(c, True)
    assert value2 == value1 and torch.equal(rec2, rec1) and torch.equal(gfg2, gfg1) and torch.equal(genv2, genv1)
    if mkind == 'empty':
        assert value == 0.0 and c['scale'] == 0.0


def test_composite_scales_by_the_upstream_scalar():
    c = MR.composite_case('holes', (2, 19, 37))
    _, _, g1, e1 = MR.composite_host(c, False, upstream=1.0)
    _, _, g2, e2 = MR.composite_host(c, False, upstream=2.0)                           # (a power of two: exact)
    assert torch.equal(g2, 2 * g1) and torch.equal(e2, 2 * e1)
    _, _, g0, e0 = MR.composite_host(c, True, upstream=0.0)                            # the scalar's gradient 0: what rec receives alone
    x, a = c['x'], c['fg'][:, 3:4]
    assert torch.equal(g0[:, :3], x * a) and torch.equal(e0[:, :3], x * (1 - a))


def test_sanitized_program_runs_clean():
    r = subprocess.run([MR.sanitized_program()], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.count(': ok') == len(MR.SHAPES)


def test_ops_torch_formula_on_cpu_tensors():
    """What the kernel does not take goes through the torch formula: CPU tensors here."""
    c = MR.case('noise', 'holes', (2, 19, 37))
    b = c['b'].clone().requires_grad_(True)
    v = ops.ssim_term(c['a'], b, masks=c['m'])                                          # count=None: one masks.sum()
    g, = torch.autograd.grad(v, b)
    assert abs(v.item() - c['v64']) <= max(c['tol_v'], 1e-6) and torch.equal(g, c['g32'])
    assert torch.equal(metrics.SSIMTerm()(c['a'], c['b'], masks=c['m'], count=c['count']), v.detach()) and metrics.SSIMTerm.takes_masks
    e = MR.case('noise', 'empty', (2, 19, 37))
    b = e['b'].clone().requires_grad_(True)
    v = ops.ssim_term(e['a'], b, masks=e['m'], count=0.0)
    g, = torch.autograd.grad(v, b)
    assert v.item() == 0.0 and not g.any()
    plain = ops.ssim_term(c['a'], c['b'])                                               # masks=None: today's path
    assert torch.equal(plain, (1 - metrics.ssim_map(c['a'], c['b'], padding=True)).mean())


@pytest.mark.parametrize('coeffs', LR.COEFFS, ids=['pincushion', 'barrel', 'mixed'])
@pytest.mark.parametrize('H,W', LR.SHAPES)
def test_lens_valid_against_fp64(coeffs, H, W):
    intr = LR.intrinsics(H, W)
    got = MR.lens_valid_host(H, W, LR.lens_array(intr, coeffs, 1.0))
    assert set(np.unique(got)) <= {0, 255}
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    u, v = dataset.lens_source(H, W, intr, coeffs, 1.0, i, j)
    want = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
    band = 64 * 2.0 ** -23 * max(H, W)                  # fp32 against fp64 within this many pixels of a frame edge: either answer
    near = (np.minimum(np.abs(u), np.abs(u - (W - 1))) < band) | (np.minimum(np.abs(v), np.abs(v - (H - 1))) < band)
    share = want.mean()
    print(f'{H}x{W} {coeffs}: valid share {share:.3f}, {int(near.sum())} pixels within {band:.2e} px of an edge')
    assert near.sum() <= 0.01 * H * W
    assert np.array_equal((got == 255)[~near], want[~near])
    assert share == 1.0 or 0.5 < share < 0.99            # (both outcomes occur over the six cases: see test below)


def test_lens_valid_has_both_outcomes_and_takes_nan():
    shares = []
    for coeffs in LR.COEFFS:
        H, W = LR.SHAPES[0]
        shares.append((MR.lens_valid_host(H, W, LR.lens_array(LR.intrinsics(H, W), coeffs, 1.0)) == 255).mean())
    assert any(s == 1.0 for s in shares) and any(s < 0.95 for s in shares), shares
    lens = LR.lens_array(LR.intrinsics(24, 32), LR.COEFFS[0], 1.0)
    lens[6] = np.nan                                     # a NaN coordinate is invalid, not a fault
    assert not MR.lens_valid_host(24, 32, lens).any()
