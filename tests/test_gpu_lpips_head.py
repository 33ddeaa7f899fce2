"""csrc/lpips_head.hip: dbw_lpips_head_fwd / _bwd called through the C ABI with raw pointers (alignment and view ids chosen freely, outputs
prefilled with NaN so that an unwritten element shows) against the float64 reference of tests/lpips_head_ref.py evaluated on the same
float32 inputs, in all three instantiations the launcher picks from:

    small    N HW < 65536                                        16 pixels x 16 channel groups, sums meet in LDS
    vector   otherwise, HW % 4 == 0 and every base 16-byte aligned   a thread owns 4 pixels (the two largest taps of a 400x300 batch)
    scalar   otherwise                                            a pixel per thread

Which one a case reached is asserted from the outside (`_forward_variant`): dbw_lpips_head_blocks(N, HW) == ceil(HW / 16) is the small
one; otherwise the vector launch leaves the partials of the workgroups beyond ceil(HW / 1024) at exactly 0 and the scalar one leaves none
at 0.  The backward has no such trace: its variant follows from the same rule with grad_feat's alignment added, and the case with only
grad_feat 4 bytes off a 16-byte boundary runs the vector forward and the scalar backward on the same inputs.

THE BAR is not a chosen number.  Per family (variant x synthetic / real taps) torch's own float32 formulation -- the non-fused branch of
LPIPSVGG.forward, lin((na - unit(fb))^2).mean((2,3)) and its autograd -- was run on the MI355X on the same inputs and measured against the
same float64 reference with the same two metrics (lpips_head_ref.head_errors: the value per image relative to itself, the gradient per
element relative to max_c |g64| of ITS pixel + 1e-2 of the image's largest entry).  The kernel's bar is 8 x the largest such error of the
family's cases -- a thread accumulates up to 128 channels serially in one float32 register where torch sums pairwise: random-walk growth
~ sqrt(128 / log2 128) ~ 4, doubled for headroom -- and never looser than the 1e-5 of tests/test_lpips.py.  Every case measures torch
again next to the kernel and records both (record_property).  Measured on the MI355X (largest of the family's cases):

    family               torch fp32 value / gradient      kernel value / gradient       bar value / gradient
    synthetic, vector    4.38e-08 / 6.13e-07              9.79e-08 / 1.04e-06           3.50e-07 / 4.90e-06
    synthetic, scalar    3.80e-08 / 4.72e-07              8.30e-08 / 7.63e-07           3.04e-07 / 3.78e-06
    synthetic, small     1.37e-07 / 2.07e-06              6.93e-08 / 3.32e-06           1.10e-06 / 1.00e-05   (gradient: the 3-channel case, both sides)
    real, vector         1.09e-07 / 5.89e-07              7.08e-08 / 4.40e-06           8.72e-07 / 4.71e-06
    real, scalar         1.24e-07 / 6.47e-07              6.61e-08 / 2.57e-06           9.92e-07 / 5.18e-06
    real, small          1.31e-07 / 1.20e-06              9.54e-08 / 3.44e-06           1.05e-06 / 9.60e-06
    all-zero pixels      (NaN)                            1.54e-07                      4.77e-07 (derived below)

A FINDING the table shows: on real taps the kernel's gradient sits 4 to 8 x above torch's float32 (2 x on synthetic taps), at 7.5 x in the
production family -- inside the bar, but only just.  It is not the accumulation order.  The kernel takes q . f out of its first walk as
-2 (sum w a f - r sum w f^2), two sums that cancel where the reconstruction's unit tap is close to the target's -- as it is for a
reconstruction that resembles its target, 0.7 image + 0.3 noise here, and ever more so as training converges -- where torch sums the
differences q_c f_c themselves.  A serial-order float32 restatement of the kernel on the CPU (the network's taps at 150x200) gives 3.6e-6
with the kernel's form of q . f and 8.6e-7 with sum_c q_c f_c in the same serial order, next to 4.9e-7 for torch: the form, not the order.
Taking q . f from the differences needs r before the walk that accumulates it, a third walk over the tap: a cost the kernel does not pay.

An all-zero pixel (planted first, last and inside the last group of four; its gradient is ~1e10 x the others') is compared apart, against
its own max_c |g64|.  Torch gives NaN there, so that bar is derived: with f = 0 the kernel's value is one product with no accumulation --
the float32 roundings of 1e-10, of r = 1 / (0 + 1e-10), of 1 / HW, of grad_value / HW, of w a, of r (.) and of the final scale (.), seven
at most, each <= 2^-24 relative -- so it is held to ZERO_BAR = 8 x 2^-24 of its own size."""
import math
import os

import numpy as np
import pytest
import torch

import lpips_ref as L                                   # oracle/ (checker only)
import lpips_head_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
ZERO_BAR = 8 * 2.0 ** -24
# (family) -> torch float32 against float64 on the MI355X, (value, gradient): the largest of the family's cases (the table above)
TORCH_FP32 = {
    ('vector', 'synthetic'): (4.38e-08, 6.13e-07),
    ('scalar', 'synthetic'): (3.80e-08, 4.72e-07),
    ('small', 'synthetic'): (1.37e-07, 2.07e-06),
    ('vector', 'real'): (1.09e-07, 5.89e-07),
    ('scalar', 'real'): (1.24e-07, 6.47e-07),
    ('small', 'real'): (1.31e-07, 1.20e-06),
}


def bar(variant, kind, which):
    return min(8.0 * TORCH_FP32[(variant, kind)][which], 1e-5)


def _at_offset(t, k):
    """A contiguous copy of t that starts k floats behind a 16-byte aligned address."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * k) % 16
    return v


def run_head(f, a, w, g, ids, gf_off=0):
    """-> (partial (N, blocks), grad_feat (N,C,h,w)), both prefilled with NaN"""
    from dbw_amd import _lib
    N, C, h, wd = f.shape
    assert all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in (f, a, w, g)) and a.shape[1:] == f.shape[1:]
    assert w.shape == (C,) and g.shape == (N,) and (a.shape[0] >= N if ids is None else ids.dtype == torch.int64 and ids.shape == (N,))
    nb = _lib.load().dbw_lpips_head_blocks(N, h * wd)
    partial = torch.full((N, nb), NAN, dtype=torch.float32, device=f.device)
    gf = _at_offset(torch.full(f.shape, NAN, dtype=torch.float32, device=f.device), gf_off)
    stream = torch.cuda.current_stream().cuda_stream
    idp = ids.data_ptr() if ids is not None else 0
    _lib.call('dbw_lpips_head_fwd', f.data_ptr(), a.data_ptr(), idp, w.data_ptr(), N, a.shape[0], C, h * wd, partial.data_ptr(), stream)
    _lib.call('dbw_lpips_head_bwd', f.data_ptr(), a.data_ptr(), idp, w.data_ptr(), N, a.shape[0], C, h * wd, g.data_ptr(), gf.data_ptr(), stream)
    torch.cuda.synchronize()
    return partial, gf


def _forward_variant(partial, HW, rows):
    """Which instantiation wrote `partial` (rows: images with w > 0 somewhere and a target that differs from the reconstruction)"""
    nb = partial.shape[1]
    if nb == math.ceil(HW / 16):
        return 'small'
    assert nb == math.ceil(HW / 256)
    p = partial[rows]
    active = math.ceil(HW / 1024)
    if active < nb and bool((p[:, active:] == 0).all()) and bool((p[:, :active] != 0).all()):
        return 'vector'
    if bool((p != 0).all()):
        return 'scalar'
    raise AssertionError('neither the vector nor the scalar pattern of partial sums')


def _backward_variant(f, a, gf):
    N, HW = f.shape[0], f.shape[2] * f.shape[3]
    if N * HW < 65536:
        return 'small'
    return 'vector' if HW % 4 == 0 and all(t.data_ptr() % 16 == 0 for t in (f, a, gf)) else 'scalar'


def torch_fp32(f, a, w, g, ids):
    """The float32 formulation torch runs on the same inputs: (values, gradient of sum_n g[n] value[n])"""
    x = f.detach().clone().requires_grad_(True)
    v = R.plain_value(x, a, w, ids)
    gr, = torch.autograd.grad((v * g).sum(), x)
    return v.detach(), gr


def measure_case(f, a, w, g, ids=None, identical=(), gf_off=0):
    """Run the kernels and torch's float32 formulation on one case -> dict: the variants reached and both sides' errors against float64"""
    partial, gf = run_head(f, a, w, g, ids, gf_off)
    others = [n for n in range(f.shape[0]) if n not in identical]
    m = {'fwd': _forward_variant(partial, f.shape[2] * f.shape[3], others), 'bwd': _backward_variant(f, a, gf)}
    m['kernel'] = R.head_errors(partial.sum(1), gf, f, a, w, g, ids, identical)
    del partial, gf
    vt, gt = torch_fp32(f, a, w, g, ids)
    m['torch'] = R.head_errors(vt, gt, f, a, w, g, ids, identical)
    return m


def check_case(name, kind, expect, f, a, w, g, ids=None, identical=(), gf_off=0, record=None, planted=None):
    """expect: (forward variant, backward variant).  Prints and records every figure -> the list of what is wrong (empty: nothing)."""
    m = measure_case(f, a, w, g, ids, identical, gf_off)
    k, t = m['kernel'], m['torch']
    bars = {'value': bar(expect[0], kind, 0), 'grad': bar(expect[1], kind, 1), 'zero_grad': ZERO_BAR}
    print(f'{name} [{kind}] fwd {m["fwd"]} bwd {m["bwd"]}: kernel value {k["value"]:.3g} grad {k["grad"]:.3g} zero-pixel grad {k["zero_grad"]:.3g} '
          f'({k["zero_pixels"]} zero pixels) | torch fp32 value {t["value"]:.3g} grad {t["grad"]:.3g} | bars {bars["value"]:.3g} {bars["grad"]:.3g} {ZERO_BAR:.3g}')
    if record is not None:
        for key in ('value', 'grad', 'zero_grad'):
            record(f'{name}.kernel_{key}', k[key])
            record(f'{name}.bar_{key}', bars[key])
        record(f'{name}.torch_fp32_value', t['value'])
        record(f'{name}.torch_fp32_grad', t['grad'])
        record(f'{name}.variants', f'{m["fwd"]}/{m["bwd"]}')
    wrong = []
    if (m['fwd'], m['bwd']) != tuple(expect):
        wrong.append(f'{name}: reached {m["fwd"]} / {m["bwd"]}, not {expect[0]} / {expect[1]}')
    if planted is not None and k['zero_pixels'] != planted:
        wrong.append(f'{name}: {k["zero_pixels"]} zero pixels, {planted} planted')
    if k['nan_elems']:
        wrong.append(f'{name}: {k["nan_elems"]} elements NaN or not exactly 0 where they must be (left unwritten?)')
    for key in ('value', 'grad', 'zero_grad'):
        if not k[key] <= bars[key]:
            wrong.append(f'{name}: {key} error {k[key]:.3g} above the bar {bars[key]:.3g} (torch fp32: {t[key]:.3g})')
    return wrong


# ---- synthetic taps ---------------------------------------------------------------------------------------------------------------------
def synthetic(N, V, C, h, wd, ids=None, seed=0):
    """relu(randn 0.5 + 0.1) taps, the targets unit-normalised in float64 and rounded to float32.  Image 0 carries the all-zero pixels (first,
    last, inside the last group of four), image 1 per-pixel norms spread over 1e-3..1e3, image 2 is an identical pair (its target row is its
    own unit tap), an image 3 gets grad_value 0; grad_value of image 0 is negative; every fifth channel has w = 0.
    -> f, a, w, g, ids, identical, planted"""
    gen = torch.Generator(device=DEV).manual_seed(1000 + seed)

    def tap(n):
        return torch.relu(torch.randn(n, C, h, wd, generator=gen, device=DEV) * 0.5 + 0.1)
    f = tap(N)
    if C < 16:
        f += 0.02          # (a handful of channels behind a ReLU are all zero at many pixels of their own: only the planted ones here)
    HW, planted = h * wd, 0
    if HW >= 8:
        for p in (0, HW - 1, HW - 3):
            f[0].view(C, HW)[:, p] = 0.0
        planted = 3
    if N >= 2:
        f[1] *= 10.0 ** (torch.rand(1, h, wd, generator=gen, device=DEV) * 6.0 - 3.0)
    a = torch.empty(V, C, h, wd, device=DEV)
    for v in range(V):
        a[v] = R.unit(tap(1).double())[0].float()
    idt = torch.tensor(ids, device=DEV, dtype=torch.int64) if ids is not None else None
    identical = ()
    if N >= 3:
        a[ids[2] if ids is not None else 2] = R.unit(f[2:3].double())[0].float()
        identical = (2,)
    w = torch.rand(C, generator=gen, device=DEV) * 4.0 / C
    w[::5] = 0.0
    if C <= 5:
        w[0], w[1] = 0.3, 0.0
    g = torch.tensor([-0.7, 1.5, 2.0, 0.0][:N], device=DEV)
    return f, a, w, g, idt, identical, planted


# (N, V, C, h, w), ids, offsets in floats of (feat, target_unit, grad_feat), expected (forward, backward) variant
CASES = {
    'vector-production-tap0': ((4, 4, 64, 300, 400), None, (0, 0, 0), ('vector', 'vector')),
    'vector-production-tap1-ids-ragged': ((4, 6, 128, 150, 200), [5, 0, 5, 2], (0, 0, 0), ('vector', 'vector')),          # 29.3 active workgroups, 88 idle
    'vector-first-size-not-small': ((1, 1, 64, 256, 256), None, (0, 0, 0), ('vector', 'vector')),
    'vector-1080x1920-tap0': ((2, 2, 64, 1080, 1920), None, (0, 0, 0), ('vector', 'vector')),
    'scalar-odd-plane': ((3, 3, 64, 149, 201), None, (0, 0, 0), ('scalar', 'scalar')),                                      # last workgroup: 253 pixels
    'scalar-feat-off-4-bytes': ((4, 4, 64, 128, 128), None, (1, 0, 0), ('scalar', 'scalar')),
    'scalar-target-off-4-bytes': ((4, 4, 64, 128, 128), None, (0, 1, 0), ('scalar', 'scalar')),
    'vector-forward-scalar-backward-grad-off-4-bytes': ((4, 4, 64, 128, 128), None, (0, 0, 1), ('vector', 'scalar')),
    'small-production-tap2': ((4, 4, 256, 75, 100), None, (0, 0, 0), ('small', 'small')),
    'small-production-tap3': ((4, 4, 512, 37, 50), None, (0, 0, 0), ('small', 'small')),
    'small-production-tap4-ids': ((4, 6, 512, 18, 25), [5, 0, 5, 2], (0, 0, 0), ('small', 'small')),
    'small-last-small-size': ((1, 1, 64, 255, 257), None, (0, 0, 0), ('small', 'small')),
    'small-3-channels': ((2, 2, 3, 33, 47), None, (0, 0, 0), ('small', 'small')),                                           # channel groups 3..15 idle
    'small-70-channels': ((3, 3, 70, 29, 31), None, (0, 0, 0), ('small', 'small')),
    'small-one-pixel': ((1, 1, 5, 1, 1), None, (0, 0, 0), ('small', 'small')),
    'small-three-pixels': ((1, 1, 5, 1, 3), None, (0, 0, 0), ('small', 'small')),
}


def synthetic_case(name):
    (N, V, C, h, wd), ids, (of, oa, og), expect = CASES[name]
    f, a, w, g, idt, identical, planted = synthetic(N, V, C, h, wd, ids, seed=sorted(CASES).index(name))
    if of:
        f = _at_offset(f, of)
    if oa:
        a = _at_offset(a, oa)
    return dict(kind='synthetic', expect=expect, f=f, a=a, w=w, g=g, ids=idt, identical=identical, gf_off=og, planted=planted)


@pytest.mark.parametrize('name', list(CASES))
def test_head_kernels_equal_the_float64_reference_on_synthetic_taps(name, record_property):
    (N, V, C, h, wd) = CASES[name][0]
    assert (N * h * wd < 65536) == (CASES[name][3][0] == 'small')
    wrong = check_case(name, record=record_property, **synthetic_case(name))
    assert not wrong, wrong
    torch.cuda.empty_cache()


# ---- real taps: what LPIPSVGG.features produces, with the sparsity behind its ReLUs ----------------------------------------------------------
REAL_SHAPES = {
    'production-4x300x400': ((4, 300, 400), ['vector', 'vector', 'small', 'small', 'small']),
    'odd-3x149x201': ((3, 149, 201), ['scalar', 'small', 'small', 'small', 'small']),
}
REAL_GRAD_VALUES = [-0.7, 1.5, 2.0, 0.25]


def fixture_net(golden_dir):
    """LPIPSVGG with the seeded weights of tests/golden/lpips_random.npz, on the device"""
    from dbw_amd.lpips_vgg import LPIPSVGG
    vgg, lin = L.random_weights(int(np.load(os.path.join(golden_dir, 'lpips_random.npz'))['seed']))
    return LPIPSVGG().load_weights(vgg, lin).to(DEV)


def check_real_taps(name, net, fb_all, target_all, ids, variants, record=None):
    """The head kernels on the taps of a batch (fb_all: the reconstruction's, target_all: the unit-normalised targets', rows `ids` of them)."""
    N = fb_all[0].shape[0]
    g = torch.tensor(REAL_GRAD_VALUES[:N], device=DEV)
    wrong = []
    for k, (fb, na, lin) in enumerate(zip(fb_all, target_all, net.lins)):
        assert fb.dtype == torch.float32 and float((fb == 0).float().mean()) > 0.05          # (the zeros of the ReLU)
        wrong += check_case(f'{name}-tap{k}', 'real', (variants[k], variants[k]), fb.detach().contiguous(), na.detach().contiguous(),
                            lin.weight.detach().reshape(-1).contiguous(), g, ids, record=record)
    assert not wrong, wrong


@pytest.mark.parametrize('name', list(REAL_SHAPES))
def test_head_kernels_equal_the_float64_reference_on_the_taps_of_the_network(name, golden_dir, record_property):
    (N, H, W), variants = REAL_SHAPES[name]
    net = fixture_net(golden_dir)
    gen = torch.Generator().manual_seed(5)
    imgs = torch.rand(N, 3, H, W, generator=gen).to(DEV)
    rec = imgs * 0.7 + 0.3 * torch.rand(N, 3, H, W, generator=gen).to(DEV)
    with torch.no_grad():
        target_all = [net._unit(t) for t in net.features(imgs * 2 - 1)]
        fb_all = net.features(rec * 2 - 1)
    check_real_taps(name, net, fb_all, target_all, None, variants, record_property)


# ---- view ids outside the cache, the empty batch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant,shape', [('vector', (4, 3, 8, 128, 128)), ('scalar', (4, 3, 8, 129, 129)), ('small', (4, 3, 8, 10, 10))])
def test_a_view_id_outside_the_cache_poisons_that_image_only(variant, shape, record_property):
    N, V, C, h, wd = shape
    f, a, w, g, _, _, _ = synthetic(N, V, C, h, wd, None, seed=99)
    a[2] = R.unit(torch.relu(torch.randn(1, C, h, wd, generator=torch.Generator(device=DEV).manual_seed(7), device=DEV) * 0.5 + 0.1).double())[0].float()          # (no identical pair here)
    g = torch.tensor([-0.7, 1.5, 2.0, 0.5], device=DEV)
    ids = torch.tensor([0, V, 2, -1], device=DEV, dtype=torch.int64)          # images 1 and 3: outside [0, V)
    partial, gf = run_head(f, a, w, g, ids)
    good, bad = [0, 2], [1, 3]
    assert _forward_variant(partial, h * wd, good) == variant == _backward_variant(f, a, gf)
    assert bool(torch.isnan(partial[bad]).all()) and bool(torch.isnan(gf[bad]).all())
    e = R.head_errors(partial[good].sum(1), gf[good], f[good].contiguous(), a, w, g[good], ids[good])
    record_property('kernel_value', e['value'])
    record_property('kernel_grad', e['grad'])
    assert e['nan_elems'] == 0 and e['value'] <= bar(variant, 'synthetic', 0) and e['grad'] <= bar(variant, 'synthetic', 1) and e['zero_grad'] <= ZERO_BAR


def test_an_empty_batch_returns_0_and_writes_nothing():
    from dbw_amd import _lib
    f = torch.rand(1, 8, 4, 4, device=DEV)
    a = R.unit(torch.rand(1, 8, 4, 4, device=DEV))
    w, g = torch.rand(8, device=DEV), torch.ones(1, device=DEV)
    ids = torch.zeros(1, dtype=torch.int64, device=DEV)
    partial = torch.full((1, 16), NAN, device=DEV)
    gf = torch.full_like(f, NAN)
    stream = torch.cuda.current_stream().cuda_stream
    for idp, V in ((0, 0), (ids.data_ptr(), 1)):          # (_lib.call raises on a return code other than 0)
        _lib.call('dbw_lpips_head_fwd', f.data_ptr(), a.data_ptr(), idp, w.data_ptr(), 0, V, 8, 16, partial.data_ptr(), stream)
        _lib.call('dbw_lpips_head_bwd', f.data_ptr(), a.data_ptr(), idp, w.data_ptr(), 0, V, 8, 16, g.data_ptr(), gf.data_ptr(), stream)
    torch.cuda.synchronize()
    assert bool(torch.isnan(partial).all()) and bool(torch.isnan(gf).all())
