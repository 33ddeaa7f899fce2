"""dbw_texbin_reduce (csrc/shade_blend.hip: texbin_reduce_kernel) on hand-built records against a float64 scatter, texel by texel,
under the bar of the kernel's own contract (tests/texbin_ref.py: bar; DESIGN.md "Texel-gradient accumulators against a float64
scatter"): every addend rounded to half a unit 2^(e - 20) of the block exponent it met, half a unit of the new exponent per rescale,
2^-21 of the sum of |g w| for the fp32 arithmetic around the tile.  The cases are built on the host (tests/test_texbin_ref_host.py
holds them to what they claim); nothing here is tuned to what the kernel returns."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import texbin_ref as T                                          # noqa: E402
from dbw_amd import _lib, ops                                   # noqa: E402

DEV = 'cuda:0'


def reduce(built, prior=None):
    """one dbw_texbin_reduce call on the case -> grad_maps (flat fp32 numpy), started from zeros or from `prior`"""
    maps = built.maps
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    info, cursor, records, layout = dev(maps.info), dev(built.cursor), dev(built.buffer), dev(built.layout.view(np.int32))
    gm = torch.zeros(maps.total, dtype=torch.float32, device=DEV) if prior is None else dev(prior.astype(np.float32))
    cap = max(len(built.buffer) // maps.nbins, built.sub)
    _lib.call('dbw_texbin_reduce', info.data_ptr(), cursor.data_ptr(), records.data_ptr(), cap, layout.data_ptr(), maps.nbins, gm.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return gm.cpu().numpy()


def hold(name, built, phases, got, record_property, prior=None):
    """every texel-channel within the bar; where no record adds anything the buffer keeps its bits"""
    ref, count = T.reference(built)
    before = np.zeros(built.maps.total, dtype=np.float32) if prior is None else prior.astype(np.float32)
    bound = T.bar(built, phases, prior)
    err = np.abs(got.astype(np.float64) - (ref + before.astype(np.float64)))
    on = count > 0
    ratio = float(np.nanmax(np.where(on, err / np.where(on, bound, 1.0), 0.0))) if np.isfinite(err).all() else float('inf')
    print(f'texbin_reduce {name}: {int(sum(len(r) for r in built.counted.values()))} records, {int(on.sum())} texel-channels, max err / bound = {ratio:.4f}')
    record_property('err_over_bound', ratio)
    assert np.array_equal(got[~on].view(np.int32), before[~on].view(np.int32))
    assert ratio <= 1.0, f'{name}: err / bound = {ratio}'
    return ratio


@pytest.fixture(scope='module')
def sub():
    return ops.bin_subcursors()


@pytest.mark.parametrize('name', sorted(T.GEOMETRY_SHAPES))
def test_geometry(name, sub, record_property):
    """One bin, four bins ragged and full, a second map behind the first (non-zero offset); halo row and halo column into the
    neighbouring tiles, one-texel footprints, weights of exactly 0 and 1."""
    built, phases = T.case_geometry(name, sub)
    hold(name, built, phases, reduce(built), record_property)


def test_counts_layout_capacity_and_adding_to_what_is_there(sub, record_property):
    """0, 1, 511, 512, 513, 1025 records per sub-range and uneven ones, a layout with gaps, cursors beyond their capacity over a buffer
    full of sentinels, an empty bin, and a gradient buffer that already holds values: the call ADDS, and texels nobody adds to keep
    their bits."""
    built, phases = T.case_counts(sub)
    prior = np.random.default_rng(3).standard_normal(built.maps.total).astype(np.float32)
    got = reduce(built, prior)
    assert np.abs(got).max() < 1e6                              # (no sentinel was read: it would be 3e30)
    hold('counts', built, phases, got, record_property, prior)
    # and on zeros: the same records, nothing else
    hold('counts_from_zero', built, phases, reduce(built), record_property)


@pytest.mark.parametrize('name', T.RANGE_CASES)
def test_dynamic_range(name, sub, record_property):
    """Forty decades upwards (every phase raises the block exponent and rescales the tile) and downwards, gradients below the exponent
    floor 2^-100, a batch of zeros between two live ones, signs that cancel."""
    built, phases = T.case_range(name, sub)
    got = reduce(built)
    hold(name, built, phases, got, record_property)
    if name == 'cancel':
        # one workgroup, one exponent, no rescale: round-to-nearest is odd and integer addition exact, so +g w and -g w cancel to the bit
        assert not got.any()


@pytest.mark.parametrize('name', sorted(T.BUDGET_CASES))
def test_overflow_budget(name, sub, record_property):
    """More near-maximal same-sign weight-1 records on one texel than the blind budget of 2047: 2136 still fit an int32 at that scale
    (the workgroup looks and goes on), 2600 cannot (it has to flush and clear) -- test_texbin_ref_host.py has the sums."""
    built, phases = T.case_budget(name, sub)
    got = reduce(built)
    hold(name, built, phases, got, record_property)
    n = T.BUDGET_CASES[name]
    assert abs(float(got.reshape(32, 32, 3)[5, 5, 0]) / (n * 1.9) - 1) < 1e-5          # (a wrapped tile would be off by its whole range)


@pytest.mark.parametrize('name', sorted(T.RESCALE_CASES))
def test_rescale_rounds_without_leaving_int32(name, sub, record_property):
    """A texel that holds more than 2^31 - 2^(sh-1) units when a batch raises the exponent by sh bits: the rounding of the rescale
    must not wrap (`q + half` did: -1 unit where 0.7 rounds to 1, -2 where 1.76 rounds to 2), and a raise of more than 31 bits must
    shift by all of them (0.0007 units round to 0, not to 1)."""
    built, phases = T.case_rescale(name, sub)
    got = reduce(built)
    a, b = got.reshape(32, 32, 3)[T.TEXEL_A], got.reshape(32, 32, 3)[T.TEXEL_B]
    print(f'texbin_reduce {name}: texel A = {a[0] * 2.0 ** 19:.4f} units of 2^-19, texel B = {b[0]}')
    hold(name, built, phases, got, record_property)
    assert (b == 1.0).all()


def test_nonfinite_gradients_poison_their_map_and_nothing_else(sub):
    """A NaN gradient, then a +inf gradient in one bin: the first float of that bin's map becomes NaN; every texel of the other bins
    (one workgroup each: order-free) keeps the bits of the run without the two records."""
    clean, dirty, bad = T.case_nonfinite(sub)
    want, got = reduce(clean), reduce(dirty)
    assert np.isfinite(want).all() and np.isnan(got[int(clean.maps.info[bad, 0])])
    other = np.ones((64, 64, 3), dtype=bool)
    ty, tx = int(clean.maps.info[bad, 3]) >> 16, int(clean.maps.info[bad, 3]) & 0xffff
    other[ty * 32:ty * 32 + 32, tx * 32:tx * 32 + 32] = False
    other = other.reshape(-1)
    other[int(clean.maps.info[bad, 0])] = False
    assert other.sum() == 3 * 3 * 32 * 32 - 1
    assert np.array_equal(got[other].view(np.int32), want[other].view(np.int32))
