"""CPU checks of tests/texbin_ref.py: the record builder and the float64 scatter against an independent brute-force scatter that
decodes the packed buffer word by word, and the conditions without which the GPU cases of tests/test_gpu_texbin_reduce.py would be
vacuous -- the budget cases reach the sums they claim, the rescale samples sit in the window where an int32 rounding add wraps, the
phases of a phase case never share a staged batch, and the sentinel would be seen if a record outside a sub-range's capacity were read."""
import struct

import numpy as np
import pytest

import texbin_ref as T

SUB = 16            # (DBW_BIN_SUBCURSORS of the shipped build; the builder takes whatever the library says on the GPU side)


def brute_force(built, ignore_capacity=False):
    """Walk the packed buffer the way a reader of the documented layout would: per (bin, sub-range) `min(cursor, capacity)` records from
    `first`, each decoded with struct from its 24 bytes, each scattered bilinearly in Python floats (= float64)."""
    maps = built.maps
    out = [0.0] * maps.total
    raw = built.buffer.tobytes()
    for i in range(maps.nbins * built.sub):
        b = i // built.sub
        off, ws, hs, tile = (int(x) for x in maps.info[b])
        ty, tx = tile >> 16, tile & 0xffff
        first, cap = int(built.layout[i, 0]), int(built.layout[i, 1])
        n = int(built.cursor[i]) if ignore_capacity else min(int(built.cursor[i]), cap)
        for k in range(first, first + n):
            packed, wx1, wy1, g0, g1, g2 = struct.unpack_from('<Ifffff', raw, k * 24)
            r0, c0, dr, dc = ty * 32 + (packed & 31), tx * 32 + ((packed >> 5) & 31), (packed >> 10) & 1, (packed >> 11) & 1
            for r, c, w in ((r0, c0, (1 - wx1) * (1 - wy1)), (r0, c0 + dc, wx1 * (1 - wy1)), (r0 - dr, c0, (1 - wx1) * wy1), (r0 - dr, c0 + dc, wx1 * wy1)):
                assert 0 <= r < hs and 0 <= c < ws
                for ch, g in enumerate((g0, g1, g2)):
                    out[off + (r * ws + c) * 3 + ch] += g * w
    return np.array(out)


@pytest.mark.parametrize('name', sorted(T.GEOMETRY_SHAPES))
def test_builder_and_scatter_equal_a_brute_force_decode(name):
    built, _ = T.case_geometry(name, SUB)
    ref, count = T.reference(built)
    bf = brute_force(built)
    _, abs_sum = T.scatter64(built.maps, T.Records.cat(list(built.counted.values())))
    assert (np.abs(ref - bf) <= 1e-13 * abs_sum).all() and np.abs(ref).max() > 1
    assert ((count > 0) == (abs_sum > 0)).mean() > 0.9
    # the geometry the case is about is in it
    rec = T.Records.cat(list(built.counted.values()))
    h = max(h for h, _ in built.maps.shapes)
    w = max(w for _, w in built.maps.shapes)
    assert ((rec.dr == 0) & (rec.dc == 0) & (rec.wx1 > 0) & (rec.wx1 < 1) & (rec.wy1 > 0) & (rec.wy1 < 1)).any()
    for wgt in (rec.wx1, rec.wy1):
        assert (wgt == 0).any() and (wgt == 1).any()
    if h > 32:
        assert ((rec.R0 % 32 == 0) & (rec.R0 >= 32) & (rec.dr == 1)).sum() >= 30           # halo row: the tile above
    if w > 32:
        assert ((rec.C0 % 32 == 31) & (rec.dc == 1)).sum() >= 30                           # halo column: the tile to the right
    if h > 32 and w > 32:
        assert ((rec.R0 % 32 == 0) & (rec.R0 >= 32) & (rec.dr == 1) & (rec.C0 % 32 == 31) & (rec.dc == 1)).any()   # the halo's corner
    if len(built.maps.shapes) > 1:
        assert built.maps.info[-1, 0] > 0 and (rec.m == 1).any()                           # a non-zero `off`


def test_counts_case_layout_and_sentinel():
    built, _ = T.case_counts(SUB)
    ref, count = T.reference(built)
    bf = brute_force(built)
    assert np.abs(ref - bf).max() <= 1e-12
    lay, cur = built.layout.astype(np.int64), built.cursor.astype(np.int64)
    assert sorted(set(lay[:SUB, 1].tolist())) == sorted(set(T.COUNTS))                     # 0, 1, 511, 512, 513, 1025, ... in bin 0
    assert (cur[SUB:2 * SUB] == 0).all()                                                   # bin 1 is empty
    over = cur > lay[:, 1]
    assert over.sum() == 3 and (cur - lay[:, 1]).max() >= 512                              # cursors beyond the capacity, one by more than a batch
    occupied = lay[lay[:, 1] > 0]
    assert (np.diff(occupied[:, 0]) >= occupied[:-1, 1]).all()                             # sub-ranges do not overlap
    assert len(set((occupied[:, 0] % 8).tolist())) > 4                                     # `first` is a multiple of nothing
    # every slot outside the counted records is the sentinel, and reading one would show
    counted = np.zeros(len(built.buffer), dtype=bool)
    for f, c in lay:
        counted[f:f + c] = True
    assert (built.buffer[~counted] == T.SENTINEL).all() and (~counted).sum() > 700
    assert not (built.buffer[counted][:, 3:6].view(np.float32) == np.float32(T.SENTINEL_G)).any()
    leak = brute_force(built, ignore_capacity=True)
    assert np.abs(leak - ref).max() > 1e29 > 1e6 * np.abs(ref).max()
    # the empty bin keeps texels nobody adds to
    untouched = (count.reshape(64, 64, 3)[:32, 32:] == 0)
    assert untouched.sum() > 100


def ideal_fixed_point(built):
    """What the contract describes, at its loosest: every addend (the fp32 product g * w) rounded to the unit of the bin's largest
    gradient, summed exactly."""
    maps = built.maps
    out = np.zeros(maps.total)
    by_bin = {}
    for (b, s), rec in built.counted.items():
        by_bin.setdefault(b, []).append(rec)
    for b, recs in by_bin.items():
        rec = T.Records.cat(recs)
        e = T.record_exponents(rec).max()
        _, w = T.corners(maps, rec)
        w32 = np.stack([(1 - rec.wx1) * (1 - rec.wy1), rec.wx1 * (1 - rec.wy1), (1 - rec.wx1) * rec.wy1, rec.wx1 * rec.wy1], 1).astype(np.float32)
        prod = (rec.g[:, None, :] * w32[:, :, None]).astype(np.float32).astype(np.float64)
        out += T._scatter(maps, rec, np.rint(prod * np.ldexp(1.0, T.BIN_FIX_SH - int(e))) * float(T.unit(e)))
    return out


@pytest.mark.parametrize('case', ['geometry', 'counts', 'floor', 'cancel'])
def test_the_bar_admits_the_contract_and_nothing_much_larger(case):
    built, phases = {'geometry': lambda: T.case_geometry('two_maps', SUB), 'counts': lambda: T.case_counts(SUB),
                     'floor': lambda: T.case_range('floor', SUB), 'cancel': lambda: T.case_range('cancel', SUB)}[case]()
    ref, count = T.reference(built)
    bound = T.bar(built, phases)
    err = np.abs(ideal_fixed_point(built) - ref)
    assert (err <= bound).all() and (bound[count > 0] > 0).all() and (bound[count == 0] == 0).all()
    # the bar is a rounding bar: 2^-20 of the bin's largest gradient per addend, not a tolerance on the sum
    e = max(T.record_exponents(r).max() for r in built.counted.values())
    assert bound.max() <= (count.max() + 2 * SUB) * float(T.unit(e))
    if case == 'cancel':
        rec = built.counted[(0, 0)]
        n = len(rec) // 2                                   # (every record has its negative: 0 but for the float64 sum's own rounding)
        assert np.array_equal(T.pack(rec[np.arange(n)])[:, :3], T.pack(rec[np.arange(n, 2 * n)])[:, :3]) and np.array_equal(rec.g[:n], -rec.g[n:])
        assert np.abs(ref).max() < 1e-12 and len(built.counted) == 1 and len(np.unique(T.record_exponents(rec))) == 1
    if case == 'floor':
        g = np.abs(T.Records.cat(list(built.counted.values())).g)
        assert g.max() < 2.0 ** -100 and g.min() > 2.0 ** -126 and (g < 2.0 ** -121).any()


@pytest.mark.parametrize('name', ['ascending', 'descending', 'zero_batch'] + sorted(k for k, v in T.RESCALE_CASES.items() if v[2] == 1))
def test_phases_never_share_a_staged_batch(name):
    built, phases = T.case_rescale(name, SUB) if name in T.RESCALE_CASES else T.case_range(name, SUB)
    assert list(built.counted) == [(0, 0)]                                                 # ONE sub-range of the bin
    rec, ph = built.counted[(0, 0)], phases[(0, 0)]
    live = np.flatnonzero(np.abs(rec.g).max(1) > 0)
    assert (T.record_exponents(rec)[live] <= ph[live]).all()
    step = ph[live][1:] != ph[live][:-1]
    change, prev = live[1:][step], live[:-1][step]
    if name in ('ascending', 'descending'):
        assert len(change) == 10 and ph[live].max() - ph[live].min() > 130                 # 40 decades = 133 bits, every phase another exponent
        assert ((ph[change] > ph[prev]) == (name == 'ascending')).all()
    assert (change - prev > 1024).all()                                                    # >= 1024 zero records between two magnitudes
    if name == 'zero_batch':
        gaps = np.diff(live)
        assert gaps.max() == 1025 and len(live) == 1200


@pytest.mark.parametrize('name', sorted(T.BUDGET_CASES))
def test_budget_cases_reach_their_branch(name):
    built, _ = T.case_budget(name, SUB)
    rec = built.counted[(0, 0)]
    n = len(rec)
    e = int(T.record_exponents(rec).max())
    total = T.fixed_point_sum(rec.g[:, 0], e)
    per = T.fixed_point_sum(rec.g[:1, 0], e)
    assert e == 1 and per == 996147 and (rec.wx1 == 0).all() and (rec.wy1 == 0).all() and n > 2047
    for stage in (128, 256, 512, 1024):
        looks, flushes, peak = T.budget_walk(np.full(n, per), stage)
        assert peak <= 2**31 - 1                                                           # what the budget is for
        if name == 'look_and_go_on':
            assert total <= 2**31 - 1 and looks >= 1 and flushes == 0                      # fits: every look finds room for the next batch
        else:
            assert total > 2**31 and looks >= 2 and flushes >= 1                           # cannot fit: some look must flush and clear


def wrapping_rescale(q, sh):
    """the rounding add as int32 arithmetic performs it"""
    s = (q + (1 << (sh - 1))) & 0xffffffff
    s = s - (1 << 32) if s >= (1 << 31) else s
    return s >> sh


@pytest.mark.parametrize('name', sorted(T.RESCALE_CASES))
def test_rescale_samples_sit_where_a_rounding_add_wraps(name):
    n, g, nsub = T.RESCALE_CASES[name]
    built, phases = T.case_rescale(name, SUB)
    a = built.counted[(0, 0)]
    a = a[np.arange(n)]
    e_a, e_b = int(T.record_exponents(a).max()), 1
    d = e_b - e_a
    assert d == int(name[1:3])
    q = T.fixed_point_sum(a.g[:, 0], e_a)
    sh = min(d, 31)
    assert 2**31 - (1 << (sh - 1)) < q <= 2**31 - 1                                        # inside the budget, and the rounding add leaves int32
    true_units = q / 2.0 ** d
    wrapped = wrapping_rescale(q, sh)
    assert wrapped < 0 and abs(wrapped - true_units) > 1                                   # the wrong sign, more than a unit away
    # ... which the bar does not allow at texel A, while the correct rounding passes it
    bound = T.bar(built, phases).reshape(32, 32, 3)[T.TEXEL_A]
    u_after = float(T.unit(e_b))
    assert (abs(wrapped - true_units) * u_after > 1.9 * bound).all()
    assert (bound < 0.51 * u_after + n * 0.5 * float(T.unit(e_a)) + 2.0 ** -21 * q * float(T.unit(e_a)) * 1.01).all()
    assert (bound < 1.5 * u_after).all() and (abs(np.rint(true_units) - true_units) * u_after < bound).all()
    # does the tile still hold q when the exponent is raised?  One sub-range: the zero records between the phases are batches too, and a
    # batch larger than the budget makes the workgroup look -- and flush and clear when less than a batch's worth of room is left.
    if nsub == 1:
        per = T.fixed_point_sum(a.g[:1, 0], e_a)
        seq = np.r_[np.full(n, per), np.zeros(1024, dtype=np.int64), [0]]
        looks, flushes, _ = T.budget_walk(seq, 512)
        assert flushes == (1 if name == 'd30' else 0)     # d30: q > 1.75 * 2^30 leaves room for < 256 records, a 512-record batch flushes first
    else:
        assert n + 1 <= 2047 and sorted(built.counted) == [(0, 0), (0, 1)]                 # inside the blind budget: nobody looks


def test_nonfinite_case():
    clean, dirty, bad_bin = T.case_nonfinite(SUB)
    assert sorted(clean.counted) == [(b, 0) for b in range(4)] == sorted(dirty.counted)    # one occupied sub-range per bin: one workgroup, order-free
    g = dirty.counted[(bad_bin, 0)].g
    assert np.isnan(g).sum() == 1 and np.isinf(g).sum() == 1 and np.flatnonzero(np.isnan(g).any(1))[0] < np.flatnonzero(np.isinf(g).any(1))[0]
    for b in range(4):
        if b != bad_bin:
            assert np.isfinite(dirty.counted[(b, 0)].g).all() and (pack_eq(clean.counted[(b, 0)], dirty.counted[(b, 0)]))
    # no footprint leaves its tile: texels outside bin 2's tile hear nothing from bin 2
    _, count = T.reference(T.build(clean.maps, SUB, {(bad_bin, 0): clean.counted[(bad_bin, 0)]}))
    c = count.reshape(64, 64, 3)
    assert c[32:, :32].sum() == c.sum() and c[32:, :32].min() >= 0


def pack_eq(a, b):
    return np.array_equal(T.pack(a), T.pack(b))
