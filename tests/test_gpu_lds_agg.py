"""LdsAgg (csrc/dbw_common.h: the LDS hash table in front of the texel-gradient atomics -- TexAgg with 256 slots, HardTexAgg with 64)
on caller-supplied keys, through tests/device_checks.hip: dbwt_lds_agg.  Whatever the key pattern -- more keys than slots (some updates
must take the global-atomic fall-through after 8 probes), exactly as many, one key per wave on either side of the wave-sum switch,
inactive lanes with arbitrary keys -- the per-key sums of the ACTIVE triples must come out: EQUAL for integer-valued floats, within
(W + 2) * 2^-24 * sum |v| of the float64 scatter for random fp32 values, W = the workgroups that touch the key (one flush each)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import device_checks                                            # noqa: E402

ROUNDS = 8
PER_WG = ROUNDS * 256


def patterns(log2, seed):
    """-> keys, active (n,) int32 for six workgroups, n_keys"""
    ns = 1 << log2
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(PER_WG)
    many = 3 * ns + 5                                           # (more distinct keys than slots, spread over the hash)
    wg = []
    # 0: more distinct keys in one workgroup than the table has slots
    wg.append(((i * 7) % many, torch.ones(PER_WG, dtype=torch.int64)))
    # 1: exactly NSLOT keys, key 0 among them
    wg.append((i % ns, torch.ones(PER_WG, dtype=torch.int64)))
    # 2: waves of one key -- 64, 8 and 7 active lanes (the wave sum takes over at 8) --, a wave of two keys, key 0 on a whole wave
    k = torch.randint(0, 24, (PER_WG,), generator=g)
    a = (torch.rand(PER_WG, generator=g) < 0.7).long()
    lane = i % 64
    for w, (key, n_on) in enumerate([(0, 64), (5, 8), (5, 7), (9, 64), (11, 8), (11, 7), (many - 1, 64), (3, 1)]):
        sel = slice(w * 64, w * 64 + 64)
        k[sel] = key
        on = torch.zeros(64, dtype=torch.int64)
        on[torch.randperm(64, generator=g)[:n_on]] = 1
        a[sel] = on
    k[8 * 64:9 * 64] = torch.where(lane[:64] < 32, 4, 6)        # two keys, every lane active
    a[8 * 64:9 * 64] = 1
    k[9 * 64:10 * 64] = torch.where(lane[:64] % 2 == 0, 4, 6)   # two keys interleaved
    a[9 * 64:10 * 64] = 1
    k[10 * 64:11 * 64] = (lane[:64] // 4) % 3                   # aligned runs of four equal keys: the lane merge has something to do
    a[10 * 64:11 * 64] = 1
    wg.append((k, a))
    # 3: inactive lanes carry arbitrary keys -- negative, far outside the output -- and must contribute nothing
    k = torch.randint(0, 24, (PER_WG,), generator=g)
    a = (torch.rand(PER_WG, generator=g) < 0.5).long()
    junk = torch.tensor([-1, -1000, 2**31 - 1, -2**31, 123456789, 7, 0])[torch.randint(0, 7, (PER_WG,), generator=g)]
    k = torch.where(a == 1, k, junk)
    k[:64], a[:64] = 7, 0                                       # a wave with nobody active
    k[64:128] = torch.where(lane[:64] < 9, 2, -5)               # 9 active lanes of one key, the rest inactive with another
    a[64:128] = (lane[:64] < 9).long()
    wg.append((k, a))
    # 4, 5: the keys of 2 and 3 again -- several workgroups flush the same key
    for _ in range(2):
        wg.append((torch.randint(0, 24, (PER_WG,), generator=g), (torch.rand(PER_WG, generator=g) < 0.8).long()))
    keys = torch.cat([w[0] for w in wg]).to(torch.int32)
    active = torch.cat([w[1] for w in wg]).to(torch.int32)
    return keys, active, many


def scatter64(keys, active, values, n_keys):
    on = active != 0
    idx = keys[on].long()
    ref = torch.zeros(n_keys, 3, dtype=torch.float64).index_add_(0, idx, values[on].double())
    mag = torch.zeros(n_keys, 3, dtype=torch.float64).index_add_(0, idx, values[on].double().abs())
    return ref, mag


@pytest.mark.parametrize('op', device_checks.LDS_AGG_OPS)
@pytest.mark.parametrize('log2', [6, 8])
def test_per_key_sums_are_exact_on_integer_values(log2, op):
    keys, active, n_keys = patterns(log2, log2)
    ns = 1 << log2
    first = keys[:PER_WG][active[:PER_WG] != 0]
    assert first.unique().numel() > ns                          # pigeonhole: some update of workgroup 0 finds no slot and goes to memory
    assert keys[PER_WG:2 * PER_WG].unique().numel() == ns and int(keys[PER_WG]) == 0
    g = torch.Generator().manual_seed(100 + log2)
    values = torch.randint(-8, 9, (keys.numel(), 3), generator=g).float()
    values[torch.rand(keys.numel(), generator=g) < 0.1] = 0.0                         # zero values (the table skips them)
    values[2 * PER_WG + 3 * 64:2 * PER_WG + 4 * 64, 1] = 0.0                          # ... and a whole wave-summed channel of them
    ref, _ = scatter64(keys, active, values, n_keys)
    assert float(ref.abs().max()) < 2**24 and bool((ref != 0).any(1).sum() > ns)
    out = device_checks.lds_agg(keys, active, values, n_keys, log2, op, ROUNDS)
    assert torch.equal(out.double(), ref)


@pytest.mark.parametrize('op', device_checks.LDS_AGG_OPS)
@pytest.mark.parametrize('log2', [6, 8])
def test_per_key_sums_of_fp32_values_against_the_float64_scatter(log2, op, record_property):
    keys, active, n_keys = patterns(log2, 50 + log2)
    g = torch.Generator().manual_seed(200 + log2)
    values = torch.randn(keys.numel(), 3, generator=g) * torch.exp(torch.randn(keys.numel(), 1, generator=g))
    ref, mag = scatter64(keys, active, values, n_keys)
    on = active != 0
    wg = torch.arange(keys.numel()) // PER_WG
    touched = torch.zeros(n_keys, 6).index_put_((keys[on].long(), wg[on]), torch.ones(int(on.sum())))
    W = touched.sum(1, keepdim=True).double()                   # workgroups that touch the key
    assert int(W.max()) >= 4
    out = device_checks.lds_agg(keys, active, values, n_keys, log2, op, ROUNDS)
    bound = (W + 2) * 2.0 ** -24 * mag
    err = (out.double() - ref).abs()
    live = mag > 0
    ratio = float((err[live] / bound[live]).max())
    print(f'LdsAgg<3, {log2}>::{op}: {int(live.sum())} key-channels, max err / bound = {ratio:.4f}')
    record_property('err_over_bound', ratio)
    assert bool((out[~live] == 0).all()) and ratio <= 1.0
