"""Host side of the texture-bin reduction tests (numpy only, importable without a GPU): hand-built records in the 24-byte layout
that dbw_texbin_reduce reads, the sub-range table that goes with them, the float64 scatter they stand for, and the error bar the
kernel's documented contract allows ("Texel-gradient accumulators against a float64 scatter").

A record = three 8-byte words {packed, wx1} {wy1, g0} {g1, g2} (csrc/shade_blend.hip: st_record), packed = (r0 & 31) | (c0 & 31) << 5 |
dr << 10 | dc << 11 with (r0, c0) the footprint's first texel in the map.  The record lives in the bin of the 32x32 tile that holds
(r0, c0) and adds g * w to four texels: (r0, c0) w = (1-wx1)(1-wy1), (r0, c0+dc) w = wx1 (1-wy1), (r0-dr, c0) w = (1-wx1) wy1,
(r0-dr, c0+dc) w = wx1 wy1.  With dr = 0 or dc = 0 two or all four of these ADDENDS land on one texel."""
import numpy as np

# csrc/shade_blend.hip, in front of texbin_reduce_kernel: `constexpr int BIN_FIX_SH = 20, BIN_FIX_EMIN = -100;` -- the tile holds
# value * 2^(SH - e) with e the block exponent (|g| < 2^e for every gradient seen so far, never below EMIN)
BIN_FIX_SH = 20
BIN_FIX_EMIN = -100
TILE = 32


class Records:
    """n records in map coordinates: map index m, first texel (R0, C0), steps dr / dc (0 | 1), weights wx1 / wy1 (fp32), g (n, 3) fp32."""
    FIELDS = ('m', 'R0', 'C0', 'dr', 'dc', 'wx1', 'wy1', 'g')

    def __init__(self, m, R0, C0, dr, dc, wx1, wy1, g):
        n = max(len(np.atleast_1d(x)) for x in (m, R0, C0, dr, dc, wx1, wy1)) if np.ndim(g) < 2 else len(g)
        as_i = lambda x: np.broadcast_to(np.asarray(x, dtype=np.int64), (n,)).copy()
        as_f = lambda x: np.broadcast_to(np.asarray(x, dtype=np.float32), (n,)).copy()
        self.m, self.R0, self.C0, self.dr, self.dc = as_i(m), as_i(R0), as_i(C0), as_i(dr), as_i(dc)
        self.wx1, self.wy1 = as_f(wx1), as_f(wy1)
        self.g = np.broadcast_to(np.asarray(g, dtype=np.float32), (n, 3)).copy()

    def __len__(self):
        return len(self.R0)

    def __getitem__(self, sel):
        return Records(*[getattr(self, f)[sel] for f in self.FIELDS])

    @staticmethod
    def cat(parts):
        parts = [p for p in parts if len(p)]
        if not parts:
            return Records.empty()
        return Records(*[np.concatenate([getattr(p, f) for p in parts]) for f in Records.FIELDS])

    @staticmethod
    def empty():
        return Records(np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((0, 3)))


def zero_records(n, m=0, R0=3, C0=3):
    """n records of zero gradient (a batch of them adds nothing and leaves the block exponent alone)."""
    return Records(np.full(n, m), np.full(n, R0), np.full(n, C0), np.ones(n), np.ones(n), np.full(n, 0.25), np.full(n, 0.75), np.zeros((n, 3)))


class Maps:
    """The maps of a case: shapes [(h, w)] and what PackedScene.describe_bins says about them (bin_base (M,), bin_info (nbins, 4) as
    numpy int32: {offset of the map in floats, ws, hs, tile_y << 16 | tile_x})."""

    def __init__(self, shapes, bin_base, bin_info):
        self.shapes = [tuple(s) for s in shapes]
        self.base = np.asarray(bin_base, dtype=np.int64).reshape(-1)
        self.info = np.asarray(bin_info, dtype=np.int32).reshape(-1, 4)
        self.nbins = self.info.shape[0]
        self.off = np.array([self.info[b, 0] for b in self.base], dtype=np.int64)
        self.total = int(sum(h * w * 3 for h, w in self.shapes))

    def bin_of(self, rec):
        ws = np.array([w for _, w in self.shapes], dtype=np.int64)[rec.m]
        return self.base[rec.m] + (rec.R0 // TILE) * ((ws + TILE - 1) // TILE) + rec.C0 // TILE

    def check_writable(self, rec):
        """Only what the backward's writer can produce: the footprint inside the map (row r0 - dr >= 0, column c0 + dc < ws)."""
        hs = np.array([h for h, _ in self.shapes], dtype=np.int64)[rec.m]
        ws = np.array([w for _, w in self.shapes], dtype=np.int64)[rec.m]
        assert ((rec.dr | rec.dc) & ~1 == 0).all()
        assert (rec.R0 - rec.dr >= 0).all() and (rec.R0 < hs).all() and (rec.C0 >= 0).all() and (rec.C0 + rec.dc < ws).all()
        assert ((rec.wx1 >= 0) & (rec.wx1 <= 1) & (rec.wy1 >= 0) & (rec.wy1 <= 1)).all()


def pack(rec):
    """-> (n, 6) int32: the records as the kernel reads them."""
    out = np.zeros((len(rec), 6), dtype=np.int32)
    out[:, 0] = ((rec.R0 & 31) | ((rec.C0 & 31) << 5) | (rec.dr << 10) | (rec.dc << 11)).astype(np.int32)
    out[:, 1] = rec.wx1.view(np.int32)
    out[:, 2] = rec.wy1.view(np.int32)
    out[:, 3:6] = rec.g.view(np.int32)
    return out


# what fills every record slot that must not be read: were it added, its texel would stand out by thirty orders of magnitude
SENTINEL_G = 3.0e30
SENTINEL = pack(Records(0, 7, 9, 1, 1, 0.5, 0.5, [[SENTINEL_G, -SENTINEL_G, SENTINEL_G]]))[0]


class Built:
    """layout (nbins * sub, 2) uint32 {first, capacity}, cursor (nbins * sub,) int32, buffer (N, 6) int32, counted {(bin, s): Records}."""


def build(maps, sub, placed, gaps=None, cursor_extra=None, head=0):
    """placed {(bin, s): Records}: the records of sub-range s of a bin, in order.  Sub-ranges lie back to back in (bin, s) order behind
    `head` unused records, sub-range i follows gaps[i % len(gaps)] unused records (a layout whose `first` is no multiple of anything);
    capacity = the number of records placed.  cursor_extra {(bin, s): k}: that cursor reads k more than the capacity, as after a launch
    whose demand did not fit -- only `capacity` records count.  Every slot outside the counted records holds SENTINEL."""
    gaps = list(gaps) if gaps else [0]
    cursor_extra = cursor_extra or {}
    n = maps.nbins * sub
    layout = np.zeros((n, 2), dtype=np.uint32)
    cursor = np.zeros(n, dtype=np.int32)
    chunks, at = [np.tile(SENTINEL, (head, 1))], head
    for i in range(n):
        key = (i // sub, i % sub)
        rec = placed.get(key)
        k = 0 if rec is None else len(rec)
        gap = gaps[i % len(gaps)]
        chunks.append(np.tile(SENTINEL, (gap, 1)))
        at += gap
        layout[i] = (at, k)
        cursor[i] = k + cursor_extra.get(key, 0)
        if k:
            maps.check_writable(rec)
            assert (maps.bin_of(rec) == key[0]).all(), 'a record belongs to the bin of the tile that holds (r0, c0)'
            chunks.append(pack(rec))
            at += k
    extra = max(cursor_extra.values(), default=0)
    chunks.append(np.tile(SENTINEL, (extra + 8, 1)))          # (what an over-full cursor would reach if the capacity were ignored)
    b = Built()
    b.layout, b.cursor, b.buffer = layout, cursor, np.concatenate(chunks).astype(np.int32)
    b.counted = {k: v for k, v in placed.items() if len(v)}
    b.maps, b.sub = maps, sub
    return b


def corners(maps, rec):
    """-> idx (n, 4) int64: float index of channel 0 of the four footprint texels in the flat gradient buffer; w (n, 4) float64: their
    bilinear weights formed in float64 from the fp32 wx1, wy1."""
    ws = np.array([w for _, w in maps.shapes], dtype=np.int64)[rec.m]
    wx1, wy1 = rec.wx1.astype(np.float64), rec.wy1.astype(np.float64)
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    w = np.stack([wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1], 1)
    rr = np.stack([rec.R0, rec.R0, rec.R0 - rec.dr, rec.R0 - rec.dr], 1)
    cc = np.stack([rec.C0, rec.C0 + rec.dc, rec.C0, rec.C0 + rec.dc], 1)
    idx = maps.off[rec.m][:, None] + (rr * ws[:, None] + cc) * 3
    return idx, w


def _scatter(maps, rec, per_corner):
    """sum into a flat float64 buffer of per_corner (n, 4, 3) at the footprint texels"""
    out = np.zeros(maps.total, dtype=np.float64)
    if len(rec):
        idx, _ = corners(maps, rec)
        np.add.at(out, (idx[:, :, None] + np.arange(3)[None, None, :]).reshape(-1), per_corner.reshape(-1))
    return out


def scatter64(maps, rec):
    """The float64 scatter of g * w -> (sum, sum of |g * w|), flat like grad_maps."""
    if not len(rec):
        return np.zeros(maps.total), np.zeros(maps.total)
    _, w = corners(maps, rec)
    gw = rec.g.astype(np.float64)[:, None, :] * w[:, :, None]
    return _scatter(maps, rec, gw), _scatter(maps, rec, np.abs(gw))


def exponent_bound(x):
    """e with |x| < 2^e as the kernel takes it from the biased exponent of the largest |g| (E - 126), never below BIN_FIX_EMIN."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    e = np.frexp(x)[1].astype(np.int64)            # x = m * 2^e, 0.5 <= m < 1
    return np.where(x > 0, np.maximum(e, BIN_FIX_EMIN), BIN_FIX_EMIN)


def record_exponents(rec):
    return exponent_bound(np.abs(rec.g).max(1)) if len(rec) else np.zeros(0, dtype=np.int64)


def unit(e):
    return np.ldexp(1.0, np.asarray(e, dtype=np.int64) - BIN_FIX_SH)


def bar(built, phases=None, prior=None):
    """Per texel-channel t of the flat gradient buffer:

        1/2 * sum_addends u_i  +  1/2 * sum_raises u_after  +  2^-21 * (sum |g_i w_i| + |prior|)

    u_i = 2^(E_i - SH), E_i >= the block exponent of the reducing workgroup when record i was added.  Every addend is rounded once:
    a record counts once per footprint corner that lands on t (twice or four times when dr or dc is 0).
    Unordered cases (phases None): E_i = the exponent of the bin's largest gradient; a workgroup raises its exponent at most once to
    every exponent some record of the bin has, except the smallest, and a bin has at most as many workgroups as occupied sub-ranges.
    Phase cases: phases {(bin, s): [exponent of record i's phase]} for bins with ONE occupied sub-range, whose phases of different
    magnitude are kept out of each other's staged batch by >= 1024 zero records (or with one phase per sub-range: a staged batch
    never spans two sub-ranges): E_i = the running maximum, one raise per increase.
    The last term: three fp32 roundings of g * w, the int -> float conversion, the fp32 adds into grad_maps (also of what was there)."""
    maps = built.maps
    out = np.zeros(maps.total, dtype=np.float64)
    by_bin = {}
    for (b, s), rec in built.counted.items():
        by_bin.setdefault(b, []).append((s, rec))
    all_rec = []
    for b, subs in by_bin.items():
        touched = np.zeros(maps.total, dtype=bool)
        exps = np.concatenate([record_exponents(rec)[np.abs(rec.g).max(1) > 0] for _, rec in subs])
        if phases is not None and (b, subs[0][0]) in phases:
            # (sub-ranges in ascending order, as a workgroup that holds several walks them; should they belong to different
            # workgroups the running maximum is still an upper bound of each one's exponent, and the raise is counted for nothing)
            subs.sort(key=lambda x: x[0])
            ph = np.concatenate([np.asarray(phases[(b, s)], dtype=np.int64) for s, _ in subs])
            rec = Records.cat([r for _, r in subs])
            assert len(ph) == len(rec) and (ph >= record_exponents(rec)).all()
            run_all = np.maximum.accumulate(ph)
            E, at = [], 0
            for _, r in subs:
                E.append(run_all[at:at + len(r)])
                at += len(r)
            live = ph[np.abs(rec.g).max(1) > 0]
            run = np.maximum.accumulate(live) if len(live) else live
            raises = run[1:][run[1:] > run[:-1]]
        else:
            e_bin = exps.max() if len(exps) else BIN_FIX_EMIN
            E = [np.full(len(rec), e_bin) for _, rec in subs]
            distinct = np.unique(exps)
            raises = np.repeat(distinct[1:], len(subs))
        for (s, rec), e in zip(subs, E):
            half_u = 0.5 * unit(e)
            out += _scatter(maps, rec, np.broadcast_to(half_u[:, None, None], (len(rec), 4, 3)))
            touched |= _scatter(maps, rec, np.ones((len(rec), 4, 3))) > 0
            all_rec.append(rec)
        out[touched] += 0.5 * float(unit(raises).sum()) if len(raises) else 0.0
    _, abs_sum = scatter64(maps, Records.cat(all_rec))
    out += np.ldexp(1.0, -21) * (abs_sum + (0.0 if prior is None else np.abs(np.asarray(prior, dtype=np.float64))))
    return out


def reference(built):
    """-> (float64 scatter of every counted record, addends per texel-channel)."""
    rec = Records.cat(list(built.counted.values()))
    ref, _ = scatter64(built.maps, rec)
    return ref, _scatter(built.maps, rec, np.ones((len(rec), 4, 3)))


def fixed_point_sum(g, e):
    """sum round(g * 2^(SH - e)) over weight-1 records, as Python ints: what an int32 tile would have to hold."""
    q = np.rint(np.asarray(g, dtype=np.float64) * np.ldexp(1.0, BIN_FIX_SH - e))
    return int(q.astype(np.int64).sum())


def budget_walk(q_per_record, stage):
    """The budget rule the kernel documents (2047 blind records for an empty tile; then look: (2^31 - 1 - B) >> SH more, or flush and
    clear), walked over ONE texel that receives q_per_record[i] >= 0 units from record i of one sub-range.  -> (looks, flushes, the
    largest tile entry seen)."""
    q = np.asarray(q_per_record, dtype=np.int64)
    full = (2**31 - 1) >> BIN_FIX_SH
    budget, tile, looks, flushes, peak = full, 0, 0, 0, 0
    for sb in range(0, len(q), stage):
        batch = q[sb:sb + stage]
        m = len(batch)
        if m > budget:
            looks += 1
            budget = (2**31 - 1 - tile) >> BIN_FIX_SH
            if m > budget:
                flushes += 1
                tile, budget = 0, full
        if batch.any():
            tile += int(batch.sum())
            budget -= m
        peak = max(peak, tile)
    return looks, flushes, peak


# ---- the cases of tests/test_gpu_texbin_reduce.py (built on the host; tests/test_texbin_ref_host.py checks that they are what they claim) ----

def maps_of(shapes):
    from dbw_amd.structures import PackedScene
    base, info, _ = PackedScene.describe_bins(shapes, 'cpu')
    return Maps(shapes, base.numpy(), info.numpy())


def _weights(rng, n):
    """bilinear weights with exact zeros and ones among them"""
    w = rng.random(n).astype(np.float32)
    pick = rng.integers(0, 8, n)
    return np.where(pick == 0, np.float32(0), np.where(pick == 1, np.float32(1), w)).astype(np.float32)


def random_records(maps, n, rng, scale=1.0, m=None, rows=None, cols=None, halo=True):
    """n writable records: anywhere in the maps, or in rows / cols [lo, hi) of map m; halo False: no footprint leaves its 32x32 tile."""
    mm = rng.integers(0, len(maps.shapes), n) if m is None else np.full(n, m)
    hs = np.array([h for h, _ in maps.shapes])[mm]
    ws = np.array([w for _, w in maps.shapes])[mm]
    r_lo, r_hi = (np.zeros(n, dtype=np.int64), hs) if rows is None else (np.full(n, rows[0]), np.minimum(rows[1], hs))
    c_lo, c_hi = (np.zeros(n, dtype=np.int64), ws) if cols is None else (np.full(n, cols[0]), np.minimum(cols[1], ws))
    R0, C0 = rng.integers(r_lo, r_hi), rng.integers(c_lo, c_hi)
    dr = rng.integers(0, 2, n) * (R0 > 0)
    dc = rng.integers(0, 2, n) * (C0 < ws - 1)
    if not halo:
        dr, dc = dr * (R0 % TILE > 0), dc * (C0 % TILE < TILE - 1)
    g = (rng.standard_normal((n, 3)) * scale).astype(np.float32)
    return Records(mm, R0, C0, dr, dc, _weights(rng, n), _weights(rng, n), g)


def place(maps, rec, sub, rng=None, only_sub=None):
    """records -> {(bin, s): Records}: every record into a random sub-range of its bin (or into only_sub), order kept"""
    b = maps.bin_of(rec)
    s = np.full(len(rec), only_sub) if only_sub is not None else rng.integers(0, sub, len(rec))
    return {(int(bb), int(ss)): rec[(b == bb) & (s == ss)] for bb, ss in sorted(set(zip(b.tolist(), s.tolist())))}


GEOMETRY_SHAPES = {'32x32': [(32, 32)], '33x40': [(33, 40)], '64x64': [(64, 64)], 'two_maps': [(33, 40), (64, 64)]}


def case_geometry(name, sub):
    maps = maps_of(GEOMETRY_SHAPES[name])
    rng = np.random.default_rng(sorted(GEOMETRY_SHAPES).index(name) + 1)
    parts = [random_records(maps, 1500, rng)]
    for m, (h, w) in enumerate(maps.shapes):
        # footprints on one texel (dr = dc = 0: four addends), with generic weights
        k = 24
        parts.append(Records(m, rng.integers(0, h, k), rng.integers(0, w, k), 0, 0, rng.random(k), rng.random(k), rng.standard_normal((k, 3))))
        if h > TILE:        # the halo row: first texel in row 0 of the tile below, dr = 1 -> row 31 of the tile above
            k = w - 1
            parts.append(Records(m, TILE, np.arange(k), 1, 1, rng.random(k), rng.random(k), rng.standard_normal((k, 3))))
        if w > TILE:        # the halo column: first texel in column 31, dc = 1 -> column 0 of the tile to the right
            k = h - 1
            parts.append(Records(m, np.arange(1, h), TILE - 1, 1, 1, rng.random(k), rng.random(k), rng.standard_normal((k, 3))))
    rec = Records.cat(parts)
    return build(maps, sub, place(maps, rec, sub, rng)), None


COUNTS = [0, 1, 511, 512, 513, 1025, 7, 300, 0, 64, 2, 0, 129, 1, 0, 33]


def case_counts(sub):
    """64x64 map, four bins.  Bin 0: the counts above per sub-range; bin 1: empty; bin 2: three sub-ranges whose cursor exceeds the capacity;
    bin 3: random.  A layout with gaps; the test adds to a non-zero gradient buffer."""
    maps = maps_of([(64, 64)])
    rng = np.random.default_rng(11)
    placed = {}
    for s in range(sub):
        n = COUNTS[s % len(COUNTS)]
        if n:
            placed[(0, s)] = random_records(maps, n, rng, m=0, rows=(0, 32), cols=(0, 32))
    for s in (0, 3, sub - 1):
        placed[(2, s)] = random_records(maps, 40 + 200 * s % 97, rng, m=0, rows=(32, 64), cols=(0, 32))
    placed.update({k: v for k, v in place(maps, random_records(maps, 900, rng, m=0, rows=(32, 64), cols=(32, 64)), sub, rng).items()})
    extra = {(2, 0): 5, (2, 3): 700, (2, sub - 1): 1}
    return build(maps, sub, placed, gaps=[3, 0, 17, 1, 5], cursor_extra=extra, head=11), None


def phase_case(sub, phases, sep=1024, shape=(32, 32)):
    """One bin, sub-range 0: the phases in order with `sep` zero records between them -> (built, {(0, 0): exponent of every record's phase})"""
    maps = maps_of([shape])
    recs, exps = [], []
    for i, ph in enumerate(phases):
        if i:
            recs.append(zero_records(sep))
            exps.append(np.full(sep, BIN_FIX_EMIN))
        recs.append(ph)
        exps.append(np.full(len(ph), record_exponents(ph).max() if len(ph) else BIN_FIX_EMIN))
    return build(maps, sub, {(0, 0): Records.cat(recs)}), {(0, 0): np.concatenate(exps)}


def _decade_phases(descending):
    rng = np.random.default_rng(5)
    texels = [(4, 4), (4, 5), (17, 30), (31, 0)]
    out = []
    for k in range(11):                                    # 1e-20 ... 1e20: 40 decades
        n = 8
        t = rng.integers(0, len(texels), n)
        g = (rng.uniform(0.5, 1.0, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3)) * 10.0 ** (-20 + 4 * k)).astype(np.float32)
        out.append(Records(0, [texels[i][0] for i in t], [texels[i][1] for i in t], 1, 1, rng.random(n), rng.random(n), g))
    return out[::-1] if descending else out


def case_range(name, sub):
    rng = np.random.default_rng(7)
    if name in ('ascending', 'descending'):
        return phase_case(sub, _decade_phases(name == 'descending'))
    maps = maps_of([(32, 32)])
    if name == 'floor':                                    # below 2^-100: the exponent floor; some so small that they round away
        n = 300
        rec = random_records(maps, n, rng, halo=True)
        rec.wx1, rec.wy1 = (rng.integers(0, 17, n) / 16).astype(np.float32), (rng.integers(0, 17, n) / 16).astype(np.float32)
        mag = np.where(np.arange(n) % 10 == 0, np.ldexp(1.0, -125), np.ldexp(1.0, -104))
        rec.g = (rng.uniform(0.5, 1.0, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3)) * mag[:, None]).astype(np.float32)
        return build(maps, sub, place(maps, rec, 3, rng)), None
    if name == 'zero_batch':                               # live, 1024 zero records, live
        live = [random_records(maps, 600, rng) for _ in range(2)]
        return phase_case(sub, live)
    if name == 'cancel':                                   # +g ... then -g ...: every texel sums to exactly 0
        n = 400
        pos = random_records(maps, n, rng)
        pos.g = (rng.uniform(1.0, 1.99, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))).astype(np.float32)
        neg = pos[np.arange(n)]
        neg.g = -neg.g
        return build(maps, sub, {(0, 0): Records.cat([pos, neg])}), None
    raise KeyError(name)


RANGE_CASES = ['ascending', 'descending', 'floor', 'zero_batch', 'cancel']
BUDGET_G = 1.9                       # |g| < 2^1: round(1.9 * 2^19) = 996147 units per weight-1 record, 0.95 of the most a record can add
BUDGET_CASES = {'look_and_go_on': 2136, 'flush_and_clear': 2600}


def one_texel(n, g, R0=5, C0=5):
    """n weight-1 records on one texel: wx1 = wy1 = 0 gives w = (1, 0, 0, 0) exactly"""
    return Records(0, R0, C0, 1, 1, 0.0, 0.0, np.full((n, 3), g, dtype=np.float32))


def case_budget(name, sub):
    return build(maps_of([(32, 32)]), sub, {(0, 0): one_texel(BUDGET_CASES[name], BUDGET_G)}), None


# the rescale samples: (records on texel A, their gradient, sub-ranges); the batch that raises the exponent is one record g = 1.0 on texel B.
# d = the raise in bits.  One sub-range: phase 1, 1024 zero records, phase 2.  Two sub-ranges: phase 1 in sub-range 0, phase 2 in
# sub-range 1 -- batches never span sub-ranges, so the phases stay apart without zero records between them.
RESCALE_CASES = {
    'd41': (1500, 1.9 * 2.0 ** -41, 1),
    'd31': (1500, 1.9 * 2.0 ** -31, 1),
    'd30': (1900, 1.9 * 2.0 ** -30, 1),
    'd30_two_subranges': (1900, 1.9 * 2.0 ** -30, 2),
    'd31_two_subranges': (1500, 1.9 * 2.0 ** -31, 2),
}
TEXEL_A, TEXEL_B = (5, 5), (9, 9)


def case_rescale(name, sub):
    n, g, nsub = RESCALE_CASES[name]
    a, b = one_texel(n, g, *TEXEL_A), one_texel(1, 1.0, *TEXEL_B)
    if nsub == 1:
        return phase_case(sub, [a, b])
    maps = maps_of([(32, 32)])
    ea, eb = record_exponents(a), record_exponents(b)
    return build(maps, sub, {(0, 0): a, (0, 1): b}), {(0, 0): ea, (0, 1): eb}


def case_nonfinite(sub):
    """64x64, four bins of 300 records in sub-range 0, no footprint leaving its tile -> (clean, the same with a NaN and a +inf gradient
    in bin 2, bin 2)"""
    maps = maps_of([(64, 64)])
    rng = np.random.default_rng(13)
    rec = random_records(maps, 1200, rng, halo=False)
    clean = place(maps, rec, sub, only_sub=0)
    bad = one_texel(2, 1.0, 40, 10)
    bad.g[0, 1], bad.g[1, 2] = np.nan, np.inf
    dirty = dict(clean)
    r = clean[(2, 0)]
    dirty[(2, 0)] = Records.cat([r[np.arange(100)], bad, r[np.arange(100, len(r))]])
    return build(maps, sub, clean), build(maps, sub, dirty), 2
