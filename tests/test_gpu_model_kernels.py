"""The model-side kernels of csrc/texture.hip and csrc/model_ops.hip -- texture preparation, TV, composite + MSE, Adam and grouped Adam,
superquadric blocks, posed mesh, overlap, block opacities, parsimony -- called through the C ABI with raw pointers at the edges of their
launch geometry, against the float64 references of tests/model_kernels_ref.py evaluated on the same float32 inputs.  Every output is
prefilled with NaN (an accumulating one with a non-zero start value) and lies inside a larger buffer with 64 sentinel floats on either
side: the sentinels must be untouched and no NaN may be left.

THE METRIC, per output element: |got - ref64| / (M + tiny), M = the float64 sum of the absolute values of the terms that make up the
element (model_kernels_ref.py returns it next to every output), tiny = the smallest normal float32 x the number of summed terms; a
difference of at most tiny itself does not count (model_kernels_ref.err: sigmoid(-90) is below the normal float32 range).

THE BAR is not a chosen number (the convention of tests/test_gpu_lpips_head.py).  Per family torch's own float32 formulation of the
operation (model_kernels_ref.torch_*: the expressions tests/test_gpu_model.py uses as its references, torch.optim.Adam for Adam) runs on
the MI355X on the same inputs and is measured against the same float64 reference with the same metric.  The kernel's bar is 8 x the
largest such error over the family's cases (model_kernels_ref.TORCH_FP32, bar()), never looser than what test_gpu_model.py asks of the
family today (model_kernels_ref.FLOOR).  Every case measures torch again next to the kernel and records both (record_property).
G: the number of workgroups whose partial sums meet in one float32 atomic.  The loss values of TV (G up to 1024, 2048 in the `_sets`
launch) and of composite + MSE (G up to 512) are held to 8 x torch x sqrt(G), still capped by the floor: every atomic rounds the running
total once, in arrival order, where torch sums pairwise.  The overlap loss (G <= 20) is held to the plain 8 x torch.

Measured on the MI355X (the largest of the family's cases; the atomic sums differ from run to run within what G allows):

    family                torch fp32 value / gradient   kernel value / gradient     bar value / gradient      G
    texture preparation   4.22e-07 / 1.00e+00           1.54e-07 / 3.37e-07         1.00e-06 / 1.00e-04       -
    TV                    7.57e-08 / 2.05e-07           6.44e-07 / 2.16e-07         1.00e-05 / 1.64e-06       2048 (in the bar)
    composite + MSE       1.55e-07 / 2.67e-07           2.23e-07 / 2.67e-07         6.00e-06 / 2.14e-06       512 (in the bar)
    Adam, grouped Adam    1.84e-07 / -                  2.37e-07 / -                1.47e-06 / -              -
    superquadric blocks   1.74e-07 / 1.20e-05           2.72e-07 / 1.20e-05         1.39e-06 / 9.60e-05       -
    posed mesh            1.28e-07 / 3.71e-08           1.42e-07 / 3.71e-08         1.02e-06 / 2.97e-07       -
    overlap               2.18e-07 / 2.98e-05           1.23e-07 / 4.14e-05         1.74e-06 / 1.00e-04       20
    block opacities       2.62e-07 / 1.50e-07           2.62e-07 / 1.83e-07         1.00e-06 / 1.20e-06       -
    parsimony             5.24e-08 / 1.79e-07           9.06e-08 / 1.49e-07         4.19e-07 / 1.43e-06       -

(texture preparation, gradient: torch's float32 loses the whole gradient of a saturated texel -- s (1 - s) from the rounded s is 0 above a
logit of 16.6 -- so its error is 1 at the planted +20 and +90 and the bar is the floor.  The kernels did the same until this test: see
tex_sigmoid(x, one_minus_s) in csrc/texture_body.h.  Overlap, gradient: occupancy = sigmoid(-sdf / 0.005) turns every float32 rounding in
front of it into 200 x as much in the exponent; torch and the kernel read 1e-5 to 4e-5 alike and the bar is the floor.  The blocks'
gradient: the error of both sides is 1.8 se (1 - se) of a shape parameter near +8, from the rounded sigmoid.  The rows of the blocks and
of overlap were measured again after load_pose began to round the exponent once, model_math.h: sq_exponent -- the same to three digits.)

An accumulating output (the gradients of the blocks, the posed mesh, overlap and parsimony; the loss values) is launched twice: from zero,
so that it is held on the magnitude of its own terms alone, and from half of each element's own magnitude, so that the sum is checked
without the start value dwarfing what is added (starts()).  Constant start values are used only where the assertion is exact equality.

The tail launch (adam_groups_tex_kernel) is held bit-equal to dbw_texture_prep_bwd_sets + dbw_adam_step_groups in
tests/test_gpu_step_tail.py; both of those are held to float64 here.  The step's fused model-side kernels (step_prologue_kernel,
regularisers_kernel, blocks_tail_kernel, loss_finish_kernel) are held to the kernels of this file bit for bit and to the same float64
references in tests/test_gpu_step_kernels.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

import model_kernels_ref as R

pytestmark = pytest.mark.gpu

from dbw_amd import _lib                                        # noqa: E402

DEV = 'cuda:0'
NAN = float('nan')
GUARD = 64
SENTINEL = -12345.678
F32 = torch.float32
c_f, c_i64 = ctypes.c_float, ctypes.c_int64


# ---- buffers ------------------------------------------------------------------------------------------------------------------------------
class Out:
    """An output of `shape` inside a larger buffer, GUARD sentinels before and after it, prefilled with `fill`"""

    def __init__(self, shape, fill=NAN, dtype=F32):
        n = int(np.prod(shape))
        self.sent = SENTINEL if dtype.is_floating_point else -12345
        self.buf = torch.full((n + 2 * GUARD,), self.sent, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if torch.is_tensor(fill):
            self.t.copy_(fill.to(DEV).view(shape))
        else:
            self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr()

    def wrong(self, name):
        w = []
        if not bool((self.buf[:GUARD] == self.sent).all()) or not bool((self.buf[-GUARD:] == self.sent).all()):
            w.append(f'{name}: a sentinel next to the output was overwritten')
        if self.t.dtype.is_floating_point and bool(torch.isnan(self.t).any()):
            w.append(f'{name}: {int(torch.isnan(self.t).sum())} elements left NaN (unwritten)')
        return w

    def np(self):
        return self.t.detach().cpu().numpy()


def dev(x, dtype=F32):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(device=DEV, dtype=dtype).contiguous()


def ptr(t):
    return 0 if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def rnd(seed):
    return np.random.RandomState(seed)


def starts(M):
    """The two start values an accumulating output is run from.  Zero: the result is held to the bar on the magnitude of its own terms
    alone.  About half the element's magnitude, signs alternating: the kernel adds, and the sum is checked from a start that does not
    dwarf what is added (M of the sum = |start| + M: at most 1.5 x the element's own)."""
    M = np.asarray(M, dtype=np.float64)
    sign = np.where(np.arange(M.size).reshape(M.shape) % 2, -1.0, 1.0)
    return np.zeros(M.shape, np.float32), (0.5 * M * sign).astype(np.float32)


def filled(start):
    """an accumulating output that starts from `start` (numpy, any shape; a scalar becomes one float)"""
    start = np.asarray(start, dtype=np.float32)
    return Out(start.shape or (1,), torch.from_numpy(start.reshape(start.shape or (1,)).copy()))


class Figures:
    """The errors of one test: kernel and torch float32 per (family, value / gradient), largest over what the test compared"""

    def __init__(self, family, record):
        self.family, self.record, self.k, self.t, self.wrong = family, record, [0.0, 0.0], [0.0, 0.0], []

    def kernel(self, name, which, got, ref, M, count=1, G=1, start=None):
        """start: what an accumulating output held before the launch -- one more term of the sum"""
        if start is not None:
            got, ref, M = np.asarray(got).reshape(np.shape(ref)), ref + R.f64(start), M + np.abs(R.f64(start))
        e = R.err(got, ref, M, count)
        self.k[which] = max(self.k[which], e)
        b = R.bar(self.family, which, G)
        if not e <= b:
            self.wrong.append(f'{name}: {"value gradient".split()[which]} error {e:.3g} above the bar {b:.3g}')
        return e

    def torch(self, which, got, ref, M, count=1):
        self.t[which] = max(self.t[which], R.err(got, ref, M, count))

    def done(self, name, G=1):
        """G: of the value's bar (TV's loss: G workgroups meet in one atomic)"""
        kinds = ('value', 'grad')[:len(R.TORCH_FP32[self.family])]          # (Adam has values only)
        bars = [R.bar(self.family, w, G if w == 0 else 1) for w in range(len(kinds))]
        print(f'FIG {self.family} {name}: ' + ' | '.join(f'{key}: kernel {self.k[w]:.3g} torch fp32 {self.t[w]:.3g} bar {bars[w]:.3g}' for w, key in enumerate(kinds)))
        for w, key in enumerate(kinds):
            self.record(f'{name}.kernel_{key}', self.k[w])
            self.record(f'{name}.torch_fp32_{key}', self.t[w])
            self.record(f'{name}.bar_{key}', bars[w])
        assert not self.wrong, self.wrong


# ---- texture preparation ------------------------------------------------------------------------------------------------------------------
def texture(shape, seed):
    """randn logits with 0, +-20, +-90 planted first, last and in between (the sigmoid saturates, expf(90) overflows to inf)"""
    t = rnd(seed).randn(*shape, 3).astype(np.float32)
    flat = t.reshape(-1)
    n = flat.size
    for k, v in enumerate((0.0, 20.0, -20.0, 90.0, -90.0)):
        flat[(k * (n - 1)) // 4] = v
        if n > 40:
            flat[7 + 3 * k] = -v
    return t


PREP_CASES = [(d, s) for s in ((3, 16, 48), (2, 32, 16)) for d in (1, 2, 4, 8, 16)] + [
    (3, (2, 6, 9)), (16, (1, 16, 16)),
    (1, (1, 512, 384)),          # 589 824 elements: above the grid clamp (2048 x 256 = 524 288)
    (2, (1, 256, 192)),          # 12 288 cells x 64 lanes = 786 432
]


def run_prep_fwd(tex, d, with_sig=True):
    n, h, w, _ = tex.shape
    maps, sig = Out((n, h // d, w // d, 3)), Out((n, h, w, 3))
    _lib.call('dbw_texture_prep_fwd', tex.data_ptr(), n, h, w, d, maps.ptr, sig.ptr if with_sig else 0, stream())
    return maps, sig


def run_prep_bwd(tex, d, gmaps, gsig):
    n, h, w, _ = tex.shape
    gtex = Out((n, h, w, 3))
    _lib.call('dbw_texture_prep_bwd', tex.data_ptr(), n, h, w, d, gmaps.data_ptr(), ptr(gsig), gtex.ptr, stream())
    return gtex


@pytest.mark.parametrize('d,shape', PREP_CASES, ids=[f'd{d}-{"x".join(map(str, s))}' for d, s in PREP_CASES])
def test_texture_preparation_equals_float64(d, shape, record_property):
    n, h, w = shape
    tex_np = texture(shape, seed=d + h)
    g = rnd(100 + d + w)
    gmaps_np, gsig_np = g.randn(n, h // d, w // d, 3).astype(np.float32), g.randn(n, h, w, 3).astype(np.float32)
    gmaps_np.reshape(-1)[0] = 0.0
    tex, gmaps, gsig = dev(tex_np), dev(gmaps_np), dev(gsig_np)
    F = Figures('prep', record_property)
    fwd = R.texture_prep_fwd(tex_np, d)
    maps, sig = run_prep_fwd(tex, d)
    torch.cuda.synchronize()
    F.wrong += maps.wrong('maps') + sig.wrong('sig')
    F.kernel('maps', 0, maps.np(), fwd['maps'], fwd['M_maps'], d * d)
    F.kernel('sig', 0, sig.np(), fwd['sig'], fwd['M_sig'])
    if d == 1:                                  # sig_out may be NULL without decimation
        maps2, sig2 = run_prep_fwd(tex, d, with_sig=False)
        torch.cuda.synchronize()
        F.wrong += maps2.wrong('maps (sig_out NULL)')
        assert torch.equal(maps2.t, maps.t) and bool(torch.isnan(sig2.t).all())
    for name, gs_np, gs in (('gsig', gsig_np, gsig), ('gsig NULL', None, None)):
        bwd = R.texture_prep_bwd(tex_np, d, gmaps_np, gs_np)
        gtex = run_prep_bwd(tex, d, gmaps, gs)
        torch.cuda.synchronize()
        F.wrong += gtex.wrong(f'gtex ({name})')
        F.kernel(f'gtex ({name})', 1, gtex.np(), bwd['gtex'], bwd['M_gtex'], 2)
        t = R.torch_texture_prep(tex, d, gmaps, gs, F32, DEV)
        F.torch(1, t['gtex'], bwd['gtex'], bwd['M_gtex'], 2)
    F.torch(0, t['maps'], fwd['maps'], fwd['M_maps'], d * d)
    F.torch(0, t['sig'], fwd['sig'], fwd['M_sig'])
    F.done(f'd{d}-{n}x{h}x{w}')


def test_a_decimation_that_does_not_divide_the_map_is_refused():
    tex = dev(texture((1, 8, 8), 0))
    maps, sig = Out((1, 2, 2, 3)), Out((1, 8, 8, 3))
    assert _lib.load().dbw_texture_prep_fwd(tex.data_ptr(), 1, 8, 8, 3, maps.ptr, sig.ptr, stream()) != 0
    assert _lib.load().dbw_texture_prep_fwd(tex.data_ptr(), 1, 8, 8, 2, maps.ptr, 0, stream()) != 0          # sig_out is required when decimating
    torch.cuda.synchronize()
    assert bool(torch.isnan(maps.t).all()) and bool(torch.isnan(sig.t).all())


SETS = [(1, (1, 40, 24)), (2, (3, 16, 48)), (4, (2, 32, 16)), (16, (1, 16, 32))]          # MAX_SETS = 4 sets, the grid is sized by the largest


def test_texture_sets_launch_equals_float64_and_the_single_launches(record_property):
    F = Figures('prep', record_property)
    sets, outs, singles, refs = [], [], [], []
    for k, (d, (n, h, w)) in enumerate(SETS):
        tex_np = texture((n, h, w), 30 + k)
        g = rnd(40 + k)
        gmaps_np, gsig_np = g.randn(n, h // d, w // d, 3).astype(np.float32), g.randn(n, h, w, 3).astype(np.float32)
        tex, gmaps, gsig = dev(tex_np), dev(gmaps_np), (dev(gsig_np) if k % 2 == 0 else None)
        o = dict(maps=Out((n, h // d, w // d, 3)), sig=Out((n, h, w, 3)), gtex=Out((n, h, w, 3)))
        outs.append(o)
        refs.append((R.texture_prep_fwd(tex_np, d), R.texture_prep_bwd(tex_np, d, gmaps_np, gsig_np if k % 2 == 0 else None), d))
        t = R.torch_texture_prep(tex, d, gmaps, gsig, F32, DEV)
        F.torch(0, t['maps'], refs[-1][0]['maps'], refs[-1][0]['M_maps'], d * d)
        F.torch(0, t['sig'], refs[-1][0]['sig'], refs[-1][0]['M_sig'])
        F.torch(1, t['gtex'], refs[-1][1]['gtex'], refs[-1][1]['M_gtex'], 2)
        sets.append(dict(texture=tex.data_ptr(), n=n, h=h, w=w, decim=d, maps=o['maps'].ptr, sig=o['sig'].ptr, grad_maps=gmaps.data_ptr(),
                         grad_sig=ptr(gsig), grad_texture=o['gtex'].ptr))
        singles.append(run_prep_fwd(tex, d) + (run_prep_bwd(tex, d, gmaps, gsig),))
        sets[-1]['_keep'] = (tex, gmaps, gsig)
    arr, ns = _lib.texture_sets([{k: v for k, v in s.items() if k != '_keep'} for s in sets])
    _lib.call('dbw_texture_prep_fwd_sets', arr, ns, stream())
    _lib.call('dbw_texture_prep_bwd_sets', arr, ns, stream())
    torch.cuda.synchronize()
    for k, (o, s, (fwd, bwd, d)) in enumerate(zip(outs, singles, refs)):
        for key, single in zip(('maps', 'sig', 'gtex'), s):
            F.wrong += o[key].wrong(f'set {k} {key}')
            assert torch.equal(o[key].t.view(torch.int32), single.t.view(torch.int32)), (k, key)
        F.kernel(f'set {k} maps', 0, o['maps'].np(), fwd['maps'], fwd['M_maps'], d * d)
        F.kernel(f'set {k} sig', 0, o['sig'].np(), fwd['sig'], fwd['M_sig'])
        F.kernel(f'set {k} gtex', 1, o['gtex'].np(), bwd['gtex'], bwd['M_gtex'], 2)
    F.done('sets-d1-d2-d4-d16')


# ---- TV -----------------------------------------------------------------------------------------------------------------------------------
TV_SHAPES = [(1, 2, 2), (1, 2, 300), (3, 200, 5), (3, 200, 300)]          # w > 256: two x-workgroups, the second mostly idle; n h = 600 > 512 rows
TV_START = 0.25


def tv_groups(n, h, w):
    return math.ceil(w / 256) * min(n * h, 512)


@pytest.mark.parametrize('shape', TV_SHAPES, ids=['x'.join(map(str, s)) for s in TV_SHAPES])
def test_tv_equals_float64(shape, record_property):
    n, h, w = shape
    maps_np = rnd(7 + w).rand(n, h, w, 3).astype(np.float32)
    maps = dev(maps_np)
    F = Figures('tv', record_property)
    for wrap in (0, 1):
        for scale in (1.0, 0.37):
            ref = R.tv_l2sq(maps_np, wrap, scale)
            t = R.torch_tv(maps, wrap, scale, F32, DEV)
            F.torch(0, t['value'], ref['value'], ref['M_value'], ref['terms'])
            F.torch(1, t['grad'], ref['grad'], ref['M_grad'], 4)
            # the kernel adds into `loss`: from zero with the gradient, from half the value's size without it
            for with_grad, start in zip((True, False), starts(ref['M_value'])):
                loss, grad = filled(start), Out((n, h, w, 3))
                _lib.call('dbw_tv_l2sq', maps.data_ptr(), n, h, w, wrap, scale, loss.ptr, grad.ptr if with_grad else 0, stream())
                torch.cuda.synchronize()
                name = f'wrap {wrap} scale {scale} grad {with_grad}'
                F.wrong += loss.wrong(f'loss ({name})')
                F.kernel(f'loss ({name})', 0, loss.np()[0], ref['value'], ref['M_value'], ref['terms'], G=tv_groups(n, h, w), start=start)
                if with_grad:
                    F.wrong += grad.wrong(f'grad ({name})')
                    F.kernel(f'grad ({name})', 1, grad.np(), ref['grad'], ref['M_grad'], 4)
                else:
                    assert bool(torch.isnan(grad.t).all())
    record_property('G', tv_groups(n, h, w))
    F.done('x'.join(map(str, shape)) + f' G={tv_groups(n, h, w)}', G=tv_groups(n, h, w))


@pytest.mark.parametrize('shape', TV_SHAPES, ids=['x'.join(map(str, s)) for s in TV_SHAPES])
def test_tv_of_a_constant_map_leaves_the_loss_alone_and_gives_a_zero_gradient(shape):
    n, h, w = shape
    maps = torch.full((n, h, w, 3), 0.3, device=DEV)
    for wrap in (0, 1):
        loss, grad = Out((1,), TV_START), Out((n, h, w, 3))
        _lib.call('dbw_tv_l2sq', maps.data_ptr(), n, h, w, wrap, 0.37, loss.ptr, grad.ptr, stream())
        torch.cuda.synchronize()
        assert not loss.wrong('loss') + grad.wrong('grad')
        assert float(loss.t) == TV_START and bool((grad.t == 0).all())


@pytest.mark.parametrize('order', [(0, 1), (1, 0)], ids=['small-first', 'large-first'])
def test_tv_sets_launch_equals_float64_and_the_single_launches(order, record_property):
    """a (1,8,8) set next to a (3,200,300) one: the grid is sized by the largest set, the narrow one rides along"""
    F = Figures('tv', record_property)
    spec = [((1, 8, 8), 0, 0.1), ((3, 200, 300), 1, 0.37)]
    sets, outs, value, M, terms = [], [], 0.0, 0.0, 0
    for k in order:
        (n, h, w), wrap, scale = spec[k]
        m_np = rnd(20 + k).rand(n, h, w, 3).astype(np.float32)
        m = dev(m_np)
        ref = R.tv_l2sq(m_np, wrap, scale)
        t = R.torch_tv(m, wrap, scale, F32, DEV)
        F.torch(0, t['value'], ref['value'], ref['M_value'], ref['terms'])
        F.torch(1, t['grad'], ref['grad'], ref['M_grad'], 4)
        value, M, terms = value + ref['value'], M + ref['M_value'], terms + ref['terms']
        single_loss, single = Out((1,), 0.0), Out((n, h, w, 3))
        _lib.call('dbw_tv_l2sq', m.data_ptr(), n, h, w, wrap, scale, single_loss.ptr, single.ptr, stream())
        o = Out((n, h, w, 3))
        outs.append((o, single, ref, m))
        sets.append(dict(sig=m.data_ptr(), n=n, h=h, w=w, decim=1, wrap_x=wrap, tv_scale=scale, grad_sig_out=o.ptr))
    arr, ns = _lib.texture_sets(sets)
    start = starts(M)[order[0]]          # (from zero in one order, from half the value's size in the other)
    loss = filled(start)
    _lib.call('dbw_tv_l2sq_sets', arr, ns, loss.ptr, stream())
    torch.cuda.synchronize()
    F.wrong += loss.wrong('loss')
    F.kernel('loss', 0, loss.np()[0], value, M, terms, G=2 * tv_groups(3, 200, 300), start=start)          # (the grid of the largest set, once per set)
    for k, (o, single, ref, _) in enumerate(outs):
        F.wrong += o.wrong(f'set {k} grad')
        assert torch.equal(o.t.view(torch.int32), single.t.view(torch.int32)), k
        F.kernel(f'set {k} grad', 1, o.np(), ref['grad'], ref['M_grad'], 4)
    record_property('G', 2 * tv_groups(3, 200, 300))
    F.done('sets-' + '-'.join(map(str, order)) + f' G={2 * tv_groups(3, 200, 300)}', G=2 * tv_groups(3, 200, 300))


# ---- composite + MSE ------------------------------------------------------------------------------------------------------------------------
COMPOSITE_SHAPES = [(1, 1, 1), (2, 9, 11), (1, 32, 32), (1, 1, 1025), (3, 300, 600)]          # one full workgroup; 1 pixel in the second; 540 000 > 524 288
LOSS_START = 0.125


@pytest.mark.parametrize('shape', COMPOSITE_SHAPES, ids=['x'.join(map(str, s)) for s in COMPOSITE_SHAPES])
def test_composite_mse_equals_float64(shape, record_property):
    N, H, W = shape
    g = rnd(3 + W)
    fg_np, env_np, img_np = (g.rand(N, c, H, W).astype(np.float32) for c in (4, 4, 3))
    mask = fg_np[:, 3].reshape(-1)
    mask[0] = 1.0
    if mask.size > 2:
        mask[-1], mask[mask.size // 2] = 0.0, 1.0
    env_np[:, 3] = 7.0                                    # env's fourth plane is not read
    fg, env, img = dev(fg_np), dev(env_np), dev(img_np)
    scale, up = 1.0 / (N * 3 * H * W), 1.7
    up_dev = torch.full((1,), up, device=DEV)
    ref = R.composite_mse(fg_np, env_np, img_np, scale, up)
    P = N * 3 * H * W
    G = min(math.ceil(N * H * W / 1024), 512)          # workgroups whose partial sums meet in the loss's one atomic
    F = Figures('composite', record_property)
    t = R.torch_composite(fg, env, img, scale, up, F32, DEV)
    F.torch(0, t['value'], ref['value'], ref['M_value'], P)
    F.torch(0, t['rec'], ref['rec'], ref['M_rec'], 2)
    F.torch(1, t['gfg'], ref['gfg'], ref['M_gfg'], 9)
    F.torch(1, t['genv'], ref['genv'], ref['M_genv'], 3)
    rec_bar = min(R.bar('composite', 0), 1e-6)

    def call(img_, rec, loss, gfg, genv, sd):
        _lib.call('dbw_composite_mse', fg.data_ptr(), env.data_ptr(), ptr(img_), N, H, W, scale, ptr(sd), ptr_o(rec), ptr_o(loss), ptr_o(gfg), ptr_o(genv), stream())
        torch.cuda.synchronize()

    def ptr_o(o):
        return 0 if o is None else o.ptr
    # loss only
    zero, half = starts(ref['M_value'])          # the kernel adds into the loss: once from half the value's size, once from zero
    loss = filled(half)
    call(img, None, loss, None, None, None)
    F.wrong += loss.wrong('loss only')
    F.kernel('loss only', 0, loss.np()[0], ref['value'], ref['M_value'], P, G=G, start=half)
    # loss + gradients under the upstream scalar (+ rec)
    loss, rec, gfg, genv = filled(zero), Out((N, 3, H, W)), Out((N, 4, H, W)), Out((N, 4, H, W))
    call(img, rec, loss, gfg, genv, up_dev)
    for name, o in (('loss', loss), ('rec', rec), ('gfg', gfg), ('genv', genv)):
        F.wrong += o.wrong(name)
    F.kernel('loss', 0, loss.np()[0], ref['value'], ref['M_value'], P, G=G, start=zero)          # (the upstream scalar does not scale the value)
    e = F.kernel('rec', 0, rec.np(), ref['rec'], ref['M_rec'], 2)
    assert e <= rec_bar, ('rec', e, rec_bar)
    F.kernel('gfg', 1, gfg.np(), ref['gfg'], ref['M_gfg'], 9)
    F.kernel('genv', 1, genv.np(), ref['genv'], ref['M_genv'], 3)
    assert bool((genv.t[:, 3] == 0).all())
    # rec only, without images
    rec2 = Out((N, 3, H, W))
    call(None, rec2, None, None, None, None)
    F.wrong += rec2.wrong('rec only')
    assert torch.equal(rec2.t.view(torch.int32), rec.t.view(torch.int32))
    record_property('G', G)
    F.done('x'.join(map(str, shape)) + f' G={G}', G=G)


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------------
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8)
ADAM_N = [1, 255, 256, 257, 600001]
ADAM_STEPS = [1, 7, 100000]


def adam_state(n, seed):
    """p, g, m, v with planted elements: g = 0 with v = 0; |g| = 1e-30 (g^2 underflows); |g| = 1e15; m and g of opposite sign"""
    g_ = rnd(seed)
    p, g, m = g_.randn(n).astype(np.float32), g_.randn(n).astype(np.float32), (g_.randn(n) * 0.1).astype(np.float32)
    v = (g_.rand(n) * 0.01).astype(np.float32)
    if n >= 255:
        for base in (0, n - 8):
            g[base], v[base] = 0.0, 0.0
            g[base + 1], g[base + 2] = 1e-30, -1e-30
            v[base + 2] = 0.0
            g[base + 3], g[base + 4] = 1e15, -1e15
            m[base + 5], g[base + 5] = 0.5, -0.5
            m[base + 6], g[base + 6] = -0.05, 0.45          # beta1 m + (1 - beta1) g cancels to ~0
    else:
        g[0], v[0] = 0.0, 0.0
    return p, g, m, v


def check_adam(F, name, got, ref):
    for key in ('p', 'm', 'v'):
        F.wrong += got[key].wrong(f'{name} {key}')
        F.kernel(f'{name} {key}', 0, got[key].np(), ref[key], ref['M_' + key], 3)


@pytest.mark.parametrize('step', ADAM_STEPS)
@pytest.mark.parametrize('n', ADAM_N)
def test_adam_step_equals_float64(n, step, record_property):
    p, g, m, v = adam_state(n, seed=n % 1000 + step % 10)
    lr = 5e-3
    ref = R.adam(p, g, m, v, step, lr, **ADAM)
    F = Figures('adam', record_property)
    t = R.torch_adam(p, g, m, v, step, lr, ADAM['beta1'], ADAM['beta2'], ADAM['eps'], F32, DEV)
    for key in ('p', 'm', 'v'):
        F.torch(0, t[key], ref[key], ref['M_' + key], 3)
    got = {k: Out((n,), torch.from_numpy(x)) for k, x in (('p', p), ('m', m), ('v', v))}
    gd = dev(g)
    _lib.call('dbw_adam_step', got['p'].ptr, gd.data_ptr(), got['m'].ptr, got['v'].ptr, n, lr, ADAM['beta1'], ADAM['beta2'], ADAM['eps'], step, stream())
    torch.cuda.synchronize()
    check_adam(F, 'adam', got, ref)
    F.done(f'n{n}-step{step}')


# (group ends, n): boundaries that are no multiples of 256, an empty group in the middle, an empty first group
ADAM_GROUPS = {
    'one-group': ([600001], 600001),
    'two-groups': ([77, 1000], 1000),
    'three-groups-empty-middle': ([333, 333, 1000], 1000),
    'four-groups-empty-first': ([0, 257, 300001, 600001], 600001),
    'four-groups': ([10, 133, 201, 255], 255),
}
GROUP_LR = [5e-3, 5e-2, 1e-3, 2e-2]
ZERO_BYTES = [0, 16, 4096, 16 * (2048 * 256 + 5)]


@pytest.mark.parametrize('skip', [None, 0.0, 1.0], ids=['skip-null', 'skip-0', 'skip-1'])
@pytest.mark.parametrize('name', list(ADAM_GROUPS))
def test_grouped_adam_equals_float64_and_clears_the_arena(name, skip, record_property):
    ends, n = ADAM_GROUPS[name]
    step = 7
    p, g, m, v = adam_state(n, seed=len(ends) + n % 100)
    lrs = GROUP_LR[:len(ends)]
    ref = R.adam(p, g, m, v, step, R.group_lr(ends, lrs, n), **ADAM)
    F = Figures('adam', record_property)
    t = R.torch_adam(p, g, m, v, step, lrs, ADAM['beta1'], ADAM['beta2'], ADAM['eps'], F32, DEV, group_end=ends)
    for key in ('p', 'm', 'v'):
        F.torch(0, t[key], ref[key], ref['M_' + key], 3)
    gd = dev(g)
    flag = None if skip is None else torch.full((1,), skip, device=DEV)
    for zb in ZERO_BYTES:
        got = {k: Out((n,), torch.from_numpy(x)) for k, x in (('p', p), ('m', m), ('v', v))}
        arena = Out((max(zb, 16) // 4,), 3.5)
        _lib.call('dbw_adam_step_groups', got['p'].ptr, gd.data_ptr(), got['m'].ptr, got['v'].ptr, (c_i64 * len(ends))(*ends), (c_f * len(ends))(*lrs),
                  len(ends), ADAM['beta1'], ADAM['beta2'], ADAM['eps'], step, arena.ptr if zb else 0, zb, ptr(flag), stream())
        torch.cuda.synchronize()
        F.wrong += arena.wrong(f'arena of {zb} bytes')
        cleared = arena.t[:zb // 4]
        assert int(cleared.count_nonzero()) == 0 and bool((arena.t[zb // 4:] == 3.5).all()), zb          # the arena is cleared whatever the flag says
        if skip:
            for k, x in (('p', p), ('m', m), ('v', v)):                                                      # a skipped step moves nothing
                assert not got[k].wrong(k) and torch.equal(got[k].t.cpu(), torch.from_numpy(x)), k
        else:
            check_adam(F, f'zero_bytes {zb}', got, ref)
    F.done(f'{name}-skip{skip}')


# ---- superquadric blocks --------------------------------------------------------------------------------------------------------------------
BLOCK_CONSTS = dict(ratio=0.5, scale_min=0.2, S_world=0.5)
BLOCK_CASES = [(1, 1), (5, 42), (5, 64), (5, 65), (1, 162), (64, 65), (5, 162)]          # (Kb, nv): the vertex loop of one wave runs 1, 2 and 3 times
GRAD_START = 0.75


def world(seed):
    g = rnd(seed)
    return g.randn(3, 3).astype(np.float32), g.randn(3).astype(np.float32)


def block_params(Kb, nv, seed):
    """sq_eps from -8 to 8 (exponents 0.1 ... 1.9), 6D vectors random and not orthonormal, a trig table of arbitrary angles with vertices
    whose cos or sin is exactly 0 and +-1 (the pole: spow's derivative in the exponent is 0 there)"""
    g = rnd(seed)
    sq = np.stack([np.linspace(-8, 8, Kb), np.linspace(8, -8, Kb)], 1) if Kb > 1 else np.array([[-8.0, 8.0]])
    sq = (sq + g.randn(Kb, 2) * 0.3).astype(np.float32)
    S, R6, T = (g.randn(Kb, 3) * 0.3).astype(np.float32), g.randn(Kb, 6).astype(np.float32), g.randn(Kb, 3).astype(np.float32)
    eta, om = g.rand(Kb, nv) * np.pi - np.pi / 2, g.rand(Kb, nv) * 2 * np.pi - np.pi
    trig = np.stack([np.cos(eta), np.sin(eta), np.cos(om), np.sin(om)]).astype(np.float32)
    poles = [(0.0, 1.0, 1.0, 0.0), (0.0, -1.0, 0.0, 1.0), (1.0, 0.0, -1.0, 0.0), (1.0, 0.0, 0.0, -1.0)]
    for k in range(Kb):
        for j, pole in enumerate(poles):
            v = (j * (nv - 1)) // 3 if nv > 3 else None
            if v is not None:
                trig[:, k, v] = pole
    if nv == 1:
        trig[:, 0, 0] = poles[0]
    return sq, S, R6, T, trig


BLOCK_GRADS = ('g_sq_eps', 'g_S', 'g_R6', 'g_T')


def run_blocks(P, keep, dense, Kb, nv, Rw, Tw, gverts, NB, start=None):
    """start: key -> what the accumulating gradients hold before the launch (default: GRAD_START everywhere)"""
    sq, S, R6, T, trig = P
    rows = NB if dense else Kb
    verts = Out((rows, nv, 3))
    kp = ptr(keep)
    c = BLOCK_CONSTS
    _lib.call('dbw_sq_blocks_fwd', sq.data_ptr(), S.data_ptr(), R6.data_ptr(), T.data_ptr(), trig.data_ptr(), kp, dense, Kb, nv, c['ratio'], c['scale_min'],
              c['S_world'], Rw.data_ptr(), Tw.data_ptr(), verts.ptr, stream())
    grads = {k: Out(s, GRAD_START) if start is None else filled(start[k]) for k, s in zip(BLOCK_GRADS, ((Kb, 2), (Kb, 3), (Kb, 6), (Kb, 3)))}
    _lib.call('dbw_sq_blocks_bwd', sq.data_ptr(), S.data_ptr(), R6.data_ptr(), T.data_ptr(), trig.data_ptr(), kp, dense, Kb, nv, c['ratio'], c['scale_min'],
              c['S_world'], Rw.data_ptr(), gverts.data_ptr(), grads['g_sq_eps'].ptr, grads['g_S'].ptr, grads['g_R6'].ptr, grads['g_T'].ptr, stream())
    torch.cuda.synchronize()
    return verts, grads


def keep_masks(Kb):
    if Kb == 1:
        return {'one': [1]}
    only = lambda i: [int(k == i) for k in range(Kb)]
    return {'all': [1] * Kb, 'first-only': only(0), 'last-only': only(Kb - 1), 'alternating': [k % 2 for k in range(Kb)],
            'alternating-from-0': [(k + 1) % 2 for k in range(Kb)], 'middle-only': only(Kb // 2)}


@pytest.mark.parametrize('Kb,nv', BLOCK_CASES, ids=[f'kb{k}-nv{v}' for k, v in BLOCK_CASES])
def test_superquadric_blocks_equal_float64(Kb, nv, record_property):
    P_np = block_params(Kb, nv, seed=Kb + nv)
    Rw_np, Tw_np = world(5)
    gv_np = rnd(9 + nv).randn(Kb, nv, 3).astype(np.float32)
    c = BLOCK_CONSTS
    ref = R.sq_blocks(*P_np, c['ratio'], c['scale_min'], c['S_world'], Rw_np, Tw_np, gv_np)
    P, Rw, Tw, gv = [dev(x) for x in P_np], dev(Rw_np), dev(Tw_np), dev(gv_np)
    F = Figures('blocks', record_property)
    t = R.torch_sq_blocks(*P, c['ratio'], c['scale_min'], c['S_world'], Rw, Tw, gv, F32, DEV)
    F.torch(0, t['verts'], ref['verts'], ref['M_verts'], 7)
    for key in ('g_sq_eps', 'g_S', 'g_R6', 'g_T'):
        F.torch(1, t[key], ref[key], ref['M_' + key], nv * 9)
    # the gradients accumulate: from zero (held on their own magnitude) and from half of it (the sum)
    for which in (0, 1):
        start = {key: starts(ref['M_' + key])[which] for key in BLOCK_GRADS}
        full, grads = run_blocks(P, None, 0, Kb, nv, Rw, Tw, gv, Kb, start)
        F.wrong += full.wrong('verts')
        F.kernel('verts', 0, full.np(), ref['verts'], ref['M_verts'], 7)
        for key, o in grads.items():
            F.wrong += o.wrong(key)
            F.kernel(f'{key} (start {which})', 1, o.np(), ref[key], ref['M_' + key], nv * 9, start=start[key])
    full, grads = run_blocks(P, None, 0, Kb, nv, Rw, Tw, gv, Kb)          # from GRAD_START: what the masked launches below are compared with, bit for bit
    for name, mask in keep_masks(Kb).items():
        keep = torch.tensor(mask, dtype=torch.int32, device=DEV)
        alive = keep.bool()
        NB = int(alive.sum())
        # dense = 1: the kept blocks packed in order, bit-equal to the rows of the unmasked result
        v1, g1 = run_blocks(P, keep, 1, Kb, nv, Rw, Tw, gv[alive].contiguous(), NB)
        F.wrong += v1.wrong(f'verts (dense, {name})')
        assert torch.equal(v1.t.view(torch.int32), full.t[alive].view(torch.int32)), name
        # dense = 0: every block keeps its slot, a dead block is exactly zero vertices and gets exactly no gradient
        v0, g0 = run_blocks(P, keep, 0, Kb, nv, Rw, Tw, gv, Kb)
        F.wrong += v0.wrong(f'verts (slots, {name})')
        assert torch.equal(v0.t[alive].view(torch.int32), full.t[alive].view(torch.int32)) and bool((v0.t[~alive] == 0).all()), name
        for key in grads:
            for g_ in (g1, g0):
                F.wrong += g_[key].wrong(f'{key} ({name})')
                assert torch.equal(g_[key].t[alive].view(torch.int32), grads[key].t[alive].view(torch.int32)), (name, key)
                assert bool((g_[key].t[~alive] == GRAD_START).all()), (name, key)
    F.done(f'kb{Kb}-nv{nv}')


# ---- posed mesh (the ground) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nv', [1, 64, 65, 1000])
def test_posed_mesh_equals_float64(nv, record_property):
    g = rnd(nv)
    base_np, R6_np, T_np, gv_np = g.randn(nv, 3).astype(np.float32), g.randn(6).astype(np.float32), g.randn(3).astype(np.float32), g.randn(nv, 3).astype(np.float32)
    Rw_np, Tw_np = world(6)
    S_world = BLOCK_CONSTS['S_world']
    ref = R.posed_mesh(base_np, R6_np, T_np, S_world, Rw_np, Tw_np, gv_np)
    base, R6, T, gv, Rw, Tw = (dev(x) for x in (base_np, R6_np, T_np, gv_np, Rw_np, Tw_np))
    F = Figures('mesh', record_property)
    t = R.torch_posed_mesh(base, R6, T, S_world, Rw, Tw, gv, F32, DEV)
    F.torch(0, t['verts'], ref['verts'], ref['M_verts'], 7)
    for key in ('g_R6', 'g_T'):
        F.torch(1, t[key], ref[key], ref['M_' + key], nv * 9)
    for which in (0, 1):          # the gradients accumulate: from zero (held on their own magnitude) and from half of it (the sum)
        start = {key: starts(ref['M_' + key])[which] for key in ('g_R6', 'g_T')}
        verts, g6, gT = Out((nv, 3)), filled(start['g_R6']), filled(start['g_T'])
        _lib.call('dbw_posed_mesh_fwd', base.data_ptr(), nv, R6.data_ptr(), T.data_ptr(), S_world, Rw.data_ptr(), Tw.data_ptr(), verts.ptr, stream())
        _lib.call('dbw_posed_mesh_bwd', base.data_ptr(), nv, R6.data_ptr(), T.data_ptr(), S_world, Rw.data_ptr(), gv.data_ptr(), g6.ptr, gT.ptr, stream())
        torch.cuda.synchronize()
        F.wrong += verts.wrong('verts') + g6.wrong('g_R6') + gT.wrong('g_T')
        F.kernel('verts', 0, verts.np(), ref['verts'], ref['M_verts'], 7)
        for key, o in (('g_R6', g6), ('g_T', gT)):
            F.kernel(f'{key} (start {which})', 1, o.np(), ref[key], ref['M_' + key], nv * 9, start=start[key])
    F.done(f'nv{nv}')


# ---- overlap --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(R.OVERLAP_CASES))
def test_overlap_equals_float64(name, record_property):
    c = R.overlap_case(name)
    ref = R.overlap_ref(c)
    assert R.well_conditioned(ref['cond']), ref['cond']          # (tests/test_model_kernels_ref_host.py asserts the same without a GPU)
    Kb, npts = c['Kb'], c['npts']
    keys = R.OVERLAP_GRADS
    d = {k: dev(c[k]) for k in ('u', 'sq_eps', 'S', 'R6', 'T', 'alpha')}
    F = Figures('overlap', record_property)
    t = R.torch_overlap(d['u'], d['sq_eps'], d['S'], d['R6'], d['T'], d['alpha'], c['ratio'], c['scale_min'], c['temperature'], c['thresh'], c['scale'], F32, DEV)
    P = Kb * npts
    F.torch(0, t['value'], ref['value'], ref['M_value'], P)
    for k in keys:
        F.torch(1, t[k], ref[k], ref['M_' + k], P * 9)
    def launch(loss, outs):
        ws = Out((Kb * 18,), 0.0)
        _lib.call('dbw_overlap_loss', d['u'].data_ptr(), npts, d['sq_eps'].data_ptr(), d['S'].data_ptr(), d['R6'].data_ptr(), d['T'].data_ptr(), d['alpha'].data_ptr(),
                  Kb, c['ratio'], c['scale_min'], c['temperature'], c['thresh'], c['scale'], loss.ptr, *[outs[k].ptr for k in keys], ws.ptr, stream())
        torch.cuda.synchronize()
        return loss.wrong('loss') + ws.wrong('workspace') + sum((outs[k].wrong(k) for k in keys), [])
    if ref['cond']['active'] == 0:                                # below the threshold everywhere: exactly nothing is added anywhere
        loss, outs = Out((1,), LOSS_START), {k: Out(ref[k].shape, GRAD_START) for k in keys}
        F.wrong += launch(loss, outs)
        assert ref['value'] == 0 and float(loss.t) == LOSS_START
        for k in keys:
            assert bool((outs[k].t == GRAD_START).all()), k
    else:
        assert ref['value'] > 1e-3
        # the loss and the gradients accumulate: from zero (held on their own magnitude) and from half of it (the sum)
        for which in (0, 1):
            start = {k: starts(ref['M_' + k])[which] for k in keys + ('value',)}
            loss, outs = filled(start['value']), {k: filled(start[k]) for k in keys}
            F.wrong += launch(loss, outs)
            F.kernel(f'loss (start {which})', 0, loss.np()[0], ref['value'], ref['M_value'], P, start=start['value'])
            for k in keys:
                F.kernel(f'{k} (start {which})', 1, outs[k].np(), ref[k], ref['M_' + k], P * 9, start=start[k])
    G = math.ceil(P / 256)
    record_property('G', G)
    F.done(f'{name} G={G}')


# ---- block opacities and parsimony ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Kb', R.ALPHA_KB)
def test_block_opacities_equal_float64(Kb, record_property):
    lg_np, nz_np = R.alpha_logits(Kb)
    assert R.alpha_margin(lg_np) > R.ALPHA_MARGIN          # no logit within 1e-3 of logit(thresh): the mask is the float64 one, none left out
    g = rnd(Kb)
    lg, nz = dev(lg_np), dev(nz_np)
    F = Figures('alpha', record_property)
    for thresh in R.ALPHA_THRESH:
        for noise_np, noise in ((None, None), (nz_np, nz)):
            ref = R.block_alpha_fwd(lg_np, noise_np, 0.3, thresh)
            alpha, full, keep = Out((Kb,)), Out((Kb,)), Out((Kb,), -7, torch.int32)
            _lib.call('dbw_block_alpha_fwd', lg.data_ptr(), ptr(noise), 0.3, thresh, Kb, alpha.ptr, full.ptr, keep.ptr, stream())
            torch.cuda.synchronize()
            name = f'thresh {thresh} noise {noise is not None}'
            F.wrong += alpha.wrong(f'alpha ({name})') + full.wrong(f'alpha_full ({name})') + keep.wrong(f'keep ({name})')
            assert np.array_equal(keep.np() != 0, ref['keep']) and set(np.unique(keep.np())) <= {0, 1}, name
            F.kernel(f'alpha ({name})', 0, alpha.np(), ref['alpha'], ref['M_alpha'])
            F.kernel(f'alpha_full ({name})', 0, full.np(), ref['alpha_full'], ref['M_alpha_full'])
            alpha2, full2 = Out((Kb,)), Out((Kb,))                                           # keep may be NULL
            _lib.call('dbw_block_alpha_fwd', lg.data_ptr(), ptr(noise), 0.3, thresh, Kb, alpha2.ptr, full2.ptr, 0, stream())
            torch.cuda.synchronize()
            assert torch.equal(alpha2.t, alpha.t) and torch.equal(full2.t, full.t) and not alpha2.wrong('') + full2.wrong('')
            for parts in (1, 3):
                ga_np, gf_np = g.randn(Kb, parts).astype(np.float32), g.randn(Kb).astype(np.float32)
                ga, gf = dev(ga_np), dev(gf_np)
                t = R.torch_block_alpha(lg, noise, 0.3, thresh, ga, gf, F32, DEV)
                F.torch(0, t['alpha'], ref['alpha'], ref['M_alpha'])
                F.torch(0, t['alpha_full'], ref['alpha_full'], ref['M_alpha_full'])
                # the backward reads the float32 alpha the forward wrote: the reference takes the same
                for what, a_, f_ in (('both', (ga_np, ga), (gf_np, gf)), ('g_alpha NULL', (None, None), (gf_np, gf)), ('g_alpha_full NULL', (ga_np, ga), (None, None))):
                    bref = R.block_alpha_bwd(alpha.np(), keep.np(), a_[0], f_[0])
                    gl = Out((Kb,))
                    _lib.call('dbw_block_alpha_bwd', alpha.ptr, keep.ptr, ptr(a_[1]), parts, ptr(f_[1]), Kb, gl.ptr, stream())
                    torch.cuda.synchronize()
                    F.wrong += gl.wrong(f'g_logit ({name}, {what})')
                    F.kernel(f'g_logit ({name}, parts {parts}, {what})', 1, gl.np(), bref['g_logit'], bref['M_g_logit'], parts + 1)
                    if what == 'both':
                        F.torch(1, t['g_logit'], bref['g_logit'], bref['M_g_logit'], parts + 1)
    F.done(f'kb{Kb}')


@pytest.mark.parametrize('n', R.PARSIMONY_N)
def test_parsimony_equals_float64(n, record_property):
    x_np = R.parsimony_values(n)
    assert R.parsimony_margin(x_np) > 1e-4
    eps, scale = R.PARSIMONY_EPS, 0.01
    ref = R.sqrt_mean(x_np, eps, scale)
    x = dev(x_np)
    F = Figures('parsimony', record_property)
    t = R.torch_sqrt_mean(x, eps, scale, F32, DEV)
    F.torch(0, t['value'], ref['value'], ref['M_value'], n)
    off = x_np != np.float32(eps)          # at x == eps torch.clamp's backward passes the gradient, the kernel's `x > eps` does not: the reference takes the kernel's side
    F.torch(1, t['grad'][off], ref['grad'][off], ref['M_grad'][off], 2)
    below = x_np <= np.float32(eps)
    # loss and gradient accumulate: from zero (held on their own magnitude) and from half of it (the sum); at or below the clamp, where
    # nothing is added, the gradient starts from GRAD_START and must keep it exactly
    for which, with_loss, with_grad in ((0, True, True), (1, True, True), (1, True, False), (1, False, True)):
        ls, gs = starts(ref['M_value'])[which], starts(ref['M_grad'])[which]
        gs[below] = GRAD_START
        loss, grad = filled(ls), filled(gs)
        _lib.call('dbw_sqrt_mean', x.data_ptr(), n, eps, scale, loss.ptr if with_loss else 0, grad.ptr if with_grad else 0, stream())
        torch.cuda.synchronize()
        F.wrong += loss.wrong('loss') + grad.wrong('grad')
        if with_loss:
            F.kernel(f'loss (start {which})', 0, loss.np()[0], ref['value'], ref['M_value'], n, start=ls)
        else:
            assert float(loss.t) == float(ls)
        if with_grad:
            F.kernel(f'grad (start {which})', 1, grad.np(), ref['grad'], ref['M_grad'], 2, start=gs)
            assert np.array_equal(grad.np()[below], gs[below])          # nothing is added at or below the clamp
        else:
            assert np.array_equal(grad.np(), gs)
    F.done(f'n{n}')
