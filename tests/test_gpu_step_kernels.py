"""The four fused model-side kernels of the one-call training step -- step_prologue_kernel, regularisers_kernel, blocks_tail_kernel
(csrc/model_ops.hip) and loss_finish_kernel (csrc/train_step.hip) -- launched on their own through the undeclared exports
dbw_debug_step_prologue / _regularisers / _blocks_tail / _loss_finish (flat arguments -> the step's own launchers), at the edges of their
launch geometry.  Every kernel is held twice:

  A  the claim of csrc/step_kernels.h: bit-equal (int32 views) to the operator-level kernels it replaces on identical inputs, wherever both
     sides add in the same order (dbw_block_alpha_fwd, dbw_sq_blocks_fwd / _bwd with keep and dense = 0, dbw_posed_mesh_fwd,
     dbw_texture_prep_fwd_sets, dbw_block_alpha_bwd, dbw_overlap_loss then dbw_sqrt_mean);
  B  element-wise against the float64 references of tests/model_kernels_ref.py with the metric and the bars of
     tests/test_gpu_model_kernels.py (its docstring: err, M, bar = 8 x torch float32, floored; accumulating outputs from zero and from
     starts()).  sq_local (the block-frame point and its two exponent derivatives the prologue keeps for the tail) and the loss values have
     no operator twin: B is their only judge.

The regularisers launch and A (bitwise_keys): the overlap term's 18 raw gradients per block meet in LDS float32 atomics, which have one
order only while one wave adds (up to 64 samples: all outputs and the workspace are bit-equal there, with 64 blocks too); its VALUE has no
LDS atomic in it and is bit-equal while the launch has one workgroup (256 samples); the parsimony value always.  Beyond that B only, G =
the number of workgroups in the value's bar.  The opacities the prologue draws itself (Philox) are held to sigmoid(logit + scale * normal)
of the HOST build of csrc/rng_math.h (tests/host_model_math.cpp) -- B only: the device's logf / cosf are not the host's.  The regularisers'
own samples (Philox) are compared on the first step counter whose draws keep the conditions of the fixed cases (no sample near a branch
of the reference; torch's float32 on the CPU within half the gradient floor: model_kernels_ref.overlap_float32_cost, a selection that
has no kernel in it but does leave out the draws on which float32 itself flips a branch).  That search ends on step 0 for each of the
three cases (PHILOX_STEP, asserted).

No case exists for one conceivable slip, on purpose: a vertex loop of the prologue that strides by 64 instead of its 256 threads changes no
output -- the threads then rewrite one another's vertices with identical values -- so no test can see it.

Measured on the MI355X (the largest over the cases of this file; `torch fp32`: torch's float32 formulation of the same operation on the
same inputs against the same float64 reference):

    kernel         output                                      kernel      torch fp32   bar
    prologue       alpha, alpha_full (value)                   2.69e-07    2.69e-07     1.00e-06
    prologue       blk_verts (value)                           2.72e-07    3.55e-07     1.39e-06
    prologue       sq_local: point, d/deps1, d/deps2 (value)   5.69e-07    1.65e-06     1.39e-06
    prologue       ground_verts (value)                        1.29e-07    1.21e-07     1.02e-06
    prologue       maps, sig (value)                           1.20e-07    1.76e-07     1.00e-06
    blocks tail    g_sq_eps, g_S, g_R6, g_T (gradient)         3.42e-05    3.42e-05     9.60e-05
    blocks tail    g_logit (gradient)                          1.57e-07    1.44e-07     1.20e-06
    regularisers   loss_overlap (value, G <= 10 in the bar)    2.55e-07    2.63e-07     1.74e-06 ... 5.52e-06
    regularisers   overlap gradients, g_alpha_full, ws (grad.)  3.93e-05    3.09e-05     1.00e-04
    regularisers   the same, samples from Philox (gradient)    2.27e-05    3.76e-05     1.00e-04   (atomic sums: 1.8e-05 in another run)
    regularisers   loss_parsimony (value)                      8.46e-08    1.07e-07     4.19e-07
    regularisers   g_alpha_full, parsimony alone (gradient)    9.13e-08    1.09e-07     1.43e-06
    loss finish    rgb, the raw sum (value, G = 32 in the bar) 9.65e-08    6.44e-08     6.00e-06

(sq_local: torch's float32 misses the bar and the kernel did until this test -- the exponent 1.8 sigmoid(sq_eps) + 0.1 in float32; see
test_prologue_kept_points_equal_float64.  Every case writes its own figures through record_property.)
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import model_kernels_ref as R
import test_host_model_math as HM
from test_gpu_model_kernels import BLOCK_CONSTS, BLOCK_GRADS, DEV, F32, Figures, Out, block_params, dev, filled, ptr, rnd, starts, stream, texture, world

pytestmark = pytest.mark.gpu

from dbw_amd import _lib                                        # noqa: E402

c_p, c_i, c_f, c_u64, c_i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_uint64, ctypes.c_int64
# the undeclared exports (tests only: not in include/, not in _lib.SIGNATURES), arguments in the order of the structs of csrc/step_kernels.h
DEBUG = {
    'dbw_debug_step_prologue': [c_p, c_i, c_p, c_p, c_f, c_f, c_i, c_p, c_p, c_p, c_u64, c_u64] + [c_p] * 5 + [c_i, c_f, c_f, c_f] + [c_p] * 5 + [c_i] + [c_p] * 4
                               + [c_i, c_p],
    'dbw_debug_regularisers': [c_p, c_i, c_u64, c_u64] + [c_p] * 5 + [c_i] + [c_f] * 7 + [c_p] * 10,
    'dbw_debug_blocks_tail': [c_p] * 6 + [c_i, c_i, c_f, c_f] + [c_p] * 9 + [c_i] + [c_p] * 4,
    'dbw_debug_loss_finish': [c_p, c_i64, c_f, c_f, c_p, c_p, c_p],
}


def debug_rc(name, *args):
    lib = _lib.load()
    fn = getattr(lib, name)
    fn.argtypes, fn.restype = DEBUG[name], c_i
    assert len(args) == len(DEBUG[name]), (name, len(args), len(DEBUG[name]))
    return fn(*args), lib


def debug(name, *args):
    rc, lib = debug_rc(name, *args)
    assert rc == 0, (name, rc, lib.dbw_last_error().decode())


def bits(a, b):
    a, b = (x.t if isinstance(x, Out) else x for x in (a, b))
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ==== step_prologue_kernel ==============================================================================================================
NB = (1, 3, 64)                                   # 64 = MAX_KB
NV = (1, 63, 64, 65, 255, 256, 257)               # the 64-lane stride of sq_blocks_fwd_kernel and of the tail, the 256-thread stride of the prologue
PATTERN = (2.0, -6.0, 0.0, 0.3)                   # under thresh 0.5: alive, dead, dead (sigmoid(0) is exactly 0.5 and `> 0.5` is false), alive
NOISE_SCALE = 0.3
SEED, RNG_STEP = 227391, 5
# the opacity modes of one (nb, nv) case; with them rotate ngv in {1, 257}, the number of texture sets in {0, 1, 3} and nzero0 in {0, 1, 300}
MODES = [dict(name='no-mask', thresh=-1.0, shift=None, noise=None), dict(name='mask', thresh=0.5, shift=0, noise=None),
         dict(name='mask-shifted', thresh=0.5, shift=1, noise=None), dict(name='noise', thresh=0.5, shift=0, noise='caller'),
         dict(name='philox', thresh=0.5, shift=0, noise='philox'), dict(name='noise-ignored', thresh=0.5, shift=0, noise='ignored')]
TEX_SHAPES = [(1, (2, 5, 7)), (8, (1, 16, 24)), (1, (2, 5, 7))]          # (decimation, (n, h, w)): tiny maps, far less work than the (nb + 1) x 256 of the blocks
NGV, NSETS, NZERO = (1, 257), (0, 1, 3), (0, 1, 300)
ZERO_FILL = 3.5


def host_noise(seed, step, n):
    L = HM.lib()
    L.host_step_noise.argtypes = [c_u64, c_u64, c_i, c_p]
    z = np.empty(n, np.float32)
    L.host_step_noise(seed, step, n, z.ctypes.data_as(c_p))
    return z


def host_uniform(seed, step, n):
    L = HM.lib()
    L.host_step_uniform.argtypes = [c_u64, c_u64, c_i, c_p]
    u = np.empty((n, 3), np.float32)
    L.host_step_uniform(seed, step, n, u.ctypes.data_as(c_p))
    return u


def logits(nb, shift):
    if shift is None:
        return R.alpha_logits(nb)[0]
    return np.array([PATTERN[(k + shift) % 4] for k in range(nb)], np.float32)


class Scene:
    """the inputs of one (nb, nv) case on the device, and their float64 references"""

    def __init__(self, nb, nv):
        self.nb, self.nv = nb, nv
        self.P_np = block_params(nb, nv, seed=nb + nv)
        self.Rw_np, self.Tw_np = world(5)
        self.P, self.Rw, self.Tw = [dev(x) for x in self.P_np], dev(self.Rw_np), dev(self.Tw_np)
        c = BLOCK_CONSTS
        self.consts = (c['ratio'], c['scale_min'], c['S_world'])

    def blocks_ref(self, gverts=None):
        return R.sq_blocks(*self.P_np, *self.consts, self.Rw_np, self.Tw_np, gverts)

    def ground(self, ngv):
        g = rnd(300 + ngv)
        return [g.randn(ngv, 3).astype(np.float32), g.randn(6).astype(np.float32), g.randn(3).astype(np.float32)]


def run_prologue(sc, lg, noise, noise_scale, thresh, ngv=1, nsets=0, nzero0=0, rng_step=RNG_STEP, with_local=True, sets_np=None, ground_np=None):
    """-> dict of the launch's outputs (Out) and inputs"""
    nb, nv = sc.nb, sc.nv
    o = dict(alpha=Out((nb,)), alpha_full=Out((nb,)), keep=Out((nb,), -7, torch.int32), verts=Out((nb, nv, 3)), local=Out((nb, nv, 9)), ground=Out((ngv, 3)),
             zero0=Out((nzero0 + 1,), ZERO_FILL))          # (one guard word behind the nzero0 floats, then the sentinels)
    ground_np = ground_np or sc.ground(ngv)
    gd = [dev(x) for x in ground_np]
    sets_np = sets_np if sets_np is not None else [texture(s, 60 + k) for k, (_, s) in enumerate(TEX_SHAPES[:nsets])]
    tex, sets = [dev(t) for t in sets_np], []
    for k, t in enumerate(tex):
        d, (n, h, w) = TEX_SHAPES[k]
        o[f'maps{k}'], o[f'sig{k}'] = Out((n, h // d, w // d, 3)), Out((n, h, w, 3))
        sets.append(dict(texture=t.data_ptr(), n=n, h=h, w=w, decim=d, maps=o[f'maps{k}'].ptr, sig=0 if k == 2 else o[f'sig{k}'].ptr))          # (sig may be NULL at decimation 1)
    arr, ns = _lib.texture_sets(sets)
    lgd, nz = dev(lg), dev(noise)
    r, sm, sw = sc.consts
    debug('dbw_debug_step_prologue', ctypes.cast(arr, c_p) if ns else None, ns, lgd.data_ptr(), ptr(nz), noise_scale, thresh, nb, o['alpha'].ptr, o['alpha_full'].ptr,
          o['keep'].ptr, SEED, rng_step, *[p.data_ptr() for p in sc.P], nv, r, sm, sw, sc.Rw.data_ptr(), sc.Tw.data_ptr(), o['verts'].ptr,
          o['local'].ptr if with_local else None, gd[0].data_ptr(), ngv, gd[1].data_ptr(), gd[2].data_ptr(), o['ground'].ptr, o['zero0'].ptr, nzero0, stream())
    torch.cuda.synchronize()
    o.update(_in=dict(lg=lgd, noise=nz, ground=gd, ground_np=ground_np, tex=tex, sets_np=sets_np, sets=sets, keepalive=arr))
    return o


def prologue_twins(sc, o, noise, noise_scale, thresh, ngv):
    """the operator-level kernels on the same inputs (assertion A)"""
    nb, nv, i = sc.nb, sc.nv, o['_in']
    t = dict(alpha=Out((nb,)), alpha_full=Out((nb,)), keep=Out((nb,), -7, torch.int32), verts=Out((nb, nv, 3)), ground=Out((ngv, 3)))
    _lib.call('dbw_block_alpha_fwd', i['lg'].data_ptr(), ptr(noise), noise_scale, thresh, nb, t['alpha'].ptr, t['alpha_full'].ptr, t['keep'].ptr, stream())
    r, sm, sw = sc.consts
    _lib.call('dbw_sq_blocks_fwd', *[p.data_ptr() for p in sc.P], o['keep'].ptr, 0, nb, nv, r, sm, sw, sc.Rw.data_ptr(), sc.Tw.data_ptr(), t['verts'].ptr, stream())
    _lib.call('dbw_posed_mesh_fwd', i['ground'][0].data_ptr(), ngv, i['ground'][1].data_ptr(), i['ground'][2].data_ptr(), sw, sc.Rw.data_ptr(), sc.Tw.data_ptr(),
              t['ground'].ptr, stream())
    sets = []
    for k, s in enumerate(i['sets']):
        t[f'maps{k}'], t[f'sig{k}'] = Out(tuple(o[f'maps{k}'].t.shape)), Out(tuple(o[f'sig{k}'].t.shape))
        sets.append(dict(s, maps=t[f'maps{k}'].ptr, sig=0 if k == 2 else t[f'sig{k}'].ptr))
    if sets:
        arr, ns = _lib.texture_sets(sets)
        _lib.call('dbw_texture_prep_fwd_sets', arr, ns, stream())
    torch.cuda.synchronize()
    return t


def sentinels_intact(o, names):
    return [f'{n}: a sentinel next to the output was overwritten' for n in names
            if not bool((o[n].buf[:64] == o[n].sent).all()) or not bool((o[n].buf[-64:] == o[n].sent).all())]


@pytest.mark.parametrize('nv', NV)
@pytest.mark.parametrize('nb', NB)
def test_prologue_equals_the_operator_kernels_and_float64(nb, nv, record_property):
    sc = Scene(nb, nv)
    ref = sc.blocks_ref()
    F = {f: Figures(f, record_property) for f in ('alpha', 'blocks', 'mesh', 'prep')}
    t = R.torch_sq_blocks(*sc.P, *sc.consts, sc.Rw, sc.Tw, None, F32, DEV)
    F['blocks'].torch(0, t['verts'], ref['verts'], ref['M_verts'], 7)
    philox_alpha = None
    for m, mode in enumerate(MODES):
        name, thresh = mode['name'], mode['thresh']
        ngv, nsets, nzero0 = NGV[m % 2], NSETS[m % 3], NZERO[(m // 2) % 3]
        lg = logits(nb, mode['shift'])
        noise_np, scale = {None: (None, 0.0), 'caller': (R.alpha_logits(nb)[1], NOISE_SCALE), 'philox': (None, NOISE_SCALE),
                           'ignored': (np.full(nb, 1e30, np.float32), 0.0)}[mode['noise']]
        o = run_prologue(sc, lg, noise_np, scale, thresh, ngv, nsets, nzero0)
        names = [k for k in o if k != '_in']
        wrong = sentinels_intact(o, names)
        for k in names:                                     # everything but the kept points of dead blocks is written
            if k not in ('local', 'sig2') and o[k].t.dtype.is_floating_point and bool(torch.isnan(o[k].t).any()):
                wrong.append(f'{k} ({name}): elements left NaN (unwritten)')
        assert not wrong, wrong
        # ---- opacities
        ref_noise = host_noise(SEED, RNG_STEP, nb) if mode['noise'] == 'philox' else (noise_np if mode['noise'] == 'caller' else None)
        ra = R.block_alpha_fwd(lg, ref_noise, scale, thresh)
        keep = o['keep'].np()
        assert np.array_equal(keep != 0, ra['keep']) and set(np.unique(keep)) <= {0, 1}, name
        if mode['shift'] is not None:
            assert np.array_equal(keep, [int(PATTERN[(k + mode['shift']) % 4] in (2.0, 0.3)) for k in range(nb)]), name
        else:
            assert keep.all(), name
        alive = torch.from_numpy(keep != 0).to(DEV)
        F['alpha'].kernel(f'alpha ({name})', 0, o['alpha'].np(), ra['alpha'], ra['M_alpha'])
        F['alpha'].kernel(f'alpha_full ({name})', 0, o['alpha_full'].np(), ra['alpha_full'], ra['M_alpha_full'])
        assert bool((o['alpha_full'].t[~alive] == 0).all()) and bits(o['alpha_full'].t[alive], o['alpha'].t[alive]), name
        ta = R.torch_block_alpha(o['_in']['lg'], dev(ref_noise), scale, thresh, None, None, F32, DEV) if nb > 0 else None
        F['alpha'].torch(0, ta['alpha'], ra['alpha'], ra['M_alpha'])
        # ---- vertices: dead blocks are exactly zero, every vertex; the kept points of a dead block are not written
        got = o['verts'].np()
        live = keep != 0
        assert not got[~live].any(), name
        F['blocks'].kernel(f'verts ({name})', 0, got[live], ref['verts'][live], ref['M_verts'][live], 7)
        sl = o['local'].np().reshape(nb, nv, 3, 3)          # (held to float64 in test_prologue_kept_points_equal_float64; the tail's tests read them)
        assert np.isnan(sl[~live]).all() and not np.isnan(sl[live]).any(), name
        # ---- ground, textures, the cleared floats and the guard word behind them
        gr = R.posed_mesh(*o['_in']['ground_np'], sc.consts[2], sc.Rw_np, sc.Tw_np)
        F['mesh'].kernel(f'ground ({name})', 0, o['ground'].np(), gr['verts'], gr['M_verts'], 7)
        tg = R.torch_posed_mesh(*o['_in']['ground'], sc.consts[2], sc.Rw, sc.Tw, None, F32, DEV)
        F['mesh'].torch(0, tg['verts'], gr['verts'], gr['M_verts'], 7)
        for k, tex_np in enumerate(o['_in']['sets_np']):
            d = TEX_SHAPES[k][0]
            fr = R.texture_prep_fwd(tex_np, d)
            F['prep'].kernel(f'maps{k} ({name})', 0, o[f'maps{k}'].np(), fr['maps'], fr['M_maps'], d * d)
            tt = R.torch_texture_prep(o['_in']['tex'][k], d, torch.zeros_like(o[f'maps{k}'].t), None, F32, DEV)
            F['prep'].torch(0, tt['maps'], fr['maps'], fr['M_maps'], d * d)
            F['prep'].torch(0, tt['sig'], fr['sig'], fr['M_sig'])
            if k == 2:
                assert bool(torch.isnan(o['sig2'].t).all())          # sig = NULL at decimation 1: not written
            else:
                F['prep'].kernel(f'sig{k} ({name})', 0, o[f'sig{k}'].np(), fr['sig'], fr['M_sig'])
        z = o['zero0'].np()
        assert not z[:nzero0].any() and z[nzero0] == np.float32(ZERO_FILL), (name, nzero0)
        # ---- A: the operator-level kernels on the same inputs, bit for bit
        tw = prologue_twins(sc, o, None if mode['noise'] in ('philox', 'ignored') else o['_in']['noise'], scale, thresh, ngv)
        for k in names:
            if k in ('local', 'zero0') or (k == 'sig2'):
                continue
            if mode['noise'] == 'philox' and k in ('alpha', 'alpha_full'):          # (the twin has no generator: keep and the vertices only)
                continue
            assert bits(o[k], tw[k]), (name, k)
        # ---- the kept points are optional: the same vertices without them
        if m in (1, 3):
            o2 = run_prologue(sc, lg, noise_np, scale, thresh, ngv, nsets, nzero0, with_local=False)
            assert bits(o2['verts'], o['verts']) and bits(o2['alpha'], o['alpha']) and bool(torch.isnan(o2['local'].t).all()), name
        if mode['noise'] == 'philox':
            philox_alpha = o['alpha']
            again = run_prologue(sc, lg, None, scale, thresh, ngv, nsets, nzero0)
            other = run_prologue(sc, lg, None, scale, thresh, ngv, nsets, nzero0, rng_step=RNG_STEP + 1)
            assert bits(again['alpha'], o['alpha']) and not bits(other['alpha'], o['alpha'])
            assert not np.array_equal(host_noise(SEED, RNG_STEP + 1, nb), ref_noise)
            ro = R.block_alpha_fwd(lg, host_noise(SEED, RNG_STEP + 1, nb), scale, thresh)
            F['alpha'].kernel('alpha (philox, next step)', 0, other['alpha'].np(), ro['alpha'], ro['M_alpha'])
        if mode['noise'] == 'ignored':                      # noise_scale == 0: the buffer is not read -- the bits of the launch without one
            plain = run_prologue(sc, lg, None, 0.0, thresh, ngv, nsets, nzero0)
            assert bits(plain['alpha'], o['alpha']) and bits(plain['alpha_full'], o['alpha_full'])
    assert philox_alpha is not None
    for f, fig in F.items():
        fig.done(f'prologue {f} nb{nb}-nv{nv}')


@pytest.mark.parametrize('nv', NV)
@pytest.mark.parametrize('nb', NB)
def test_prologue_kept_points_equal_float64(nb, nv, record_property):
    """sq_local of every live block -- the block-frame point, d / d eps1, d / d eps2 -- element-wise against float64 from the float32
    sq_eps, on the superquadric family's VALUE bar (1.39e-06), M = the element's own absolute value (it is one product).

    This test found the one inaccuracy of the family.  With the exponent eps = 1.8 sigmoid(sq_eps) + 0.1 evaluated in float32 (expf,
    division, product, sum: 1.7e-07 to 2e-07 from its float64 value) three of the 21 cases missed the bar, kernel and torch float32
    alike to three digits: nb1-nv256 1.65e-06, nb64-nv255 1.54e-06, nb64-nv256 1.60e-06 -- |t|^eps turns an error of the exponent into
    |log |t|| as much, and the trig tables of these cases hold cosines down to 7e-05, 5e-06 and 2e-05.  Float64 powers of the
    float32-computed exponent alone read 1.62e-06, 1.51e-06 and 1.46e-06 on the same cases: all of the error was the exponent's, none
    the powf's.  csrc/model_math.h now does the arithmetic behind the expf in double and rounds the exponent once (sq_exponent); torch's
    float32 column keeps showing what the float32 exponent costs."""
    sc = Scene(nb, nv)
    loc = R.sq_local(sc.P_np[0], sc.P_np[4], sc.consts[0])
    F = Figures('blocks', record_property)
    tl = R.torch_sq_local(sc.P[0], sc.P[4], sc.consts[0], F32, DEV)
    for key in ('loc', 'de1', 'de2'):
        F.torch(0, tl[key], loc[key], loc['M_' + key], 3)
    for shift in (None, 0, 1):
        o = run_prologue(sc, logits(nb, shift), None, 0.0, -1.0 if shift is None else 0.5)
        live = o['keep'].np() != 0
        sl = o['local'].np().reshape(nb, nv, 3, 3)
        assert not sentinels_intact(o, ['local']) and np.isnan(sl[~live]).all() and not np.isnan(sl[live]).any()
        for j, key in enumerate(('loc', 'de1', 'de2')):
            F.kernel(f'sq_local {key} (shift {shift})', 0, sl[live][:, :, j], loc[key][live], loc['M_' + key][live], 3)
        assert not sl[live][:, :, 2, 1].any()          # d y / d eps2 is exactly 0
    F.done(f'prologue sq_local nb{nb}-nv{nv}')


def test_prologue_refuses_more_than_64_blocks_and_a_decimation_that_does_not_divide_the_map():
    """host-side checks: nothing is launched, nothing is written"""
    sc = Scene(3, 5)
    lg = dev(logits(3, 0))
    o = dict(alpha=Out((3,)), alpha_full=Out((3,)), keep=Out((3,), -7, torch.int32), verts=Out((3, 5, 3)), local=Out((3, 5, 9)), ground=Out((1, 3)), zero0=Out((4,), ZERO_FILL))
    gd = [dev(x) for x in sc.ground(1)]
    tex = dev(texture((1, 8, 8), 0))
    maps, sig = Out((1, 2, 2, 3)), Out((1, 8, 8, 3))
    r, sm, sw = sc.consts

    def call(nb, sets):
        arr, ns = _lib.texture_sets(sets)
        rc, lib = debug_rc('dbw_debug_step_prologue', ctypes.cast(arr, c_p) if ns else None, ns, lg.data_ptr(), None, 0.0, 0.5, nb, o['alpha'].ptr, o['alpha_full'].ptr,
                           o['keep'].ptr, SEED, RNG_STEP, *[p.data_ptr() for p in sc.P], 5, r, sm, sw, sc.Rw.data_ptr(), sc.Tw.data_ptr(), o['verts'].ptr, o['local'].ptr,
                           gd[0].data_ptr(), 1, gd[1].data_ptr(), gd[2].data_ptr(), o['ground'].ptr, o['zero0'].ptr, 3, stream())
        return rc, lib.dbw_last_error().decode()
    rc, text = call(65, [])
    assert rc != 0 and 'bad size' in text, (rc, text)
    rc, text = call(3, [dict(texture=tex.data_ptr(), n=1, h=8, w=8, decim=3, maps=maps.ptr, sig=sig.ptr)])
    assert rc != 0 and 'bad texture set' in text, (rc, text)
    torch.cuda.synchronize()
    for k in ('alpha', 'alpha_full', 'verts', 'local', 'ground'):
        assert bool(torch.isnan(o[k].t).all()), k
    assert bool((o['zero0'].t == ZERO_FILL).all()) and bool((o['keep'].t == -7).all()) and bool(torch.isnan(maps.t).all()) and bool(torch.isnan(sig.t).all())


# ==== blocks_tail_kernel ================================================================================================================
# (parts, g_alpha_parts given, g_alpha_full given, keep given)
TAIL_VARIANTS = [(1, True, True, True), (2, True, True, True), (49, True, True, True), (1, False, True, True), (2, True, False, True), (2, True, True, False)]
PLANTED = 1e6          # in g_alpha_full of a dead block: must not enter its g_logit


def run_tail(sc, o, keep, gv, start, ga, parts, gf, raised=None):
    nb, nv = sc.nb, sc.nv
    g = {k: filled(start[k]) for k in BLOCK_GRADS}
    gl = Out((nb,))
    flag = None if raised is None else Out((1,))
    rs = None if raised is None else torch.full((1,), raised, device=DEV)
    _, sm, sw = sc.consts
    debug('dbw_debug_blocks_tail', *[p.data_ptr() for p in sc.P[:4]], o['local'].ptr, ptr(keep), nb, nv, sm, sw, sc.Rw.data_ptr(), gv.data_ptr(), g['g_sq_eps'].ptr, g['g_S'].ptr,
          g['g_R6'].ptr, g['g_T'].ptr, o['alpha'].ptr, ptr(ga), ptr(gf), parts, gl.ptr, ptr(rs), None if flag is None else flag.ptr, stream())
    torch.cuda.synchronize()
    return g, gl, flag


def tail_twins(sc, o, keep, gv, start, ga, parts, gf):
    nb, nv = sc.nb, sc.nv
    g = {k: filled(start[k]) for k in BLOCK_GRADS}
    gl = Out((nb,))
    r, sm, sw = sc.consts
    _lib.call('dbw_sq_blocks_bwd', *[p.data_ptr() for p in sc.P], ptr(keep), 0, nb, nv, r, sm, sw, sc.Rw.data_ptr(), gv.data_ptr(), g['g_sq_eps'].ptr, g['g_S'].ptr,
              g['g_R6'].ptr, g['g_T'].ptr, stream())
    _lib.call('dbw_block_alpha_bwd', o['alpha'].ptr, ptr(keep), ptr(ga), parts, ptr(gf), nb, gl.ptr, stream())
    torch.cuda.synchronize()
    return g, gl


@pytest.mark.parametrize('nv', NV)
@pytest.mark.parametrize('nb', NB)
def test_blocks_tail_equals_the_operator_kernels_and_float64(nb, nv, record_property):
    sc = Scene(nb, nv)
    g_ = rnd(11 + nb + nv)
    gv_np = g_.randn(nb, nv, 3).astype(np.float32)
    gv = dev(gv_np)
    ref = sc.blocks_ref(gv_np)
    FB, FA = Figures('blocks', record_property), Figures('alpha', record_property)
    t = R.torch_sq_blocks(*sc.P, *sc.consts, sc.Rw, sc.Tw, gv, F32, DEV)
    for key in BLOCK_GRADS:
        FB.torch(1, t[key], ref[key], ref['M_' + key], nv * 9)
    # the prologue of the same step: its kept points (sq_local), its opacities and its mask are what the tail reads
    pro = {shift: run_prologue(sc, logits(nb, shift), None, 0.0, 0.5 if shift is not None else -1.0) for shift in (0, 1, None)}
    for shift, o in pro.items():
        keep_np = o['keep'].np()
        live = keep_np != 0
        lg = o['_in']['lg']
        for v, (parts, with_parts, with_full, with_keep) in enumerate(TAIL_VARIANTS):
            if (shift is None) != (not with_keep):          # keep = NULL: every block is alive, so every block's points must have been kept
                continue
            ga_np, gf_np = g_.randn(nb, parts).astype(np.float32), g_.randn(nb).astype(np.float32)
            gf_np[~live] = PLANTED
            ga, gf = (dev(ga_np) if with_parts else None), (dev(gf_np) if with_full else None)
            keep = o['keep'].t if with_keep else None
            bref = R.block_alpha_bwd(o['alpha'].np(), keep_np if with_keep else None, ga_np if with_parts else None, gf_np if with_full else None)
            if with_parts and with_full:
                ta = R.torch_block_alpha(lg, None, 0.0, 0.5 if with_keep else -1.0, ga, gf, F32, DEV)
                FA.torch(1, ta['g_logit'], bref['g_logit'], bref['M_g_logit'], parts + 1)
            for which in (0, 1):
                name = f'shift {shift} parts {parts} {with_parts}/{with_full}/{with_keep} start {which}'
                start = {key: starts(ref['M_' + key])[which] for key in BLOCK_GRADS}
                if which == 1:
                    for key in BLOCK_GRADS:
                        start[key][~live] = 0.75          # a dead block's gradients keep exactly what they held
                g, gl, flag = run_tail(sc, o, keep, gv, start, ga, parts, gf, raised=0.0 if v == 0 else None)
                wrong = gl.wrong('g_logit') + sum((g[key].wrong(key) for key in BLOCK_GRADS), [])
                assert not wrong, (name, wrong)
                # B, element-wise: every block's every entry on its own magnitude
                for key in BLOCK_GRADS:
                    got = g[key].np()
                    FB.kernel(f'{key} ({name})', 1, got[live], ref[key][live], ref['M_' + key][live], nv * 9, start=start[key][live])
                    assert np.array_equal(got[~live], start[key][~live]), (name, key)
                # (a dead block: the reference and its M hold the parts' sum only, so the 1e6 planted in its g_alpha_full is an error of ~1e6 / M if it enters)
                FA.kernel(f'g_logit ({name})', 1, gl.np(), bref['g_logit'], bref['M_g_logit'], parts + 1)
                if not with_parts and with_keep:
                    assert not gl.np()[~live].any(), name          # no parts: a dead block's g_logit is exactly 0
                # A: sq_blocks_bwd + block_alpha_bwd on the same inputs from the same start values
                tg, tgl = tail_twins(sc, o, keep, gv, start, ga, parts, gf)
                for key in BLOCK_GRADS:
                    assert bits(g[key], tg[key]), (name, key)
                assert bits(gl, tgl), name
                # the latch: void_flag = void_raised, whatever it is; the tail itself does not gate on it (Adam does)
                if v == 0:
                    assert float(flag.t) == 0.0 and not flag.wrong('void_flag')
                    g1, gl1, flag1 = run_tail(sc, o, keep, gv, start, ga, parts, gf, raised=1.0)
                    assert float(flag1.t) == 1.0 and not flag1.wrong('void_flag')
                    assert bits(gl1, gl) and all(bits(g1[key], g[key]) for key in BLOCK_GRADS), name
    FB.done(f'tail blocks nb{nb}-nv{nv}')
    FA.done(f'tail alpha nb{nb}-nv{nv}')


# ==== regularisers_kernel ===============================================================================================================
REG_KEYS = R.OVERLAP_GRADS          # g_sq_eps, g_S, g_R6, g_T, g_alpha
PARS_SCALE = 0.01
# Assertion A of the overlap term holds up to this many sample points.  Every point adds its share of each block's 18 raw gradients into
# LDS with float32 atomics (overlap_block: atomicAdd(g + ...)), the four waves of a workgroup in the order they arrive: with more than
# one wave at work two launches of the SAME kernel on the same inputs differ in the last bits (measured here: dbw_overlap_loss against
# itself, and the fused launch against itself, at 256 points), so there is no order for the fused kernel to share with the operator.
ONE_WAVE = 64


def bitwise_keys(P, overlap):
    """What assertion A compares.  Everything where one wave does the overlap term's adding (ONE_WAVE) or the term is off.  Beyond, what has
    one order still: the parsimony value (one wave's fixed-order sum) at any size, and the overlap value while the launch has one
    workgroup -- a sample's share comes from its first pass alone, then wave_sum, the fixed sum of the four waves' parts and ONE atomic by
    thread 0: no LDS atomics in it.  (With more workgroups their atomics meet in `loss` in arrival order.)"""
    if P <= ONE_WAVE or not overlap:
        return REG_KEYS + ('value', 'pars', 'ws')
    return ('value', 'pars') if P <= 256 else ('pars',)


def reg_outputs(c, start):
    """loss_overlap, loss_parsimony, the five gradients (g_alpha = g_alpha_full), the workspace"""
    o = {k: filled(start[k]) for k in REG_KEYS + ('value', 'pars')}
    o['ws'] = Out((c['Kb'] * 18,), 0.0)
    return o


def run_regularisers(c, d, o, ticket, overlap, pars, u='given', rng=(0, 0)):
    inv_temp = float(np.float32(1.0) / np.float32(c['temperature']))          # (what the step passes: 1.f / overlap_temperature)
    rc, lib = debug_rc('dbw_debug_regularisers', ptr(d['u']) if u == 'given' else ptr(u), c['npts'], rng[0], rng[1], d['sq_eps'].data_ptr(), d['S'].data_ptr(), d['R6'].data_ptr(),
                       d['T'].data_ptr(), d['alpha'].data_ptr(), c['Kb'], c['ratio'], c['scale_min'], inv_temp, c['thresh'], c['scale'] if overlap else 0.0, R.PARSIMONY_EPS,
                       PARS_SCALE if pars else 0.0, o['pars'].ptr, o['value'].ptr, *[o[k].ptr for k in REG_KEYS], o['ws'].ptr, ticket.ptr, stream())
    assert rc == 0, lib.dbw_last_error().decode()
    torch.cuda.synchronize()
    return o['ws'].wrong('workspace') + ticket.wrong('ticket') + sum((o[k].wrong(k) for k in REG_KEYS + ('value', 'pars')), [])


def reg_twins(c, d, o, overlap, pars):
    if overlap:
        _lib.call('dbw_overlap_loss', d['u'].data_ptr(), c['npts'], d['sq_eps'].data_ptr(), d['S'].data_ptr(), d['R6'].data_ptr(), d['T'].data_ptr(), d['alpha'].data_ptr(), c['Kb'],
                  c['ratio'], c['scale_min'], c['temperature'], c['thresh'], c['scale'], o['value'].ptr, *[o[k].ptr for k in REG_KEYS], o['ws'].ptr, stream())
    if pars:
        _lib.call('dbw_sqrt_mean', d['alpha'].data_ptr(), c['Kb'], R.PARSIMONY_EPS, PARS_SCALE, o['pars'].ptr, o['g_alpha'].ptr, stream())
    torch.cuda.synchronize()


def reg_reference(c, ref, overlap, pars):
    """the launch's float64 reference: the overlap term and / or the parsimony term, both adding into g_alpha"""
    Kb = c['Kb']
    out = {k: (ref[k] if overlap else np.zeros_like(ref[k])) for k in REG_KEYS + ('value',)}
    out.update({'M_' + k: (ref['M_' + k] if overlap else np.zeros_like(R.f64(ref['M_' + k]))) for k in REG_KEYS + ('value',)})
    ps = R.sqrt_mean(c['alpha'], R.PARSIMONY_EPS, PARS_SCALE)
    out['pars'], out['M_pars'] = (ps['value'], ps['M_value']) if pars else (0.0, 0.0)
    if pars:
        out['g_alpha'], out['M_g_alpha'] = out['g_alpha'] + ps['grad'], out['M_g_alpha'] + ps['M_grad']
    return out, ps


def check_regularisers(F, FP, name, c, o, exp, start, G, overlap, pars, ref):
    """ref: the overlap term's own reference (exp: with the parsimony term in g_alpha)"""
    P = c['Kb'] * c['npts']
    if overlap:
        F.kernel(f'loss_overlap ({name})', 0, o['value'].np()[0], exp['value'], exp['M_value'], P, G=G, start=start['value'])
        for k in REG_KEYS:
            F.kernel(f'{k} ({name})', 1, o[k].np(), exp[k], exp['M_' + k], P * 9, start=start[k])
        # the workspace is left holding the raw accumulators (from zero): of a block's 18, the sums for T (14..16) and the opacity's share
        # (17) are the overlap term's g_T and g_alpha as they stand (finish_pose_grads adds them unchanged)
        ws = o['ws'].np().reshape(c['Kb'], 18)
        F.kernel(f'ws[:, 14:17] ({name})', 1, ws[:, 14:17], ref['g_T'], ref['M_g_T'], P * 9)
        F.kernel(f'ws[:, 17] ({name})', 1, ws[:, 17], ref['g_alpha'], ref['M_g_alpha'], P * 9)
    else:
        for k in REG_KEYS[:4] + ('value',):
            assert np.array_equal(o[k].np().reshape(-1), np.asarray(start[k]).reshape(-1)), (name, k)
        FP.kernel(f'g_alpha_full ({name})', 1, o['g_alpha'].np(), exp['g_alpha'], exp['M_g_alpha'], 2, start=start['g_alpha'])
    if pars:
        FP.kernel(f'loss_parsimony ({name})', 0, o['pars'].np()[0], exp['pars'], exp['M_pars'], c['Kb'], start=start['pars'])
    else:
        assert np.array_equal(o['pars'].np(), np.asarray(start['pars']).reshape(1)), name


@pytest.mark.parametrize('name', list(R.STEP_OVERLAP_CASES))
def test_regularisers_equal_the_operator_kernels_and_float64(name, record_property):
    c = R.overlap_case(name)
    ref = R.overlap_ref(c)
    assert R.well_conditioned(ref['cond']), ref['cond']          # (tests/test_model_kernels_ref_host.py asserts the same without a GPU)
    Kb, npts = c['Kb'], c['npts']
    P = Kb * npts
    G = math.ceil(P / 256)
    d = {k: dev(c[k]) for k in ('u', 'sq_eps', 'S', 'R6', 'T', 'alpha')}
    F, FP = Figures('overlap', record_property), Figures('parsimony', record_property)
    t = R.torch_overlap(d['u'], d['sq_eps'], d['S'], d['R6'], d['T'], d['alpha'], c['ratio'], c['scale_min'], c['temperature'], c['thresh'], c['scale'], F32, DEV)
    F.torch(0, t['value'], ref['value'], ref['M_value'], P)
    for k in REG_KEYS:
        F.torch(1, t[k], ref[k], ref['M_' + k], P * 9)
    ticket = Out((1,), 0, torch.int32)          # ONE ticket for every launch of this test, back to back: it must come back to 0 each time
    for overlap, pars in ((True, False), (False, True), (True, True), (True, True)):
        exp, ps = reg_reference(c, ref, overlap, pars)
        tp = R.torch_sqrt_mean(d['alpha'], R.PARSIMONY_EPS, PARS_SCALE, F32, DEV)
        off = c['alpha'] != np.float32(R.PARSIMONY_EPS)
        FP.torch(0, tp['value'], ps['value'], ps['M_value'], Kb)
        FP.torch(1, tp['grad'][off], ps['grad'][off], ps['M_grad'][off], 2)
        for which in (0, 1):
            start = {k: starts(exp['M_' + k])[which] for k in REG_KEYS + ('value', 'pars')}
            o = reg_outputs(c, start)
            wrong = run_regularisers(c, d, o, ticket, overlap, pars)
            label = f'overlap {overlap} parsimony {pars} start {which}'
            assert not wrong, (label, wrong)
            assert int(ticket.t) == 0, label
            check_regularisers(F, FP, label, c, o, exp, start, G, overlap, pars, ref)
            if pars:          # at or below the clamp: no contribution from the parsimony term (index 1: an exact 0 when Kb >= 3)
                below = c['alpha'] <= np.float32(R.PARSIMONY_EPS)
                assert not ps['grad'][below].any()
            # A: dbw_overlap_loss, then dbw_sqrt_mean into the same g_alpha_full
            tw = reg_outputs(c, start)
            reg_twins(c, d, tw, overlap, pars)
            for k in bitwise_keys(P, overlap):
                assert bits(o[k], tw[k]), (label, k)
    record_property('G', G)
    F.done(f'regularisers {name} G={G}', G=G)
    FP.done(f'regularisers parsimony {name}')


@pytest.mark.parametrize('name', list(R.STEP_BITWISE_CASES))
def test_regularisers_finish_of_64_blocks_equals_the_operator_kernels_bit_for_bit(name, record_property):
    """64 blocks x 1 sample: one wave, one order of the LDS atomics -- so the fused finish (load_pose + finish_pose_grads +
    g_alpha_full += ws[17] on `tid < nb` of 256 threads, then the parsimony term into the same g_alpha_full) is compared with
    overlap_finish_kernel + sqrt_mean_kernel for every block: dead ones (opacity 0), the opacity at the parsimony clamp and the one a
    float32 step above it.  The values are held to float64 as well; the gradients are not (model_kernels_ref.STEP_BITWISE_CASES: with one
    sample per block float32 itself is above the floor on the host, whatever the seed) -- their float64 judge is the other cases."""
    c = R.overlap_case(name)
    ref = R.overlap_ref(c)
    assert R.well_conditioned(ref['cond']) and c['Kb'] * c['npts'] <= ONE_WAVE, ref['cond']
    assert c['alpha'][1] == 0 and c['alpha'][2] == np.float32(R.PARSIMONY_EPS) and c['alpha'][3] > np.float32(R.PARSIMONY_EPS)
    d = {k: dev(c[k]) for k in ('u', 'sq_eps', 'S', 'R6', 'T', 'alpha')}
    F, FP = Figures('overlap', record_property), Figures('parsimony', record_property)
    ticket = Out((1,), 0, torch.int32)
    for overlap, pars in ((True, False), (True, True)):
        exp, ps = reg_reference(c, ref, overlap, pars)
        for which in (0, 1):
            start = {k: starts(exp['M_' + k])[which] for k in REG_KEYS + ('value', 'pars')}
            o, tw = reg_outputs(c, start), reg_outputs(c, start)
            label = f'overlap {overlap} parsimony {pars} start {which}'
            assert not run_regularisers(c, d, o, ticket, overlap, pars) and int(ticket.t) == 0, label
            reg_twins(c, d, tw, overlap, pars)
            for k in REG_KEYS + ('value', 'pars', 'ws'):
                assert bits(o[k], tw[k]), (label, k)
            assert bool(o['ws'].t.any()) and not np.array_equal(o['g_S'].np(), start['g_S'])          # not a comparison of nothing
            F.kernel(f'loss_overlap ({label})', 0, o['value'].np()[0], exp['value'], exp['M_value'], c['Kb'] * c['npts'], start=start['value'])
            if pars:
                FP.kernel(f'loss_parsimony ({label})', 0, o['pars'].np()[0], exp['pars'], exp['M_pars'], c['Kb'], start=start['pars'])
    F.done(f'regularisers bitwise {name}')
    FP.done(f'regularisers bitwise parsimony {name}')


PHILOX_STEP = {'kb2-32': 0, 'kb4-64': 0, 'kb64-40': 0}          # the step counter the search below ends on, per case (seed 227391)


@pytest.mark.parametrize('name', list(PHILOX_STEP))
def test_regularisers_draw_their_samples_from_the_counter_based_generator(name, record_property):
    """u = NULL: the samples are uniforms of (seed, rng_step, stream 1, index = the point) -- the host build of the same generator draws
    them, a second launch reads them through `u`; both are held to the float64 reference on those samples, and with one wave at work
    (ONE_WAVE) they are bit-equal.  The step counter is the first whose draws keep the margins of the fixed cases: no sample near a branch
    of the reference, and torch's float32 on the CPU within half the gradient floor (conditions on the reference and the yardstick, no
    kernel in them; with 64 samples most draws do not keep the second: model_kernels_ref.overlap_float32_cost)."""
    c = R.overlap_case(name)
    Kb, npts = c['Kb'], c['npts']
    P = Kb * npts
    G = math.ceil(P / 256)
    for step in range(64):
        c['u'] = host_uniform(SEED, step, P).reshape(Kb, npts, 3)
        ref = R.overlap_ref(c)
        if (R.well_conditioned(ref['cond']) and ref['cond']['active'] > 10
                and R.overlap_float32_cost(c, ref) < R.FLOAT32_COST_MARGIN * R.FLOOR['overlap'][1]):          # (the conditions of the fixed cases: model_kernels_ref.py)
            break
    else:
        raise AssertionError('no step counter below 64 whose draws keep the margins')
    assert step == PHILOX_STEP[name]          # (a host-side search with a fixed outcome: written down, so that nobody has to run it to know)
    assert float(c['u'].min()) >= 0 and float(c['u'].max()) < 1
    d = {k: dev(c[k]) for k in ('u', 'sq_eps', 'S', 'R6', 'T', 'alpha')}
    F, FP = Figures('overlap', record_property), Figures('parsimony', record_property)
    t = R.torch_overlap(d['u'], d['sq_eps'], d['S'], d['R6'], d['T'], d['alpha'], c['ratio'], c['scale_min'], c['temperature'], c['thresh'], c['scale'], F32, DEV)
    F.torch(0, t['value'], ref['value'], ref['M_value'], P)
    for k in REG_KEYS:
        F.torch(1, t[k], ref[k], ref['M_' + k], P * 9)
    exp, _ = reg_reference(c, ref, True, True)
    ticket = Out((1,), 0, torch.int32)
    start = {k: starts(exp['M_' + k])[1] for k in REG_KEYS + ('value', 'pars')}
    outs = []
    for u in (None, 'given'):
        o = reg_outputs(c, start)
        wrong = run_regularisers(c, d, o, ticket, True, True, u=u, rng=(SEED, step))
        assert not wrong and int(ticket.t) == 0, (u, wrong)
        check_regularisers(F, FP, f'u {u}', c, o, exp, start, G, True, True, ref)
        outs.append(o)
    for k in bitwise_keys(P, True):
        assert bits(outs[0][k], outs[1][k]), k
    other = reg_outputs(c, start)
    assert not run_regularisers(c, d, other, ticket, True, True, u=None, rng=(SEED, step + 1))
    assert not bits(other['value'], outs[0]['value'])          # another step, other samples
    F.done(f'regularisers philox {name} step {step} G={G}', G=G)
    FP.done(f'regularisers philox parsimony {name}')


def pars_alpha(nb):
    """opacities with dead blocks (0), one exactly at the clamp and one a float32 step above it"""
    x = (rnd(80 + nb).rand(nb) * 0.98 + 0.01).astype(np.float32)
    if nb >= 5:
        x[0], x[1], x[2], x[4] = 0.0, np.float32(R.PARSIMONY_EPS), np.nextafter(np.float32(R.PARSIMONY_EPS), np.float32(1)), 0.0
    return x


@pytest.mark.parametrize('nb', [1, 5, 64])
def test_regularisers_parsimony_alone_needs_no_overlap_argument(nb, record_property):
    """overlap_scale = 0: a grid of one workgroup; u, the overlap's outputs, its workspace and the blocks' parameters may be NULL"""
    x_np = pars_alpha(nb)
    ps = R.sqrt_mean(x_np, R.PARSIMONY_EPS, PARS_SCALE)
    x = dev(x_np)
    FP = Figures('parsimony', record_property)
    tp = R.torch_sqrt_mean(x, R.PARSIMONY_EPS, PARS_SCALE, F32, DEV)
    off = x_np != np.float32(R.PARSIMONY_EPS)
    FP.torch(0, tp['value'], ps['value'], ps['M_value'], nb)
    FP.torch(1, tp['grad'][off], ps['grad'][off], ps['M_grad'][off], 2)
    below = x_np <= np.float32(R.PARSIMONY_EPS)
    ticket = Out((1,), 0, torch.int32)
    for which in (0, 1):
        ls, gs = starts(ps['M_value'])[which], starts(ps['M_grad'])[which]
        gs[below] = 0.75
        loss, grad = filled(ls), filled(gs)
        debug('dbw_debug_regularisers', None, 0, 0, 0, None, None, None, None, x.data_ptr(), nb, 0.5, 0.2, 1.0, 0.0, 0.0, R.PARSIMONY_EPS, PARS_SCALE, loss.ptr, None, None, None, None,
              None, grad.ptr, None, ticket.ptr, stream())
        torch.cuda.synchronize()
        assert not loss.wrong('loss') + grad.wrong('grad') + ticket.wrong('ticket') and int(ticket.t) == 0
        FP.kernel(f'loss (start {which})', 0, loss.np()[0], ps['value'], ps['M_value'], nb, start=ls)
        FP.kernel(f'grad (start {which})', 1, grad.np(), ps['grad'], ps['M_grad'], 2, start=gs)
        assert np.array_equal(grad.np()[below], gs[below])          # at or below the clamp (0, and the value equal to it): nothing is added
        if nb >= 5:
            assert below[:2].all() and not below[2] and grad.np()[2] != gs[2]          # a float32 step above the clamp: the gradient is there
        loss2, grad2 = filled(ls), filled(gs)
        _lib.call('dbw_sqrt_mean', x.data_ptr(), nb, R.PARSIMONY_EPS, PARS_SCALE, loss2.ptr, grad2.ptr, stream())
        torch.cuda.synchronize()
        assert bits(loss, loss2) and bits(grad, grad2)
    FP.done(f'regularisers parsimony-only nb{nb}')


def test_regularisers_add_nothing_where_the_occupancy_sum_equals_the_threshold_exactly():
    """every block dead (alpha_full = 0) and a threshold of 0: every sample's sum is exactly 0 = the threshold, `sum - thresh > 0` is
    false (the reference's clamp(0) has no gradient there either, dbw.py:398), so neither the loss nor any gradient moves -- planted, like
    the logit 0 of the opacity mask: the one place where `>` and `>=` differ"""
    c = dict(R.overlap_case('kb4-64'), thresh=0.0)
    c['alpha'] = np.zeros(4, np.float32)
    ref = R.overlap_ref(c)
    assert ref['value'] == 0 and ref['cond']['active'] == 0 and ref['cond']['sum'] == 0
    d = {k: dev(c[k]) for k in ('u', 'sq_eps', 'S', 'R6', 'T', 'alpha')}
    start = {k: np.full(np.shape(ref[k]) or (1,), 0.75, np.float32) for k in REG_KEYS + ('value',)}
    start['pars'] = np.float32(0.75)
    ticket = Out((1,), 0, torch.int32)
    for u, rng in (('given', (0, 0)), (None, (SEED, RNG_STEP))):
        o = reg_outputs(c, start)
        assert not run_regularisers(c, d, o, ticket, True, False, u=u, rng=rng) and int(ticket.t) == 0
        for k in REG_KEYS + ('value', 'pars'):
            assert bool((o[k].t == 0.75).all()), (u, k)
        assert not bool(o['ws'].t.any()), u


def test_regularisers_with_both_terms_off_launch_nothing():
    c = R.overlap_case('kb4-64')
    d = {k: dev(c[k]) for k in ('u', 'sq_eps', 'S', 'R6', 'T', 'alpha')}
    start = {k: np.full(np.shape(R.overlap_ref(c)[k]) or (1,), 0.75, np.float32) for k in REG_KEYS + ('value',)}
    start['pars'] = np.float32(0.75)
    o = reg_outputs(c, start)
    o['ws'].t.fill_(0.5)
    ticket = Out((1,), 7, torch.int32)          # (a marker, not a ticket: the launcher returns on the host before any launch, so nothing ever counts on it)
    assert not run_regularisers(c, d, o, ticket, False, False)
    assert int(ticket.t) == 7 and bool((o['ws'].t == 0.5).all())
    for k in REG_KEYS + ('value', 'pars'):
        assert bool((o[k].t == 0.75).all()), k


# ==== loss_finish_kernel ================================================================================================================
LOSS_BLOCKS = 32                                   # csrc/train_step.hip: the grid of loss_finish_kernel
NPARTS = [0, 1, 255, 256, 257, 8192, 8193, 100003]          # 8192 = 32 workgroups x 256: every thread one element; 8193: one thread a second one
SENTINEL5 = -777.25


@pytest.mark.parametrize('vals123,tvs,want', [((2.0 ** 24, 2.0, 1.0), 0.5, 2.0 ** 24), ((1.0, 2.0 ** 25, -2.0 ** 24), 0.5, 2.0)],
                         ids=['absorbed-one-by-one', 'cancelled-last'])
def test_loss_finish_adds_the_total_in_one_fixed_order(vals123, tvs, want):
    """out5[4] = ((rgb + parsimony) + tv) + overlap in float32, in that order -- on values where every other grouping gives another
    float32: rgb = 1 exactly (one partial of 1, scale 1).  ((1 + 2^24) + 1) + 1 = 2^24 (each 1 is half an ulp of 2^24 and ties go to
    even) where (1 + 2^24) + (1 + 1) and (1 + 1) + (2^24 + 1) are 2^24 + 2; ((1 + 1) + 2^24) - 2^24 = 2 where 1 + ((1 + 2^24) - 2^24) is 1.
    (Random loss values do not tell groupings apart: on the values of test_loss_finish_equals_float64... a total grouped as
    (rgb + parsimony) + (tv + overlap) had the same float32 in every case.)"""
    vals_np = np.array([0, vals123[0], vals123[1], vals123[2], 0, 0, 0, 0], np.float32)
    part, vals, out5 = dev(np.ones(1, np.float32)), Out((8,), torch.from_numpy(vals_np)), Out((5,), SENTINEL5)
    debug('dbw_debug_loss_finish', part.data_ptr(), 1, 1.0, tvs, vals.ptr, out5.ptr, stream())
    torch.cuda.synchronize()
    assert not vals.wrong('vals') + out5.wrong('out5')
    got, f = out5.np(), np.float32
    assert got[0] == 1.0 and got[2] == f(vals123[1]) * f(tvs)
    assert got[4] == ((f(got[0]) + f(got[1])) + f(got[2])) + f(got[3]) == f(want)


@pytest.mark.parametrize('zeros', [False, True], ids=['random', 'all-zero'])
@pytest.mark.parametrize('nparts', NPARTS)
def test_loss_finish_equals_float64_and_leaves_its_state_to_the_arena_clear(nparts, zeros, record_property):
    """The five loss values.  State: the kernel adds into vals[0] and counts its workgroups in vals[5] and resets neither -- the step
    relies on the zero arena for both: `vals` lies inside it (csrc/train_step.hip, compute_layout: `L.arena_begin = o; ... L.vals = o;`),
    the arena is cleared by the run's own Adam launch (`the zero arena: cleared by the plan's own Adam launch at the end of a run; before
    the first run ... by a fill`, the hipMemsetAsync of arena_begin .. arena_end at the head of dbw_train_step_run, and T.zero_buf =
    ws + L.arena_begin of its Adam tail).  So after a launch vals[0] holds the raw sum, vals[5] the number of workgroups, and the launch
    here starts from zeros as the step's does."""
    g = rnd(900 + nparts)
    part_np = np.zeros(nparts, np.float32) if zeros else (g.rand(nparts) * 3 + 0.01).astype(np.float32)
    vals_np = np.array([0, 0.0123, 1.7, 0.31, 0, 0, 0, 0], np.float32)
    scale, tvs = 1.0 / (3 * 64 * max(nparts, 1)), 0.37
    ref = R.loss_finish(part_np, scale, tvs, vals_np)
    part, vals, out5 = dev(part_np) if nparts else None, Out((8,), torch.from_numpy(vals_np)), Out((5,), SENTINEL5)
    debug('dbw_debug_loss_finish', ptr(part), nparts, scale, tvs, vals.ptr, out5.ptr, stream())
    torch.cuda.synchronize()
    assert not vals.wrong('vals') + out5.wrong('out5')
    got, v = out5.np(), vals.np()
    assert not (got == np.float32(SENTINEL5)).any()          # every slot written
    F = Figures('composite', record_property)
    if nparts:
        F.torch(0, float(part.sum() * R.f32v(scale)), ref['rgb'], ref['M_rgb'], nparts)
    F.kernel('rgb', 0, got[0], ref['rgb'], ref['M_rgb'], max(nparts, 1), G=LOSS_BLOCKS)
    if zeros or nparts == 0:
        assert got[0] == 0.0 and v[0] == 0.0
    f = np.float32
    assert got[1] == vals_np[1] and got[3] == vals_np[3]
    assert got[2] == f(vals_np[2]) * f(tvs)
    assert got[4] == ((f(got[0]) + f(got[1])) + f(got[2])) + f(got[3])
    # the state left behind: the raw sum and the count of workgroups; slots 1..3 are read only
    F.kernel('vals[0]', 0, v[0], ref['sum'], ref['M_sum'], max(nparts, 1), G=LOSS_BLOCKS)
    assert got[0] == f(v[0]) * f(scale)
    assert int(vals.t.view(torch.int32)[5]) == LOSS_BLOCKS
    assert np.array_equal(v[1:5], vals_np[1:5]) and np.array_equal(v[6:], vals_np[6:])
    record_property('G', LOSS_BLOCKS)
    F.done(f'loss-finish n{nparts}{"-zero" if zeros else ""} G={LOSS_BLOCKS}', G=LOSS_BLOCKS)
