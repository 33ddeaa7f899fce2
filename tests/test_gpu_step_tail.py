"""GPU: the training step's last launch (csrc/texture.hip: adam_groups_tex_kernel, behind the join with the env chain) -- the backward of
the sky / ground texture preparation, Adam on both lr groups, the run's void latch and the zero-arena clear in one launch -- against
dbw_texture_prep_bwd_sets followed by dbw_adam_step_groups on identical inputs (bit-equal); and the C step at fuse 127 with Adam in the
call, in the schedule modes no other test runs that way, against the operator-level step (fuse 0).  `-m gpu`."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from dbw_amd import _lib                                        # noqa: E402
from trajectory import assert_same_trajectory                   # noqa: E402

DEV = 'cuda:0'
c_p, c_i, c_f, c_i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tail_fn():
    lib = _lib.load()
    fn = lib.dbw_debug_adam_tail           # (an undeclared export: tests only)
    fn.argtypes = [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_f, c_f, c_f, c_i, c_p, c_i64, c_i64, c_i64, c_p, c_i, c_p, c_p, c_p]
    fn.restype = c_i
    return lib, fn


# where the texture sets lie in the flat buffers: tex_n (one set's elements) -> (n, the sets' offsets, the lr groups' ends)
LAYOUTS = {
    'default': lambda t: (3 * t + 1234, [1000, 1000 + t + 777], [1000 + t // 2, 3 * t + 1234]),
    'no-sets': lambda t: (t + 1234, [], [600, t + 1234]),
    'one-set': lambda t: (2 * t + 1234, [1000], [1000 + t // 2, 2 * t + 1234]),
    'descending': lambda t: (3 * t + 1234, [1000 + t + 777, 1000], [1000 + t // 2, 3 * t + 1234]),          # the second set lower in memory than the first
    'offset-0': lambda t: (3 * t + 1234, [0, t + 777], [t // 2, 3 * t + 1234]),
    'ends-at-n': lambda t: (3 * t + 1234, [1000, 2 * t + 1234], [1000 + t // 2, 3 * t + 1234]),
    'adjacent': lambda t: (3 * t + 1234, [1000, 1000 + t], [1000 + t // 2, 3 * t + 1234]),
    'adjacent-descending': lambda t: (3 * t + 1234, [1000 + t, 1000], [1000 + t // 2, 3 * t + 1234]),
    'rest-0': lambda t: (2 * t, [0, t], [t // 2, 2 * t]),                                                    # the whole buffer is the two sets
    'rest-0-descending': lambda t: (2 * t, [t, 0], [t // 2, 2 * t]),
    'one-workgroup': lambda t: (2 * t + 100, [16, t + 60], [t // 2, 2 * t + 100]),                           # with a small set: grid_for(n) == 1, the launcher's grid = 2
}


def _case(ts, decim, tv, seed, shape=None, layout='default'):
    """flat buffers of 3 groups' worth of parameters, the sky texture straddling the lr groups' boundary, the ground texture in group 1
    (LAYOUTS: other placements; shape: (n, h, w) of a set instead of (1, ts, ts));
    an arena of random bytes whose hole holds the two prepared maps' gradients (cell resolution)"""
    g = torch.Generator().manual_seed(seed)
    tn, h, w = shape or (1, ts, ts)
    tex_n = tn * h * w * 3
    cells = tn * (h // decim) * (w // decim) * 3
    n, off, group_end = LAYOUTS[layout](tex_n)
    B = {'param': torch.randn(n, generator=g), 'grad': torch.randn(n, generator=g),
         'm': torch.randn(n, generator=g) * 0.1, 'v': torch.rand(n, generator=g) * 0.01}
    hole_lo = 4096
    hole_hi = hole_lo + (((2 * cells * 4 + 255) // 256) * 256 if off else 0)
    arena = torch.randint(1, 255, (hole_hi + 8192,), generator=g, dtype=torch.uint8)
    maps = torch.randn(2 * cells, generator=g)
    hole = torch.zeros((hole_hi - hole_lo) // 4)
    hole[:len(off) * cells] = maps[:len(off) * cells]          # (the lanes that read a map's gradient clear it: the hole holds nothing else)
    arena[hole_lo:hole_hi] = hole.view(torch.uint8)
    B['arena'] = arena
    B['gsig'] = torch.randn(2 * tex_n, generator=g) if tv else None
    B = {k: (None if v is None else v.to(DEV)) for k, v in B.items()}
    return B, dict(shape=(tn, h, w), decim=decim, tex_n=tex_n, cells=cells, off=off, group_end=group_end, hole=(hole_lo, hole_hi))


def _sets(B, c):
    maps = B['arena'][c['hole'][0]:].view(torch.float32)
    out = []
    tn, h, w = c['shape']
    for k, o in enumerate(c['off']):
        out.append(dict(texture=B['param'][o:].data_ptr(), n=tn, h=h, w=w, decim=c['decim'],
                        grad_maps=maps[k * c['cells']:].data_ptr(),
                        grad_sig=0 if B['gsig'] is None else B['gsig'][k * c['tex_n']:].data_ptr(),
                        grad_texture=B['grad'][o:].data_ptr()))
    return _lib.texture_sets(out)


ADAM = dict(lr=(5e-3, 5e-2), beta1=0.9, beta2=0.999, eps=1e-8, step=7)


def _reference(B, c, raised):
    lib = _lib.load()
    arr, ns = _sets(B, c)
    if ns:
        rc = lib.dbw_texture_prep_bwd_sets(arr, ns, _stream())
        assert rc == 0, lib.dbw_last_error()
    ends = (c_i64 * 2)(*c['group_end'])
    lr = (c_f * 2)(*ADAM['lr'])
    skip = torch.full((1,), raised, device=DEV)
    rc = lib.dbw_adam_step_groups(_p(B['param']), _p(B['grad']), _p(B['m']), _p(B['v']), ends, lr, 2, ADAM['beta1'], ADAM['beta2'], ADAM['eps'],
                                  ADAM['step'], _p(B['arena']), B['arena'].numel(), _p(skip), _stream())
    assert rc == 0, lib.dbw_last_error()


def _tail(B, c, raised):
    lib, fn = _tail_fn()
    arr, ns = _sets(B, c)
    ends = (c_i64 * 2)(*c['group_end'])
    lr = (c_f * 2)(*ADAM['lr'])
    void_raised = torch.full((1,), raised, device=DEV)
    void_flag = torch.full((1,), -5.0, device=DEV)
    rc = fn(_p(B['param']), _p(B['grad']), _p(B['m']), _p(B['v']), ends, lr, 2, ADAM['beta1'], ADAM['beta2'], ADAM['eps'], ADAM['step'],
            _p(B['arena']), B['arena'].numel(), c['hole'][0], c['hole'][1], arr, ns, _p(void_raised), _p(void_flag), _stream())
    assert rc == 0, lib.dbw_last_error()
    return void_flag


def _check_tail(ref, c, raised):
    got = {k: (None if v is None else v.clone()) for k, v in ref.items()}
    before = {k: (None if v is None else v.clone()) for k, v in ref.items()}
    _reference(ref, c, raised)
    flag = _tail(got, c, raised)
    torch.cuda.synchronize()
    for k in ('param', 'grad', 'm', 'v'):
        assert torch.equal(got[k].view(torch.int32), ref[k].view(torch.int32)), (k, float((got[k] - ref[k]).abs().max()))
    if raised:
        for k in ('param', 'm', 'v'):
            assert torch.equal(got[k], before[k]), k          # a voided step moves nothing ...
    else:
        assert not any(torch.equal(got[k], before[k]) for k in ('param', 'm', 'v'))
    if c['off']:
        assert not torch.equal(got['grad'], before['grad'])    # ... but its texture gradients are still written
    else:
        assert torch.equal(got['grad'], before['grad'])
    assert float(flag) == raised                                 # the latch
    # the whole arena is clear: the hole by the lanes that read it, the rest by the arena loop
    assert int(got['arena'].count_nonzero()) == 0
    assert int(ref['arena'].count_nonzero()) == 0


@pytest.mark.parametrize('raised', [0.0, 1.0])
@pytest.mark.parametrize('tv', [False, True])
@pytest.mark.parametrize('decim', [8, 1, 2, 4, 16])
def test_adam_tail_is_bit_equal_to_the_texture_backward_then_adam(decim, tv, raised):
    ref, c = _case(64, decim, tv, seed=11 + decim + 2 * tv)
    _check_tail(ref, c, raised)


@pytest.mark.parametrize('raised', [0.0, 1.0])
@pytest.mark.parametrize('decim', [1, 2, 4, 8, 16])
def test_adam_tail_on_several_oblong_maps_per_set(decim, raised):
    """sets of 3 maps of 16 x 48: n > 1 and h != w in the cell indexing of the decimated tail"""
    ref, c = _case(0, decim, True, seed=31 + decim, shape=(3, 16, 48))
    _check_tail(ref, c, raised)


@pytest.mark.parametrize('decim', [1, 4])
@pytest.mark.parametrize('layout', [k for k in LAYOUTS if k != 'default'])
def test_adam_tail_wherever_the_sets_lie_in_the_flat_buffers(layout, decim):
    """0, 1 and 2 sets; the second set lower in memory than the first (the launcher orders the ranges its compacted Adam index steps over);
    a set at offset 0, a set ending at n, adjacent sets, nothing but the two sets, and a buffer of one workgroup"""
    shape = (1, 4, 4) if layout == 'one-workgroup' else (3, 16, 48)
    ref, c = _case(0, decim, True, seed=51 + decim, shape=shape, layout=layout)
    if layout == 'one-workgroup':
        assert c['group_end'][-1] <= 256
    _check_tail(ref, c, 0.0)


def test_adam_tail_refuses_textures_outside_the_flat_buffers():
    B, c = _case(16, 8, True, seed=5)
    lib, fn = _tail_fn()
    outside = torch.zeros(16 * 16 * 3, device=DEV)
    arr, ns = _sets(B, c)
    arr[1].grad_texture = outside.data_ptr()
    ends = (c_i64 * 2)(*c['group_end'])
    lr = (c_f * 2)(*ADAM['lr'])
    raised = torch.zeros(1, device=DEV)
    rc = fn(_p(B['param']), _p(B['grad']), _p(B['m']), _p(B['v']), ends, lr, 2, 0.9, 0.999, 1e-8, 1, _p(B['arena']), B['arena'].numel(),
            c['hole'][0], c['hole'][1], arr, ns, _p(raised), None, _stream())
    assert rc != 0


# ---- the C step at fuse 127 with Adam in the call, in the modes no other test runs that way ----

import oracle as O                                              # noqa: E402  (checker only)
import dbw_amd                                                  # noqa: E402
from dbw_amd.parallel import ShardedTrainStep                   # noqa: E402


def _cfg(n_blocks, ts, fpp):
    return {'model': {'name': 'dbw', 'mesh': {'n_blocks': n_blocks, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': ts},
                      'renderer': {'faces_per_pixel': fpp, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                      'rend_optim': {'coarse_learning': 1500, 'decimate_txt': 750, 'decimate_factor': 8, 'kill_blocks': True,
                                     'decouple_rendering': True, 'opacity_noise': True},
                      'loss': {'rgb_weight': 1, 'perceptual_weight': 0, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}}}


def _model(epoch, nb=10, ts=256, fpp=10, H=300, W=400):
    torch.manual_seed(227391)
    model = dbw_amd.create_model(_cfg(nb, ts, fpp), (H, W)).to(DEV).train()
    with torch.no_grad():
        model.T.mul_(0.5)
    model.set_cur_epoch(epoch)
    model.sync_free = True
    return model


def _run(epoch, inp, noise, u, fuse, mode, steps=3):
    model = _model(epoch)
    model._noise_override, model._overlap_u_override = noise, u
    step = ShardedTrainStep(model, lr=5e-3, lr_texture=5e-2, seed=99, use_c_step=True, fuse=fuse)
    for k, v in mode.items():
        setattr(step.cstep, k, v)
    out = step(inp)
    torch.cuda.synchronize()
    vals = {k: float(v) for k, v in out.items()}
    grad1 = step.params.grad.clone()
    for _ in range(steps - 1):
        step(inp)
    torch.cuda.synchronize()
    assert step.cstep.supported() and step.cstep._cur is not None, 'the C step did not run'
    return step, vals, grad1, step.params.flat.clone()


def _tail_ran(step):
    fn = _lib.load().dbw_debug_train_step_last_tail           # (an undeclared export: tests only)
    fn.argtypes, fn.restype = [c_p], c_i
    return fn(step.cstep._cur[0])


# The one-launch tail runs where the env backward ends last: more than serial_setup_max_views views on decimated maps (no texture bins).
# At 5 views the threshold is lowered to 2 to get it; epoch 800 (texture bins) and single_stream keep the parent's order, also at fuse 127.
# (binned_concurrent 1 and the other modes at the default threshold already run at fuse 127 in test_gpu_c_step.py)
TAIL = {'serial_setup_max_views': 2}
MODES = [(0, dict(TAIL)), (0, dict(TAIL, backward_order=1)), (0, dict(TAIL, sync_events=True)), (800, {'backward_order': 1}),
         (800, {'binned_concurrent': 0}), (0, {'use_side_stream': False})]


@pytest.mark.parametrize('epoch,mode', MODES, ids=[f'e{e}-' + '-'.join(f'{k}{int(v)}' for k, v in m.items()) for e, m in MODES])
def test_c_step_tail_in_other_schedule_modes_equals_operator_level_step(epoch, mode):
    """Config-2 geometry on 5 views.  Gradients and parameters: the tolerances and trajectory helper of test_gpu_c_step.py.  Loss values:
    sums of unordered fp32 atomics, so the bar is their own spread -- the largest difference between two runs of the same build (fuse 0
    twice, fuse 127 twice), times 4, plus 4 ulp of the value (a spread that happens to come out 0 still leaves room for one more
    reordering of the sums)."""
    R, T, Km = O.synthetic_cameras(5, R_world=O.world_rotation(115, 0, 0))
    imgs = torch.rand(5, 3, 300, 400, generator=torch.Generator().manual_seed(2))
    inp = {k: v.to(DEV) for k, v in dict(imgs=imgs, R=R, T=T, K=Km).items()}
    noise = torch.randn(10, generator=torch.Generator().manual_seed(3)).to(DEV)
    u = torch.rand(10, 1000, 3, generator=torch.Generator().manual_seed(4)).to(DEV)
    refs = [_run(epoch, inp, noise, u, 0, mode) for _ in range(2)]
    gots = [_run(epoch, inp, noise, u, 127, mode) for _ in range(2)]
    ref, got = refs[0], gots[0]
    assert [_tail_ran(r[0]) for r in refs + gots] == [0, 0] + [int('serial_setup_max_views' in mode)] * 2
    for k in ref[1]:
        spread = max(abs(refs[0][1][k] - refs[1][1][k]), abs(gots[0][1][k] - gots[1][1][k]))
        bar = 4 * spread + 4 * 2.0 ** -23 * abs(ref[1][k])
        diff = abs(got[1][k] - ref[1][k])
        print(f'{k}: fuse127 - fuse0 {diff:.3e}, spread {spread:.3e}, bar {bar:.3e}')
        assert diff <= bar, (k, got[1][k], ref[1][k], spread)
    for n, off, k in ref[0].params.names:
        x, y = got[2][off:off + k], ref[2][off:off + k]
        assert float((x - y).abs().max()) <= 1e-5 * float(y.abs().max()) + 1e-12, (n, float((x - y).abs().max()), float(y.abs().max()))
    assert_same_trajectory(got[3], ref[3])


def _void_step(events, threshold):
    torch.manual_seed(227391)
    model = dbw_amd.create_model(_cfg(4, 32, 6), (48, 64)).to(DEV).train()
    with torch.no_grad():
        model.T.mul_(0.5)
        model.alpha_logit.add_(torch.tensor([1.0, -6.0, 0.3, 2.0], device=DEV))
    model.set_cur_epoch(0)
    model.sync_free = True
    model._noise_override = torch.zeros(4, device=DEV)
    model._overlap_u_override = torch.rand(4, 1000, 3, generator=torch.Generator().manual_seed(4)).to(DEV)
    step = ShardedTrainStep(model, lr=5e-3, lr_texture=5e-2, seed=99)
    step.cstep.sync_events = events
    step.cstep.serial_setup_max_views = threshold
    return step


def _small_inputs():
    R, T, Km = O.synthetic_cameras(2, R_world=O.world_rotation(115, 0, 0))
    imgs = torch.rand(2, 3, 48, 64, generator=torch.Generator().manual_seed(2))
    return {k: v.to(DEV) for k, v in dict(imgs=imgs, R=R, T=T, K=Km).items()}


@pytest.mark.parametrize('hasty', [False, True], ids=['join', 'prologue'])
def test_one_launch_tail_is_voided_by_a_poll_that_gave_up(hasty):
    """The void protocol with the one-launch tail on (2 views, threshold 1): the join's poll for the env chain given up for real (0.05 s), or
    the side streams' prologue polls given up in front of a main stream stalled for 0.25 s -- the tail's latch sits behind the last poll of
    the run, so Adam moves no parameter and no moment; the plan goes on through events and equals a reference run on events."""
    import warnings
    inp = _small_inputs()
    ref = _void_step(True, 1)
    ref(inp)
    ref(inp)
    step = _void_step(False, 1)
    step(inp)
    torch.cuda.synchronize()
    assert step.cstep.sync_timeouts() == 0 and step.cstep.voided_runs() == 0 and _tail_ran(step) == 1
    cycles = 0
    if hasty:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); torch.cuda._sleep(20_000_000); e1.record(); torch.cuda.synchronize()
        cycles = int(20_000_000 * 250.0 / max(e0.elapsed_time(e1), 1e-3))
    before = (step.params.flat.clone(), step.exp_avg.clone(), step.exp_avg_sq.clone())
    _lib.call('dbw_debug_train_step_hasty_prologue_wait' if hasty else 'dbw_debug_train_step_force_timeout', step.cstep._cur[0])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        if hasty:
            torch.cuda._sleep(cycles)
        step(inp)
        torch.cuda.synchronize()
        assert step.cstep.sync_timeouts() >= 1 and step.cstep.voided_runs() == 1
        assert step.cstep.last_timeout()[0] == ('prologue' if hasty else 'env chain') and _tail_ran(step) == 1
        for a, b in zip(before, (step.params.flat, step.exp_avg, step.exp_avg_sq)):
            assert torch.equal(a, b)
        step.n_steps -= 1                  # (line the Adam step count up with the reference's two applied steps)
        out = step(inp)
        torch.cuda.synchronize()
    assert any('gave up' in str(x.message) for x in w)
    assert step.cstep.voided_runs() == 1
    assert all(torch.isfinite(v).all() for v in out.values())
    assert_same_trajectory(step.params.flat, ref.params.flat)
