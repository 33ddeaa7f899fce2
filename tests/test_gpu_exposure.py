"""GPU tests of the per-view exposure compensation: dbw_monitor_exposure_composite (csrc/exposure_loss.hip) and the model,
the step and the trainer with a batch that carries `exposure`.  `-m gpu`.

Kernels.  exposure_ref.CASES -- (N,H,W) in {(1,1,1), (2,5,7), (3,12,16), (3,40,100)}: the element path, the 16-byte path, more than one
workgroup a view with a ragged last one; masks in {none, random in [0, 1], one view all zero}; V = 5 rows, ids a shuffled subset, theta
random in +-0.3 -- each with and without a gradient sent to rec, held to the numpy float64 restatement of tests/exposure_ref.py (whose
gradients tests/test_host_exposure_math.py holds to central differences):
  rec, grad_fg, grad_env   within 1e-4 of the largest element of the reference (the project's tolerance for images and gradients),
  value                    within 1e-5 relative,
  each of the six sums     |dev - ref64| <= 1e-5 * sum|terms| (a term passes through about eight fp32 roundings of 6e-8, the sum is fp64:
                           a margin of about 20).
Rows of grad_theta outside ids keep a sentinel's bits; a second call adds exactly the first call's sums; two runs give the same bytes; an
id of -1 or V touches no row and gives the plain composite; theta = 0 gives ops.composite's rec bit for bit and, with masks,
composite_mse_masked's rec bit for bit and its value to 1e-12 relative (another order of the same fp64 additions).

Model (the tiny model of tests/test_gpu_masked_loss.py: 2 views of 32 x 48, 3 blocks, perceptual_name: ssim): a batch with `exposure`
against a float64 torch restatement on render_layers' output; the batch without the key never reaches the new entry point; neither the C
step nor the native step sees such a batch.  Optimum: targets made from the model's own composite with known gains and offsets; at the
least-squares theta the gradient vanishes.  Trainer: two epochs on 6 views of 12 x 16, and a resume after the first that gives the bits of
the uninterrupted run."""
import math

import numpy as np
import pytest
import torch

import exposure_ref as ER
import oracle as O
import dbw_amd
from dbw_amd import metrics, ops, phase
from dbw_amd.parallel import ShardedTrainStep
from dbw_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IDS = [ER.case_id(c) for c in ER.CASES]


def _dev(c):
    t = {k: (None if c[k] is None else c[k].to(DEV)) for k in ('fg', 'env', 'imgs', 'm', 'x', 'theta', 'ids')}
    t['up'] = torch.tensor([ER.UPSTREAM], dtype=torch.float32, device=DEV)
    return t


def _fwd(t, c, theta=None, ids=None):
    value, rec, _ = ops.exposure_composite_fwd(t['fg'], t['env'], t['imgs'], t['m'], t['theta'] if theta is None else theta,
                                               t['ids'] if ids is None else ids, c['scale'])
    return value, rec


def _bwd(t, c, extra, theta=None, ids=None, grad_theta=None):
    return ops.exposure_composite_bwd(t['fg'], t['env'], t['imgs'], t['m'], t['theta'] if theta is None else theta,
                                      t['ids'] if ids is None else ids, c['scale'], t['up'], t['x'] if extra else None, grad_theta=grad_theta)


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize('shape,mkind', ER.CASES, ids=IDS)
def test_kernel_accuracy(shape, mkind):
    c = ER.case(shape, mkind)
    t = _dev(c)
    value, rec = _fwd(t, c)
    for extra in (False, True):
        gfg, genv, gth = _bwd(t, c, extra)
        torch.cuda.synchronize()
        ref = ER.reference(c, extra)
        big = lambda a: float(np.abs(a).max())
        e_rec = float(np.abs(rec.cpu().double().numpy() - ref['rec']).max())
        e_fg, e_env = float(np.abs(gfg.cpu().double().numpy() - ref['gfg']).max()), float(np.abs(genv.cpu().double().numpy() - ref['genv']).max())
        e_v = abs(value.item() - ref['value'])
        e_th = np.abs(gth.cpu().double().numpy() - ref['gth'])
        print(f"{ER.case_id((shape, mkind))} extra={extra}: rec err {e_rec:.2e} of {big(ref['rec']):.2e}; value {value.item():.9e} err {e_v:.2e}; "
              f"grad_fg err {e_fg:.2e} of {big(ref['gfg']):.2e}; grad_env err {e_env:.2e} of {big(ref['genv']):.2e}; "
              f"sums err / sum|terms| {float(np.max(e_th / np.maximum(ref['ath'], 1e-300))):.2e}")
        assert bool(torch.isfinite(rec).all() and torch.isfinite(gfg).all() and torch.isfinite(genv).all() and torch.isfinite(gth).all())
        assert e_rec <= 1e-4 * big(ref['rec']) and e_fg <= 1e-4 * big(ref['gfg']) and e_env <= 1e-4 * big(ref['genv'])
        assert e_v <= 1e-5 * abs(ref['value'])
        assert (e_th <= 1e-5 * ref['ath']).all()
        assert not genv[:, 3].any()


@pytest.mark.parametrize('shape,mkind', ER.CASES, ids=IDS)
def test_rows_and_repeatability(shape, mkind):
    c = ER.case(shape, mkind)
    t = _dev(c)
    inside = c['ids'].long().tolist()
    outside = [i for i in range(ER.V) if i not in inside]
    value, rec = _fwd(t, c)
    value2, rec2 = _fwd(t, c)
    assert torch.equal(value, value2) and torch.equal(rec, rec2)                       # two runs: the same bytes
    for extra in (False, True):
        gfg, genv, first = _bwd(t, c, extra)
        gfg2, genv2, again = _bwd(t, c, extra)
        assert torch.equal(gfg, gfg2) and torch.equal(genv, genv2) and torch.equal(first, again)
        assert not first[outside].any()
        # rows outside ids keep a sentinel's bits; the rows inside receive the sums on top of it
        table = torch.full((ER.V, 6), 7.25, dtype=torch.float32, device=DEV)
        _, _, out = _bwd(t, c, extra, grad_theta=table)
        assert out is table and torch.equal(table[outside], torch.full((len(outside), 6), 7.25, device=DEV))
        assert torch.equal(table[inside], 7.25 + first[inside])
        # a second call adds exactly the first call's sums again
        twice = first.clone()
        _bwd(t, c, extra, grad_theta=twice)
        assert torch.equal(twice, 2 * first)
        # an id of -1 or V: no row is touched, theta reads as 0 -- the gradients of the plain composite
        zero = torch.zeros_like(t['theta'])
        for bad in (-1, ER.V):
            ids = torch.full_like(t['ids'], bad)
            table = torch.full((ER.V, 6), 7.25, dtype=torch.float32, device=DEV)
            gfg_b, genv_b, _ = _bwd(t, c, extra, ids=ids, grad_theta=table)
            gfg_0, genv_0, _ = _bwd(t, c, extra, theta=zero)
            assert torch.equal(table, torch.full_like(table, 7.25)) and torch.equal(gfg_b, gfg_0) and torch.equal(genv_b, genv_0)
    plain = ops.composite(t['fg'], t['env'])
    for bad in (-1, ER.V):
        _, rec_b = _fwd(t, c, ids=torch.full_like(t['ids'], bad))
        assert torch.equal(rec_b, plain)
    if shape[0] > 1:                                                                   # one bad id among good ones: only its row is skipped
        ids = t['ids'].clone()
        ids[0] = ER.V
        ref = ER.reference(c, True, ids=ids.cpu())
        _, rec_m = _fwd(t, c, ids=ids)
        _, _, gth = _bwd(t, c, True, ids=ids)
        assert torch.equal(rec_m[0], plain[0]) and torch.equal(rec_m[1:], rec[1:])
        assert (np.abs(gth.cpu().double().numpy() - ref['gth']) <= 1e-5 * ref['ath']).all() and not gth[inside[0]].any()


@pytest.mark.parametrize('shape,mkind', ER.CASES, ids=IDS)
def test_zero_theta_is_the_composite(shape, mkind):
    c = ER.case(shape, mkind)
    t = _dev(c)
    zero = torch.zeros_like(t['theta'])
    value, rec = _fwd(t, c, theta=zero)
    assert torch.equal(rec, ops.composite(t['fg'], t['env']))
    if c['m'] is not None:
        value_m, rec_m, _ = ops.masked_composite_fwd(t['fg'], t['env'], t['imgs'], t['m'], c['scale'])
        assert torch.equal(rec, rec_m)
        assert abs(value.item() - value_m.item()) <= 1e-12 * abs(value_m.item())
        for extra in (False, True):                                                    # ... and the gradients through the composite
            gfg, genv, _ = _bwd(t, c, extra, theta=zero)
            gfg_m, genv_m = ops.masked_composite_bwd(t['fg'], t['env'], t['imgs'], t['m'], c['scale'], t['up'], t['x'] if extra else None)
            assert torch.equal(gfg, gfg_m) and torch.equal(genv, genv_m)
    # the element path on the shapes of the 16-byte path: a pointer off the 16-byte grid, the same bits
    pad = lambda a: torch.cat([a.new_zeros(1), a.flatten()])[1:].view(a.shape)
    value_e, rec_e, _ = ops.exposure_composite_fwd(pad(t['fg']), t['env'], t['imgs'], t['m'], t['theta'], t['ids'], c['scale'])
    value_v, rec_v = _fwd(t, c)
    assert torch.equal(rec_e, rec_v) and abs(value_e.item() - value_v.item()) <= 1e-12 * abs(value_v.item())
    gfg_e, genv_e, gth_e = ops.exposure_composite_bwd(pad(t['fg']), t['env'], t['imgs'], t['m'], t['theta'], t['ids'], c['scale'], t['up'], t['x'])
    gfg_v, genv_v, gth_v = _bwd(t, c, True)
    assert torch.equal(gfg_e, gfg_v) and torch.equal(genv_e, genv_v)
    ath = torch.from_numpy(ER.reference(c, True)['ath']).to(DEV)
    assert bool(((gth_e.double() - gth_v.double()).abs() <= 1e-6 * ath).all())         # (fp64 sums in another order, rounded to fp32)


def test_function_is_one_node_and_accumulates_in_place(monkeypatch):
    c = ER.case((3, 12, 16), 'random')
    t = _dev(c)
    calls, call = [], ops._lib.call
    monkeypatch.setattr(ops._lib, 'call', lambda name, *a: calls.append(name) or call(name, *a))
    f, e = t['fg'].clone().requires_grad_(True), t['env'].clone().requires_grad_(True)
    flat = torch.zeros(ER.V * 6, device=DEV)
    grad = torch.full_like(flat, 0.5)
    with torch.no_grad():
        flat.copy_(t['theta'].reshape(-1))
    theta = flat.view(ER.V, 6).requires_grad_(True)
    theta.grad = grad.view(ER.V, 6)
    value, rec = ops.composite_mse_exposure(f, e, t['imgs'], t['m'], ER.WEIGHT, c['count'], theta, t['ids'].long(), ids_host=c['ids'].tolist())
    assert value.dim() == 0 and value.dtype == torch.float32 and rec.shape == t['imgs'].shape
    n_fwd = len(calls)
    (ER.UPSTREAM * value + (t['x'] * rec).sum()).backward()
    assert calls[n_fwd:] == ['dbw_monitor_exposure_composite']                         # ONE call for both incoming gradients
    want_fg, want_env, want_th = _bwd(t, c, True)
    assert torch.equal(f.grad, want_fg) and torch.equal(e.grad, want_env)
    assert theta.grad.data_ptr() == grad.data_ptr() and torch.equal(grad.view(ER.V, 6), 0.5 + want_th)      # accumulated into the flat buffer
    # only rec is used downstream: the scalar's gradient is 0
    f.grad = e.grad = None
    value, rec = ops.composite_mse_exposure(f, e, t['imgs'], t['m'], ER.WEIGHT, c['count'], theta.detach(), t['ids'])
    (t['x'] * rec).sum().backward()
    g0, e0, _ = ops.exposure_composite_bwd(t['fg'], t['env'], t['imgs'], t['m'], t['theta'], t['ids'], c['scale'], torch.zeros(1, device=DEV), t['x'])
    assert torch.equal(f.grad, g0) and torch.equal(e.grad, e0)
    with pytest.raises(ValueError, match='distinct'):
        ops.composite_mse_exposure(f, e, t['imgs'], t['m'], ER.WEIGHT, c['count'], theta, t['ids'], ids_host=[1, 1, 2])


# ---------------------------------------------------------------------------------------------------------------- the model
H, W, NB, TS, FPP = 32, 48, 3, 16, 4
WEIGHT = 0.1
N_ROWS = 5
ROWS = [3, 1]                                     # the batch's rows of theta


def _cfg(perceptual=True):
    term = {'perceptual_weight': WEIGHT, 'perceptual_name': 'ssim'} if perceptual else {}
    return {'model': {'name': 'dbw', 'mesh': {'n_blocks': NB, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': TS},
                      'renderer': {'faces_per_pixel': FPP, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                      'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True,
                                     'opacity_noise': False},
                      'loss': dict({'rgb_weight': 1, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}, **term)}}


def _model(perceptual=True, size=(H, W)):
    torch.manual_seed(227391)
    model = dbw_amd.create_model(_cfg(perceptual), size).to(DEV).train()
    model._overlap_u_override = torch.rand(NB, 1000, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    return model


def _theta(seed=11):
    return ((torch.rand(N_ROWS, 6, generator=torch.Generator().manual_seed(seed)) - 0.5) * 0.6).to(DEV)


@pytest.fixture(scope='module')
def inp():
    R, T, Km = O.synthetic_cameras(2, R_world=O.world_rotation(115, 0, 0))
    imgs = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(0))
    batch = {k: v.to(DEV) for k, v in dict(imgs=imgs, R=R, T=T, K=Km).items()}
    batch['view_ids'] = torch.tensor(ROWS, device=DEV)
    return batch


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'masks'])
def test_model_losses_and_gradients(inp, masked):
    batch = dict(inp)
    if masked:
        m = torch.ones(2, 1, H, W)
        m[0, :, 8:17, 20:33] = 0
        m[1, :, :, :5] = 0
        batch['masks'] = m.to(DEV)
    model = _model()
    theta = _theta().requires_grad_(True)
    out = model(dict(batch, exposure=theta))
    out['total'].backward()
    # the same model with both image terms restated in float64 torch on render_layers' output
    ref = _model()
    ref.loss_weights.pop('perceptual')
    plain = {k: v for k, v in inp.items()}
    fg, env = ref.render_layers(plain)
    regs = ref.compute_losses(plain['imgs'], None, layers=None, rgb_value=torch.zeros((), device=DEV))['total']
    factor = phase.phase_of(model, True).perceptual_factor
    imgs = plain['imgs'].double()
    th = theta.detach().double().requires_grad_(True)
    fg64, env64 = fg.double(), env.double()
    comp = fg64[:, :3] * fg64[:, 3:4] + (1 - fg64[:, 3:4]) * env64[:, :3]
    rows = th[ROWS]
    rec = rows[:, :3].exp()[:, :, None, None] * comp + rows[:, 3:, None, None]
    if masked:
        mk = batch['masks'].double()
        count = 3 * mk.sum().item()
        rgb = (mk * (rec - imgs) ** 2).sum() / count
        per = WEIGHT * factor * ((1 - metrics.ssim_map(imgs * mk, rec * mk, padding=True)) * mk).sum() / count
    else:
        rgb = ((rec - imgs) ** 2).mean()
        per = WEIGHT * factor * (1 - metrics.ssim_map(imgs, rec, padding=True)).mean()
    total = regs.double() + rgb + per
    total.backward()
    torch.cuda.synchronize()
    print(f"model masked={masked}: rgb {out['rgb'].item():.9f} (float64 {rgb.item():.9f}), perceptual {out['perceptual'].item():.9f} "
          f"(float64 {per.item():.9f}), total {out['total'].item():.9f} (float64 {total.item():.9f}); "
          f"grad theta rel err {_rel(theta.grad.double(), th.grad):.2e}")
    assert abs(out['rgb'].item() - rgb.item()) <= 1e-5 * rgb.item() and abs(out['perceptual'].item() - per.item()) <= 1e-5 * per.item()
    assert abs(out['total'].item() - total.item()) <= 1e-5 * abs(total.item())
    assert _rel(theta.grad.double(), th.grad) < 1e-4 and not theta.grad[[0, 2, 4]].any()
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert (p.grad is None) == (q.grad is None), n
        if p.grad is not None:
            assert _rel(p.grad, q.grad) < 1e-4, f'grad {n}: rel err {_rel(p.grad, q.grad)}'


# Two calls that enqueue the same work differ only in the order of the float atomic additions (tests/test_gpu_pose.py: ORDER_ULPS): eight
# units in the last place of the largest element of a tensor is the room the project gives to that.
ORDER_ULPS = 8


def test_a_batch_without_the_key_goes_through_todays_code(inp):
    """A key-less batch before any exposed batch was seen, an exposed batch, the key-less batch again: the second key-less call enqueues
    the work of the first -- the same library calls in the same order with the same sizes, flags and scales, a call recorded as its name
    and every argument that is not a pointer -- and the new entry point is not among them.

    What of its result is bytes: everything up to the first float atomic.  The layers render_layers hands to the loss are the same bits
    before and after (the forward render has no atomics); so is `perceptual` (the SSIM kernels add in a fixed order), and `rgb` where
    the fused epilogue forms it (no perceptual term: csrc/render_fused.hip reduces without atomics).  The other values of the key-less
    path are NOT reproducible to the bit between two identical calls, with or without this feature: dbw_composite_mse
    (csrc/texture.hip: composite_mse_kernel, one unsafeAtomicAdd per workgroup, three workgroups at this size), the TV, parsimony and
    overlap kernels (csrc/texture.hip, csrc/model_ops.hip) add their workgroups' partial sums into one float with atomics, and the
    parameter gradients are summed by atomics as well.  They are held to ORDER_ULPS units in the last place of the value (of a
    gradient's largest element), the bound tests/test_gpu_pose.py uses for two identical calls; which of them came out bit-equal is
    printed.  The exposed batch at theta = 0 gives the key-less losses to 1e-5 relative, the bound the issue sets for the model's
    losses (another path and another order of summation: the fp64 fixed-order sum against fp32 atomics)."""
    argtypes = dict(ops._lib.SIGNATURES)
    for f in ops._lib.FAMILIES.values():
        argtypes.update(f.signatures)
    calls, call = [], ops._lib.call

    def recording(name, *args):
        calls.append((name,) + tuple(a for a, t in zip(args, argtypes[name]) if t is not ops._lib.c_p))
        return call(name, *args)

    def run(model, batch):
        del calls[:]
        model.zero_grad(set_to_none=True)
        ops._lib.call = recording
        try:
            out = model(batch)
            out['total'].backward()
            torch.cuda.synchronize()
        finally:
            ops._lib.call = call
        grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        with torch.no_grad():
            layers = [t.clone() for t in model.render_layers(batch)]
        return {k: v.detach().clone() for k, v in out.items()}, grads, layers, list(calls)

    room = ORDER_ULPS * 2.0 ** -23
    for perceptual in (True, False):
        model = _model(perceptual)
        run(model, dict(inp))                                    # (a first call differs from later ones: the texture bins have no demand yet)
        out0, grads0, layers0, calls0 = run(model, dict(inp))    # key-less, before any exposed batch
        theta = torch.zeros(N_ROWS, 6, device=DEV, requires_grad=True)
        out_e, _, _, calls_e = run(model, dict(inp, exposure=theta))
        out1, grads1, layers1, calls1 = run(model, dict(inp))    # key-less, after it
        assert calls0 and not any(c[0] == 'dbw_monitor_exposure_composite' for c in calls0)
        assert calls1 == calls0                                  # names, sizes, flags, scales
        mine = [c for c in calls_e if c[0] == 'dbw_monitor_exposure_composite']
        assert len(mine) == 2 and all(c[1:5] == (2, H, W, N_ROWS) for c in mine)       # the forward and the backward: N, H, W, V
        assert torch.equal(layers1[0], layers0[0]) and torch.equal(layers1[1], layers0[1])
        exact = ['perceptual'] if perceptual else ['rgb']
        for k in out0:
            same = torch.equal(out1[k], out0[k])
            print(f"perceptual={perceptual} {k}: {out0[k].item():.9e} before, {out1[k].item():.9e} after{' (same bits)' if same else ''}")
            if k in exact:
                assert same, k
            assert abs(out1[k].item() - out0[k].item()) <= room * abs(out0[k].item()), k
            assert abs(out_e[k].item() - out0[k].item()) <= 1e-5 * abs(out0[k].item()), k
        assert set(grads1) == set(grads0)
        for n in grads0:
            assert _rel(grads1[n], grads0[n]) <= room, n
    with pytest.raises(KeyError, match='view_ids'):
        model({k: v for k, v in dict(inp, exposure=theta).items() if k != 'view_ids'})


def test_refusals(inp):
    theta = torch.zeros(N_ROWS, 6, device=DEV)
    model = _model()
    model.decouple_rendering = False
    with pytest.raises(NotImplementedError, match='a batch with exposure: decouple_rendering is off'):
        model(dict(inp, exposure=theta))
    model = _model()
    model.world_size = 2
    with pytest.raises(NotImplementedError, match='a batch with exposure: data-parallel'):
        model(dict(inp, exposure=theta))
    model = _model()
    model.default_criteria = False
    with pytest.raises(NotImplementedError, match='a batch with exposure: criteria'):
        model(dict(inp, exposure=theta))


def test_exposed_batch_reaches_neither_the_c_step_nor_the_native_step(inp, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('a batch with exposure reached a step without the term')
    # with the SSIM term the one-call C step would take the batch, without a perceptual term (and the C step off) the native step would
    for perceptual in (True, False):
        model = _model(perceptual)
        model.sync_free = True
        step = ShardedTrainStep(model, lr=1e-3, lr_texture=1e-2, seed=1, use_c_step=perceptual)
        if perceptual:
            assert step.cstep is not None and step.cstep.supported()
        else:
            assert step.cstep is None and step.native is not None and step.native.supported()
        monkeypatch.setattr(step, '_c_iteration', refuse)
        monkeypatch.setattr(type(step.native), '__call__', refuse)
        theta = _theta().requires_grad_(True)
        losses = step(dict(inp, exposure=theta))
        torch.cuda.synchronize()
        assert all(math.isfinite(float(v)) for v in losses.values()) and float(losses['rgb']) > 0 and step.n_steps == 1
        assert ('perceptual' in losses) == perceptual and bool(theta.grad[ROWS].any()) and not theta.grad[[0, 2, 4]].any()
    step.world_size = 2
    with pytest.raises(NotImplementedError, match='exposure'):
        step(dict(inp, exposure=theta))


def test_the_least_squares_exposure_is_the_optimum(inp):
    """Targets: the model's own composite under known per-view gains and offsets.  The model is frozen, there are no masks and no
    perceptual term, so theta meets the loss through the reconstruction term alone, and the float64 least-squares fit of (gain, offset)
    per view and channel from the composite is its minimiser: there the gradient is 1e-4 of what it is at theta = 0, no optimiser run."""
    model = _model(perceptual=False)
    seen, node = [], ops.composite_mse_exposure

    def spy(*a, **k):
        out = node(*a, **k)
        seen.append(out[1].detach().clone())
        return out
    ops.composite_mse_exposure = spy
    try:
        model(dict(inp, exposure=torch.zeros(N_ROWS, 6, device=DEV)))
    finally:
        ops.composite_mse_exposure = node
    comp = seen[0]                                                                      # theta = 0: rec is the composite
    gains = torch.tensor([[1.15, 0.9, 1.05], [0.8, 1.25, 0.95]], device=DEV)
    offsets = torch.tensor([[0.03, -0.02, 0.0], [-0.04, 0.01, 0.05]], device=DEV)
    targets = gains[:, :, None, None] * comp + offsets[:, :, None, None]
    x, y = comp.double().flatten(2), targets.double().flatten(2)                        # (2,3,P)
    xm, ym = x.mean(2, keepdim=True), y.mean(2, keepdim=True)
    g_ls = (((x - xm) * (y - ym)).sum(2) / ((x - xm) ** 2).sum(2))
    b_ls = ym[:, :, 0] - g_ls * xm[:, :, 0]
    assert float((g_ls - gains.double()).abs().max()) <= 1e-5 and float((b_ls - offsets.double()).abs().max()) <= 1e-5

    def grad_at(theta):
        theta = theta.clone().requires_grad_(True)
        model.zero_grad(set_to_none=True)
        model(dict(inp, imgs=targets, exposure=theta))['total'].backward()
        return theta.grad.clone()
    best = torch.zeros(N_ROWS, 6, device=DEV)
    best[ROWS] = torch.cat([g_ls.log(), b_ls], 1).float()
    g0, g1 = grad_at(torch.zeros(N_ROWS, 6, device=DEV)), grad_at(best)
    torch.cuda.synchronize()
    print(f'|grad| at theta = 0: {g0.norm().item():.3e}, at the least-squares theta: {g1.norm().item():.3e}')
    assert g0.norm().item() > 0 and g1.norm().item() <= 1e-4 * g0.norm().item()
    assert float((best[ROWS, :3].exp().double() - gains.double()).abs().max()) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- the trainer
TH, TW, TV = 12, 16, 6


def _trainer(lr=0.0, lr_texture=0.0):
    """6 views of 12 x 16.  By default the model's learning rates are 0: its parameters stand still (the render backward adds with float atomics, so
    two runs of a moving model differ in their last bits, tests/trajectory.py), while theta -- whose gradient comes out of kernels without
    atomics, behind a forward that is the same from run to run -- is optimised with lr 1e-2 and can be compared bit for bit."""
    model = _model(size=(TH, TW))
    R, T, Km = O.synthetic_cameras(TV, R_world=O.world_rotation(115, 0, 0))
    g = torch.Generator().manual_seed(4)
    imgs = torch.rand(TV, 3, TH, TW, generator=g) * (0.6 + 0.8 * torch.rand(TV, 1, 1, 1, generator=g))
    views = {k: v.to(DEV) for k, v in dict(imgs=imgs.clamp(0, 1), R=R, T=T, K=Km).items()}
    cfg = {'training': {'batch_size': 2, 'n_epoches': 2, 'seed': 3, 'optimizer': {'name': 'adam', 'lr': lr, 'texture': {'lr': lr_texture}},
                        'scheduler': {'name': 'multi_step'}, 'exposure': {'lr': 1e-2}}}
    return Trainer(cfg, model, views), views


def test_trainer_two_epochs_and_a_resume_after_the_first(tmp_path, monkeypatch):
    full, views = _trainer()
    assert full.exposure is not None and full.exposure.lr == 1e-2 and full.view_ids
    seen, step = [], full.step_fn.__call__
    monkeypatch.setattr(type(full.step_fn), '__call__', lambda self, batch, **k: seen.append(batch) or step.__func__(self, batch, **k))
    totals = [float(full.run_epoch(shuffle=False)['total']) for _ in range(2)]
    torch.cuda.synchronize()
    assert len(seen) == 6 and all(b['exposure'] is full.exposure.theta and 'view_ids' in b for b in seen)
    theta = full.exposure.flat.view(TV, 6)
    print('trainer with exposure, total per epoch:', totals, 'theta rows:', theta.tolist())
    assert all(math.isfinite(v) for v in totals) and bool(theta.abs().max() > 1e-3) and bool((theta != 0).all())
    # centred after every step: the column means are zero up to the rounding of fp32 values of size 0.1
    assert float(theta.mean(0).abs().max()) <= 1e-7
    assert full.exposure.n_steps == 6 and not full.exposure.grad.any()
    # evaluate writes the table (the two evaluation walks stubbed: they are not what is tested here)
    monkeypatch.setattr(full.model, 'qualitative_eval', lambda loader, device, path=None, **kw: None)
    monkeypatch.setattr(full.model, 'quantitative_eval', lambda loader, device, hard_inference=True: {'PSNR': 1.0})
    full.evaluate([], tmp_path)
    lines = (tmp_path / 'exposures.tsv').read_text().splitlines()
    assert len(lines) == TV + 1 and abs(float(lines[1].split('\t')[1]) - math.exp(theta[0, 0].item())) <= 5.1e-7
    # a checkpoint after epoch 1, resumed by a new Trainer: the bits of the uninterrupted run after epoch 2
    first, _ = _trainer()
    first.run_epoch(shuffle=False)
    ckpt = first.state_dict()
    assert 'exposure' in ckpt and ckpt['exposure']['n_steps'] == 3 and bool(ckpt['exposure']['theta'].any())
    torch.save(ckpt, tmp_path / 'model.pkl')
    resumed, _ = _trainer()
    resumed.load_state_dict(torch.load(tmp_path / 'model.pkl', map_location=DEV, weights_only=False))
    assert resumed.epoch == 2 and torch.equal(resumed.exposure.flat, first.exposure.flat)
    resumed.run_epoch(shuffle=False)
    torch.cuda.synchronize()
    for name in ('flat', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(getattr(resumed.exposure, name), getattr(full.exposure, name)), name
    assert resumed.exposure.n_steps == 6



def test_resume_with_a_moving_model_follows_the_uninterrupted_run():
    """The same resume with the model learning (lr 5e-3, textures 5e-2): the model, its Adam moments and theta are restored together.
    Two runs of a moving model are two samples of a slightly chaotic system (tests/trajectory.py), so the parameters after epoch 2 are
    held to its bound and not to the bit; theta, which moves by at most lr = 1e-2 a step, to the same bound at its own step length."""
    from trajectory import assert_same_trajectory
    full, _ = _trainer(5e-3, 5e-2)
    for _ in range(2):
        full.run_epoch(shuffle=False)
    first, _ = _trainer(5e-3, 5e-2)
    first.run_epoch(shuffle=False)
    ckpt = first.state_dict()
    resumed, _ = _trainer(5e-3, 5e-2)
    resumed.load_state_dict(ckpt)
    assert torch.equal(resumed.step_fn.params.flat, first.step_fn.params.flat) and torch.equal(resumed.step_fn.exp_avg, first.step_fn.exp_avg)
    assert torch.equal(resumed.exposure.flat, first.exposure.flat) and torch.equal(resumed.exposure.exp_avg_sq, first.exposure.exp_avg_sq)
    assert resumed.step_fn.n_steps == first.step_fn.n_steps == 3 and resumed.exposure.n_steps == 3
    moved = float((first.step_fn.params.flat - _trainer(5e-3, 5e-2)[0].step_fn.params.flat).abs().max())
    assert moved > 1e-3                                                                # the model did move in epoch 1
    resumed.run_epoch(shuffle=False)
    torch.cuda.synchronize()
    assert_same_trajectory(resumed.step_fn.params.flat, full.step_fn.params.flat, lr_max=5e-2)
    assert_same_trajectory(resumed.exposure.flat, full.exposure.flat, lr_max=1e-2)
    assert resumed.exposure.n_steps == full.exposure.n_steps == 6 and resumed.step_fn.n_steps == full.step_fn.n_steps == 6
