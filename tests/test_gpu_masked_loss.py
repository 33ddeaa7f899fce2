"""GPU tests of the masked image terms: dbw_monitor_masked_composite and dbw_monitor_masked_ssim_term
(csrc/masked_loss.hip, csrc/ssim_term.hip) and the model, the step and the trainer with a batch that carries masks.

Kernels.  The cases of tests/test_host_masked_loss.py -- ssim_term_ref.SHAPES x {noise, equal, black} x the masks {ones, holes, fraction,
ring, empty}; for the composite the same masks on the same shapes and on 3x40x100, where more than one workgroup feeds the fixed-order sum
-- held to the same float64 oracles and bars (tests/masked_loss_ref.py).  The gradients and rec are the host build's bit for bit; two
calls give the same bits; with a mask of ones the SSIM gradient is ops.ssim_term_value_grad's bit for bit (the value too: the same tiles,
the same order); what rec and imgs hold where m = 0 changes no bit; an empty mask gives 0 and 0.  The composite's one-launch backward
scales by the incoming scalar, with and without a gradient sent to rec.

Model (the geometry of smoke(): 2 views of 32 x 48, 3 blocks, 4 faces per pixel, perceptual_name: ssim, weight 0.1; masks with a
rectangular hole and a lens-like border): `rgb` and `perceptual` of the loss dict equal the float64 formulas evaluated on the image the
model rendered (1e-5 relative); one autograd step gives the parameter gradients of the same model with both terms restated in torch on
render_layers' output (1e-4 of the largest element, smoke()'s tolerance); repainting the targets inside the invalid region changes no bit
of `rgb`, `perceptual`, the rendered image or the gradients the two terms send into the layers (the regularisers' kernels and the render
backward behind the layers add with float atomics: two runs on identical inputs differ in their last bits, tests/trajectory.py, so the
other losses are held to 1e-6 relative and the parameter gradients to 1e-4 of the largest element instead); all-ones masks give the
losses and gradients of the same model stepped without masks through ShardedTrainStep(use_c_step=False, use_native=False); a batch with
masks reaches neither the C step nor the native step; three Trainer epochs with masks run and the loss falls."""
import math

import pytest
import torch

import masked_loss_ref as MR
import oracle as O
import dbw_amd
from dbw_amd import metrics, ops, phase
from dbw_amd.parallel import ShardedTrainStep
from dbw_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize('kind,mkind,shape', MR.CASES, ids=[MR.case_id(c) for c in MR.CASES])
def test_ssim_term_kernel(kind, mkind, shape):
    c = MR.case(kind, mkind, shape)
    a, b, m = c['a'].to(DEV), c['b'].to(DEV), c['m'].to(DEV)
    value, grad = ops.masked_ssim_term_value_grad(a, b, m, c['count'])
    value2, grad2 = ops.masked_ssim_term_value_grad(a, b, m, c['count'])
    value0, none = ops.masked_ssim_term_value_grad(a, b, m, c['count'], with_grad=False)
    torch.cuda.synchronize()
    MR.check(f'kernel {MR.case_id((kind, mkind, shape))}', c, value.item(), grad)
    assert torch.equal(value, value2) and torch.equal(grad, grad2)                    # two calls: the same bits
    assert none is None and torch.equal(value0, value)                                # a null gradient: the same value bits
    _, host_grad = MR.term_host(c['a'], c['b'], c['m'])
    assert torch.equal(grad.cpu(), host_grad)                                         # the host build of the same headers, bit for bit
    assert not grad[(m == 0).expand_as(grad)].any()
    value_r, grad_r = ops.masked_ssim_term_value_grad(MR.repaint(a, m, 1), MR.repaint(b, m, 2), m, c['count'])
    assert torch.equal(value_r, value) and torch.equal(grad_r, grad)                  # invalid content reaches nothing
    if mkind == 'empty':
        assert value.item() == 0.0 and not grad.any()
    if mkind == 'ones':
        plain_v, plain_g = ops.ssim_term_value_grad(a, b)
        assert torch.equal(grad, plain_g) and torch.equal(value, plain_v)
    if kind == 'equal':
        assert value.item() == 0.0 and not grad.any()


def test_ssim_term_function_and_routing():
    c = MR.case('noise', 'holes', (2, 19, 37))
    a, b, m = c['a'].to(DEV), c['b'].to(DEV), c['m'].to(DEV)
    _, grad = ops.masked_ssim_term_value_grad(a, b, m, c['count'])
    rec = b.clone().requires_grad_(True)
    term = ops.ssim_term(a, rec, masks=m, count=c['count'])
    assert term.dim() == 0 and term.dtype == torch.float32 and term.grad_fn is not None
    (3 * term).backward()
    assert torch.equal(rec.grad, grad * 3)
    assert torch.equal(ops.ssim_term(a, b, masks=m), term.detach())                   # count=None: one host read, the same number
    assert metrics.SSIMTerm()(a, b, masks=m, count=c['count']).item() == term.item()
    v = ops.ssim_term(a.double(), b.double(), masks=m.double(), count=c['count'])     # another dtype: the torch formula
    assert abs(v.item() - c['v64']) < 1e-12
    plain = ops.ssim_term(a, b)                                                       # no masks: the plain kernel, as before
    assert torch.equal(plain, ops.ssim_term_value_grad(a, b, with_grad=False)[0][0].float())


COMP_IDS = [f'{m}_{s[0]}x{s[1]}x{s[2]}' for m, s in MR.COMPOSITE_CASES]


@pytest.mark.parametrize('mkind,shape', MR.COMPOSITE_CASES, ids=COMP_IDS)
def test_composite_kernel(mkind, shape):
    c = MR.composite_case(mkind, shape)
    fg, env, imgs, m, x = (c[k].to(DEV) for k in ('fg', 'env', 'imgs', 'm', 'x'))
    up = torch.tensor([MR.UPSTREAM], dtype=torch.float32, device=DEV)
    value, rec, _ = ops.masked_composite_fwd(fg, env, imgs, m, c['scale'])
    value2, rec2, _ = ops.masked_composite_fwd(fg, env, imgs, m, c['scale'])
    assert torch.equal(value, value2) and torch.equal(rec, rec2)                       # two calls: the same bits
    for extra in (False, True):
        gfg, genv = ops.masked_composite_bwd(fg, env, imgs, m, c['scale'], up, x if extra else None)
        torch.cuda.synchronize()
        MR.composite_check(f'kernel composite {mkind} {shape} extra={extra}', c, extra, rec, value.item(), gfg, genv)
        h_rec, h_value, h_gfg, h_genv = MR.composite_host(c, extra)
        assert torch.equal(rec.cpu(), h_rec) and torch.equal(gfg.cpu(), h_gfg) and torch.equal(genv.cpu(), h_genv)
        assert abs(value.item() - h_value) <= 1e-12 * max(abs(h_value), 1e-30)         # (another order of the same fp64 additions)
    imgs_r = MR.repaint(imgs, m, 5)                                                    # the target of an invalid pixel reaches nothing
    value_r, rec_r, _ = ops.masked_composite_fwd(fg, env, imgs_r, m, c['scale'])
    gfg_r, genv_r = ops.masked_composite_bwd(fg, env, imgs_r, m, c['scale'], up, x)
    assert torch.equal(value_r, value) and torch.equal(rec_r, rec) and torch.equal(gfg_r, gfg) and torch.equal(genv_r, genv)
    if mkind == 'empty':
        assert value.item() == 0.0
    # the same through element loads: pointers off the 16-byte grid
    pad = lambda t: torch.cat([t.new_zeros(1), t.flatten()])[1:].view(t.shape)
    value_e, rec_e, _ = ops.masked_composite_fwd(pad(fg), env, imgs, m, c['scale'])
    gfg_e, genv_e = ops.masked_composite_bwd(pad(fg), env, imgs, m, c['scale'], up, x)
    assert torch.equal(rec_e, rec) and torch.equal(gfg_e, gfg) and torch.equal(genv_e, genv)
    assert abs(value_e.item() - value.item()) <= 1e-12 * max(abs(value.item()), 1e-30)


def test_composite_function_backward_is_one_launch_fed_by_both_gradients(monkeypatch):
    c = MR.composite_case('holes', (2, 19, 37))
    fg, env, imgs, m, x = (c[k].to(DEV) for k in ('fg', 'env', 'imgs', 'm', 'x'))
    up = lambda s: torch.tensor([s], dtype=torch.float32, device=DEV)
    g1, e1 = ops.masked_composite_bwd(fg, env, imgs, m, c['scale'], up(1.0))
    g2, e2 = ops.masked_composite_bwd(fg, env, imgs, m, c['scale'], up(2.0))
    assert torch.equal(g2, 2 * g1) and torch.equal(e2, 2 * e1)                          # scales by the incoming scalar (a power of two: exact)
    g1x, e1x = ops.masked_composite_bwd(fg, env, imgs, m, c['scale'], up(1.0), x)
    g0x, e0x = ops.masked_composite_bwd(fg, env, imgs, m, c['scale'], up(0.0), x)
    assert torch.equal(g0x[:, :3], x * fg[:, 3:4]) and (g1x - g1 - g0x).abs().max() <= 1e-6 * g1x.abs().max()
    calls, call = [], ops._lib.call
    monkeypatch.setattr(ops._lib, 'call', lambda name, *a: calls.append(name) or call(name, *a))
    f, e = fg.clone().requires_grad_(True), env.clone().requires_grad_(True)
    value, rec = ops.composite_mse_masked(f, e, imgs, m, MR.WEIGHT, c['count'])
    assert value.dim() == 0 and value.dtype == torch.float32 and rec.shape == imgs.shape
    n_fwd = len(calls)
    (MR.UPSTREAM * value + (x * rec).sum()).backward()
    assert calls[n_fwd:] == ['dbw_monitor_masked_composite']                            # ONE launch for both incoming gradients
    want_g, want_e = ops.masked_composite_bwd(fg, env, imgs, m, c['scale'], up(MR.UPSTREAM), x)
    assert torch.equal(f.grad, want_g) and torch.equal(e.grad, want_e)
    f.grad = e.grad = None                                                              # only rec is used downstream: the scalar's gradient is 0
    value, rec = ops.composite_mse_masked(f, e, imgs, m, MR.WEIGHT, c['count'])
    (x * rec).sum().backward()
    assert torch.equal(f.grad, g0x) and torch.equal(e.grad, e0x)
    value, rec = ops.composite_mse_masked(fg, env, imgs, torch.zeros_like(m), MR.WEIGHT, 0.0)      # count == 0: nothing is divided
    assert value.item() == 0.0 and bool(torch.isfinite(rec).all())


# ---------------------------------------------------------------------------------------------------------------- the model
H, W, NB, TS, FPP = 32, 48, 3, 16, 4
WEIGHT = 0.1


def _cfg(perceptual=True):
    term = {'perceptual_weight': WEIGHT, 'perceptual_name': 'ssim'} if perceptual else {}
    return {'model': {'name': 'dbw', 'mesh': {'n_blocks': NB, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': TS},
                      'renderer': {'faces_per_pixel': FPP, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                      'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True,
                                     'opacity_noise': False},
                      'loss': dict({'rgb_weight': 1, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}, **term)}}


def _model(perceptual=True):
    torch.manual_seed(227391)
    model = dbw_amd.create_model(_cfg(perceptual), (H, W)).to(DEV).train()
    model._overlap_u_override = torch.rand(NB, 1000, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    return model


def _masks():
    """(2,1,H,W): a lens-like border on both views, a rectangular hole in each (another one per view)."""
    m = MR.mask('ring', (2, H, W)).clone()
    m[0, :, 8:17, 20:33] = 0
    m[1, :, 15:25, 5:16] = 0
    return m


@pytest.fixture(scope='module')
def inp():
    R, T, Km = O.synthetic_cameras(2, R_world=O.world_rotation(115, 0, 0))
    imgs = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(0))
    return {k: v.to(DEV) for k, v in dict(imgs=imgs, R=R, T=T, K=Km, masks=_masks()).items()}


def _run(model, batch):
    """One forward + backward of the model itself -> (losses, the image it rendered, the gradients that reached the layers)."""
    seen, layers, composite = [], [], ops.composite_mse_masked

    def spy(fg, env, *a):
        fg.retain_grad(), env.retain_grad()
        layers.extend([fg, env])
        return composite(fg, env, *a)
    ops.composite_mse_masked = spy
    hook = model.perceptual_fn.register_forward_hook(lambda mod, args, out: seen.append(args[1].detach().clone()))
    try:
        out = model(batch)
        out['total'].backward()
        torch.cuda.synchronize()
    finally:
        ops.composite_mse_masked = composite
        hook.remove()
    assert len(seen) == 1 and len(layers) == 2
    return out, seen[0], [t.grad.clone() for t in layers]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


def test_model_losses_and_gradients(inp):
    model = _model()
    out, rec, _ = _run(model, inp)
    imgs, m = inp['imgs'].cpu().double(), inp['masks'].cpu().double()
    count = 3 * m.sum().item()
    factor = phase.phase_of(model, True).perceptual_factor
    rgb64 = (m * (rec.cpu().double() - imgs) ** 2).sum().item() / count
    per64 = WEIGHT * factor * MR.term_torch(imgs, rec.cpu(), m, torch.float64)[0].item()
    print(f"model: rgb {out['rgb'].item():.9f} (float64 {rgb64:.9f}), perceptual {out['perceptual'].item():.9f} (float64 {per64:.9f})")
    assert abs(out['rgb'].item() - rgb64) <= 1e-5 * rgb64 and abs(out['perceptual'].item() - per64) <= 1e-5 * per64
    assert abs(out['total'].item() - sum(out[k].item() for k in out if k != 'total')) <= 1e-5 * out['total'].item()
    # the same model with both terms restated in torch on render_layers' output
    ref = _model()
    ref.loss_weights.pop('perceptual')
    batch = {k: v for k, v in inp.items() if k != 'masks'}
    fg, env = ref.render_layers(batch)
    regs = ref.compute_losses(batch['imgs'], None, layers=None, rgb_value=torch.zeros((), device=DEV))['total']
    r = fg[:, :3] * fg[:, 3:4] + (1 - fg[:, 3:4]) * env[:, :3]
    mk = inp['masks']
    s = metrics.ssim_map(batch['imgs'] * mk, r * mk, padding=True)
    total = regs + (mk * (r - batch['imgs']) ** 2).sum() / count + WEIGHT * factor * ((1 - s) * mk).sum() / count
    total.backward()
    torch.cuda.synchronize()
    assert abs(out['total'].item() - total.item()) <= 1e-4 * abs(total.item())
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert (p.grad is None) == (q.grad is None), n
        if p.grad is not None:
            assert _rel(p.grad, q.grad) < 1e-4, f'grad {n}: rel err {_rel(p.grad, q.grad)}'


def test_repainting_invalid_targets_changes_no_bit(inp):
    out, rec, layer_grads = _run(_model(), inp)
    painted = dict(inp, imgs=MR.repaint(inp['imgs'], inp['masks'], 9))
    assert not torch.equal(painted['imgs'], inp['imgs'])
    model = _model()
    out_p, rec_p, layer_grads_p = _run(model, painted)
    assert torch.equal(rec_p, rec)
    for k in ('rgb', 'perceptual'):                                                    # the two terms the targets enter
        assert torch.equal(out_p[k], out[k]), k
    for k in out:                                                                      # (the regularisers never see a target; their kernels add
        assert abs(out_p[k].item() - out[k].item()) <= 1e-6 * abs(out[k].item()), k    # with float atomics: the last bits move from run to run)
    for g, gp in zip(layer_grads, layer_grads_p):
        assert torch.equal(gp, g)
    ref = _model()
    ref(inp)['total'].backward()
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        if p.grad is not None:
            assert _rel(p.grad, q.grad) < 1e-4, n


def test_all_ones_masks_are_the_unmasked_step(inp):
    res = []
    for masked in (True, False):
        model = _model()
        model.sync_free = True
        step = ShardedTrainStep(model, lr=0.0, lr_texture=0.0, seed=1, use_c_step=False, use_native=False)
        batch = {k: v for k, v in inp.items() if k != 'masks'}
        if masked:
            batch['masks'] = torch.ones_like(inp['masks'])
        losses = step(batch)
        torch.cuda.synchronize()
        res.append(({k: float(v) for k, v in losses.items()}, step.params.grad.clone(), step.params.names))
    (lm, gm, names), (lu, gu, _) = res
    for k in lu:
        assert abs(lm[k] - lu[k]) <= 1e-5 * abs(lu[k]), (k, lm[k], lu[k])
    for name, off, n in names:
        assert _rel(gm[off:off + n], gu[off:off + n]) < 1e-4, name


def test_masked_batch_reaches_neither_the_c_step_nor_the_native_step(inp, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('a batch with masks reached a step without them')
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
        losses = step(dict(inp, mask_sum=float(inp['masks'].sum())))
        torch.cuda.synchronize()
        assert all(math.isfinite(float(v)) for v in losses.values()) and float(losses['rgb']) > 0 and step.n_steps == 1
        assert ('perceptual' in losses) == perceptual
    step.world_size = 2
    with pytest.raises(NotImplementedError, match='valid count'):
        step(inp)


def test_trainer_runs_with_masks_and_the_loss_falls(inp, monkeypatch):
    model = _model()
    cfg = {'training': {'batch_size': 2, 'n_epoches': 3, 'seed': 3, 'optimizer': {'name': 'adam', 'lr': 5e-3, 'texture': {'lr': 5e-2}},
                        'scheduler': {'name': 'multi_step'}}}
    tr = Trainer(cfg, model, dict(inp))
    want = inp['masks'].double().flatten(1).sum(1).cpu()
    assert torch.equal(tr.mask_sums, want)
    seen, step = [], tr.step_fn.__call__
    monkeypatch.setattr(type(tr.step_fn), '__call__', lambda self, batch, **k: seen.append(batch) or step(batch, **k))
    totals = [float(tr.run_epoch()['total']) for _ in range(3)]
    torch.cuda.synchronize()
    assert len(seen) == 3 and all('masks' in b and b['mask_sum'] == float(want.sum()) for b in seen)
    print('trainer with masks, total per epoch:', totals)
    assert all(math.isfinite(t) for t in totals) and totals[2] < totals[0]
