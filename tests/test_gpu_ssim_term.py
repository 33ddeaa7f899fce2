"""GPU tests of the SSIM term (ops.ssim_term, dbw_monitor_ssim_term, csrc/ssim_term.hip) and of the model that trains with it.

Kernel.  The tile is 16 x 32, so the shapes are (ssim_term_ref.SHAPES): 1x3x5x7 (smaller than the window), 2x3x16x32 (exactly one tile, two
images: the plane index), 1x3x17x33 (one pixel into the next tile both ways), 2x3x19x37 (ragged, W % 4 != 0: element loads), 1x3x48x96 (a
tile with all eight neighbours, W % 4 == 0: 16-byte loads); the inputs seeded noise, rec == target and a nearly black pair on each, and the
constant-block pair of tests/golden/ssim_term.npz.  Oracle: metrics.ssim_map(padding=True) in float64 under autograd on the CPU; bar
(ssim_term_ref.bars): at most 4 x the error of torch's fp32 evaluation of the same input, floors 1e-6 relative (value) and
1e-6 * max(max|g64|, 1/M) (gradient).  Both errors are printed per case (profiles/ssim_term.md keeps a copy).  The gradient is the host
build's (tests/host_ssim_term.cpp) bit for bit.

Properties: two calls give the same bits; a null gradient gives the same value bits; inputs 4 bytes off the 16-byte grid (the element-load
instantiations) give the bits of the aligned call, for the plain and for the masked entry point; the Function's backward scales by the
incoming scalar;
imgs gets no gradient; the value is 1 - image_scores(padding=True) within 1e-6; what the kernel does not take goes through the torch formula.

Model (the geometry of smoke(): 2 views of 32 x 48, 3 blocks, 4 faces per pixel, perceptual_name: ssim, perceptual_weight: 0.1): the loss
dict's `perceptual` is weight x phase factor x the float64 term of the image the model rendered; one autograd step gives the parameter
gradients of the same model with the torch-formula term installed by set_perceptual (1e-4 of the largest element, smoke()'s tolerance); the
one-call C step accepts the model and three of its steps agree with three steps under the torch-formula term as tests/trajectory.py allows
two runs of one optimisation; quantitative_eval reports LPIPS as NaN and a finite L_rec."""
import math

import numpy as np
import pytest
import torch

import masked_loss_ref as MR
import oracle as O
import ssim_term_ref as TR
import dbw_amd
from dbw_amd import metrics, ops
from dbw_amd.parallel import ShardedTrainStep
from trajectory import assert_same_trajectory

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IDS = [TR.case_id(c) for c in TR.CASES]


def _torch_term(imgs, rec):
    return (1 - metrics.ssim_map(imgs, rec, padding=True)).mean()


@pytest.mark.parametrize('kind,shape', TR.CASES, ids=IDS)
def test_value_and_gradient_against_fp64(kind, shape):
    c = TR.case(kind, shape)
    a, b = c['a'].to(DEV), c['b'].to(DEV)
    value, grad = ops.ssim_term_value_grad(a, b)
    value2, grad2 = ops.ssim_term_value_grad(a, b)
    value0, none = ops.ssim_term_value_grad(a, b, with_grad=False)
    torch.cuda.synchronize()
    TR.check(f'kernel {TR.case_id((kind, shape))}', c, value.item(), grad)
    assert torch.equal(value, value2) and torch.equal(grad, grad2)                    # two calls: the same bits
    assert none is None and torch.equal(value0, value)                                # a null gradient: the same value bits
    _, host_grad, _ = TR.term_host(c['a'], c['b'])
    assert torch.equal(grad.cpu(), host_grad)                                         # the host build of the same header, bit for bit
    mse, s = ops.image_scores(a, b, padding=True)
    assert abs(value.item() - (1 - s.mean().item())) < 1e-6
    if kind == 'equal':
        assert value.item() == 0.0 and not grad.any()


@pytest.mark.parametrize('shape', [(2, 16, 32), (1, 48, 96)], ids=lambda s: f'{s[0]}x3x{s[1]}x{s[2]}')
def test_element_loads_give_the_bits_of_16_byte_loads(shape):
    """W % 4 == 0: the aligned call takes the 16-byte loads, the same images 4 bytes off the grid the element loads.  The same tiles, the
    same operations in the same order: the same gradient and value bits, with and without a gradient, plain and under a mask."""
    a, b = (t.to(DEV) for t in TR.pair('noise', shape))
    m = MR.mask('fraction', shape).to(DEV)
    count = MR.count_of(m)
    pad = lambda t: torch.cat([t.new_zeros(1), t.flatten()])[1:].view(t.shape)
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0 and m.data_ptr() % 16 == 0 and pad(b).data_ptr() % 16 == 4
    terms = {'plain': lambda a, b, m, **k: ops.ssim_term_value_grad(a, b, **k),
             'masked': lambda a, b, m, **k: ops.masked_ssim_term_value_grad(a, b, m, count, **k)}
    for name, term in terms.items():
        value, grad = term(a, b, m)
        moved = [(pad(a), b, m), (a, pad(b), m)] + ([(a, b, pad(m))] if name == 'masked' else [])
        for args in moved:
            value_e, grad_e = term(*args)
            value_e0, none = term(*args, with_grad=False)
            assert torch.equal(grad_e, grad) and torch.equal(value_e, value), name
            assert none is None and torch.equal(value_e0, value), name


def test_golden_fixture(golden_dir):
    for name, a, b, ref_v, ref_g in TR.fixture_pairs(golden_dir):
        value, grad = ops.ssim_term_value_grad(a.to(DEV), b.to(DEV))
        TR.fixture_check(f'kernel, {name}', a, b, ref_v, ref_g, value.item(), grad)


def test_function_scales_its_gradient_and_leaves_imgs_alone():
    c = TR.case('noise', (2, 19, 37))
    a, b = c['a'].to(DEV), c['b'].to(DEV)
    _, grad = ops.ssim_term_value_grad(a, b)
    rec = b.clone().requires_grad_(True)
    term = ops.ssim_term(a, rec)
    assert term.dim() == 0 and term.dtype == torch.float32 and term.device == rec.device and term.grad_fn is not None
    (3 * term).backward()
    assert torch.equal(rec.grad, grad * 3) and a.grad is None
    imgs = a.clone().requires_grad_(True)                                              # the Function itself has no gradient for imgs
    rec2 = b.clone().requires_grad_(True)
    ops._SsimTerm.apply(imgs, rec2).backward()
    assert imgs.grad is None and torch.equal(rec2.grad, grad)
    with torch.no_grad():                                                              # evaluation: the value alone, the same bits
        assert torch.equal(ops.ssim_term(a, b), term.detach())
    assert metrics.SSIMTerm()(a, b).item() == term.item()


def test_what_the_kernel_does_not_take_goes_through_the_torch_formula():
    c = TR.case('noise', (2, 19, 37))
    a, b = c['a'].to(DEV), c['b'].to(DEV)
    want = ops.ssim_term(a, b).item()
    wide = torch.zeros(2, 3, 19, 40, device=DEV)
    wide[..., :37] = b
    strided = wide[..., :37].requires_grad_(True)                                      # strides
    v = ops.ssim_term(a, strided)
    g, = torch.autograd.grad(v, strided)
    # (a routing test: the fp32 formula through the GPU's convolutions, 1e-4 of the largest element on noise)
    assert abs(v.item() - want) < 1e-5 and (g.cpu().double() - c['g64']).abs().max().item() < 1e-4 * c['g64'].abs().max().item()
    assert abs(ops.ssim_term(a.double(), b.double()).item() - c['v64']) < 1e-12        # another dtype
    imgs = a.clone().requires_grad_(True)                                              # imgs that requires a gradient gets one
    ops.ssim_term(imgs, b).backward()
    assert imgs.grad is not None and imgs.grad.abs().max() > 0
    with pytest.raises(ValueError):
        ops.ssim_term(a, b[:, :, :-1])


# ---------------------------------------------------------------------------------------------------------------- the model
H, W, NB, TS, FPP = 32, 48, 3, 16, 4
WEIGHT = 0.1


def _cfg(name='ssim'):
    return {'model': {'name': 'dbw', 'mesh': {'n_blocks': NB, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': TS},
                      'renderer': {'faces_per_pixel': FPP, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                      'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True,
                                     'opacity_noise': False},
                      'loss': {'rgb_weight': 1, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1, 'perceptual_weight': WEIGHT,
                               'perceptual_name': name}}}


def _model(name='ssim'):
    torch.manual_seed(227391)
    model = dbw_amd.create_model(_cfg(name), (H, W)).to(DEV).train()
    model._overlap_u_override = torch.rand(NB, 1000, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    return model


@pytest.fixture(scope='module')
def inp():
    R, T, Km = O.synthetic_cameras(2, R_world=O.world_rotation(115, 0, 0))
    imgs = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(0))
    return {k: v.to(DEV) for k, v in dict(imgs=imgs, R=R, T=T, K=Km).items()}


def test_model_loss_and_gradients(inp, monkeypatch):
    model = _model()
    assert isinstance(model.perceptual_fn, metrics.SSIMTerm)
    seen, calls, kernel = [], [], ops.ssim_term_value_grad
    monkeypatch.setattr(ops, 'ssim_term_value_grad', lambda *a, **k: calls.append(k) or kernel(*a, **k))
    model.perceptual_fn.register_forward_hook(lambda mod, args, out: seen.append(args[1].detach().clone()))
    out = model(inp)
    out['total'].backward()
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0].shape == inp['imgs'].shape
    assert calls == [{'with_grad': True}]                                              # the model's image went to the kernel, once
    # the float64 term of the image the model rendered, and torch's fp32 evaluation of it for the bar
    a, rec = inp['imgs'].cpu(), seen[0].cpu()
    v64, g64 = TR.term_torch(a, rec, torch.float64)
    v32, g32 = TR.term_torch(a, rec, torch.float32)
    bar = TR.bars(v64.item(), g64, v32.double().item(), g32)
    from dbw_amd import phase
    factor = phase.phase_of(model, True).perceptual_factor
    got = out['perceptual'].item() / (WEIGHT * factor)
    print(f"model: perceptual {out['perceptual'].item():.8f} = {WEIGHT} x {factor} x {got:.8f}; float64 term {v64.item():.8f}, "
          f"error {abs(got - v64.item()):.3e} (torch fp32 {bar['torch_err_v']:.3e}, bar {bar['tol_v']:.3e})")
    assert math.isfinite(got) and abs(got - v64.item()) <= bar['tol_v']
    # the same step with the torch-formula term installed by set_perceptual
    ref = _model('lpips')
    assert ref.perceptual_fn is None
    ref.set_perceptual(_torch_term)
    ref_out = ref(inp)
    ref_out['total'].backward()
    torch.cuda.synchronize()
    assert abs(out['total'].item() - ref_out['total'].item()) <= 1e-4 * abs(ref_out['total'].item())
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert (p.grad is None) == (q.grad is None), n
        if p.grad is None:
            continue
        e = float((p.grad - q.grad).abs().max() / q.grad.abs().max().clamp(min=1e-12))
        assert e < 1e-4, f'grad {n}: rel err {e}'


def test_c_step_accepts_the_model(inp):
    flats = []
    for name in ('ssim', 'lpips'):
        model = _model(name)
        if name == 'lpips':
            model.set_perceptual(_torch_term)
        model.sync_free = True
        step = ShardedTrainStep(model, lr=5e-3, lr_texture=5e-2, seed=99)
        assert step.cstep is not None and step.cstep.supported(), 'the one-call C step refused the model'
        for k in range(3):
            out = step(inp)
            torch.cuda.synchronize()
            vals = {k_: float(v) for k_, v in out.items()}
            assert all(math.isfinite(v) for v in vals.values()) and vals['perceptual'] > 0
        assert step.cstep.sync_timeouts() == 0
        flats.append((step.params.flat.clone(), vals))
    assert abs(flats[0][1]['total'] - flats[1][1]['total']) <= 1e-3 * abs(flats[1][1]['total'])
    assert_same_trajectory(flats[0][0], flats[1][0])


def test_quantitative_eval_keeps_lpips_nan(inp):
    model = _model()
    res = model.quantitative_eval([(inp, {})], DEV)
    assert np.isnan(res['LPIPS']) and math.isfinite(res['L_rec']) and math.isfinite(res['L_tot']) and res['L_rec'] > 0
    assert math.isfinite(res['SSIM']) and math.isfinite(res['PSNR'])
    plain = _model('lpips')
    plain.loss_weights.pop('perceptual')                                               # the same model without the term: a smaller L_rec
    res0 = plain.quantitative_eval([(inp, {})], DEV)
    assert res['L_rec'] > res0['L_rec'] and abs(res['SSIM'] - res0['SSIM']) < 1e-5 and abs(res['PSNR'] - res0['PSNR']) < 1e-3
    assert model.training
