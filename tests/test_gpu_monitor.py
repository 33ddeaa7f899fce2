"""GPU tests of the run monitor's kernels (csrc/run_monitor.hip, include/dbw_monitor.h).

dbw_image_scores: the SSIM map equals the HOST build of the same header (tests/host_score_math.cpp, which tests/test_host_score_math.py
holds to the reference's golden map and to an fp64 arbiter) bit for bit -- every fp32 operation rounds once, in one order, on both sides
-- for both paddings, N = 1 and N = 3, shapes with one window, one tile, several tiles, ragged tiles, interior tiles of the
16-byte path ((20,100): three and four tiles along x), a W that is no multiple of 4 and a view off its 16-byte alignment (the scalar
path).  The two sums are fp64 sums of fp64 terms in another order than numpy's: 1e-12 relative.
Two calls give the same bits.

dbw_meter_add / dbw_meter_reset: the table equals numpy's sequential fp64 accumulation bit for bit; the first step with a value that is
not finite stays in the flag; the loss scalars of a real C step accumulate to what StepLosses.host() reads."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle as O                                              # noqa: E402  (checker only)
import dbw_amd                                                  # noqa: E402
import score_ref as SR                                          # noqa: E402
from dbw_amd import _lib, ops                                   # noqa: E402
from dbw_amd.parallel import ShardedTrainStep                   # noqa: E402
from dbw_amd.runlog import DeviceMeter                          # noqa: E402

DEV = 'cuda:0'
CASES = [f'noise_{h}x{w}' for h, w in SR.NOISE_SHAPES] + ['render', 'noise_40x52', 'noise_20x100']      # (20,100): 3 / 4 tiles along x on the 16-byte path


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _check(c, a, b, pad, N):
    out, m = ops.image_score_sums(a, b, padding=bool(pad), return_map=True)
    want_map, want_out = c[f'host_map{pad}'], c[f'host_out{pad}']
    assert m.shape == want_map.shape and out.shape == (N, 2) and out.dtype == torch.float64
    bad = int((_bits(m) != _bits(want_map)).sum())
    assert bad == 0, f'{bad} of {m.numel()} pixels differ from the host build, max {float((m.cpu() - want_map).abs().max()):.3e}'
    out = out.cpu().numpy()
    ss = m.cpu().numpy().astype(np.float64).reshape(N, -1).sum(1)
    se = ((c['a'].numpy().astype(np.float64) - c['b'].numpy().astype(np.float64)) ** 2).reshape(N, -1).sum(1)
    e_ss, e_se = np.abs(out[:, 1] / ss - 1).max(), np.abs(out[:, 0] / se - 1).max()
    print(f'padding {pad}, N {N}: sum ssim rel {e_ss:.2e}, sum sq err rel {e_se:.2e}')
    assert e_ss < 1e-12 and e_se < 1e-12
    assert np.abs(out[:, 0] / want_out[:, 0].numpy() - 1).max() < 1e-12
    again = ops.image_score_sums(a, b, padding=bool(pad))
    assert np.array_equal(again.cpu().numpy().view(np.int64), out.view(np.int64))          # the same bits
    return out


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('name', CASES)
def test_map_equals_the_host_build_bit_for_bit_and_the_sums_are_its_sums(name, N):
    c = SR.case(name, N)
    a, b = c['a'].to(DEV), c['b'].to(DEV)
    for pad in (0, 1):
        _check(c, a, b, pad, N)


def test_an_unaligned_view_takes_the_scalar_path_with_the_same_bits():
    """(12,16) and (48,64): W a multiple of 4, the tensors one float off a 16-byte boundary."""
    for name in ('noise_12x16', 'render'):
        c = SR.case(name, 3)
        n = c['a'].numel()
        bufs = [torch.empty(n + 1, device=DEV) for _ in range(2)]
        a, b = [buf[1:].view(c['a'].shape).copy_(c[k]) for buf, k in zip(bufs, 'ab')]
        assert a.data_ptr() % 16 == 4 and a.is_contiguous()
        for pad in (0, 1):
            unaligned = _check(c, a, b, pad, 3)
            aligned = ops.image_score_sums(c['a'].to(DEV), c['b'].to(DEV), padding=bool(pad)).cpu().numpy()
            assert np.array_equal(unaligned[:, 1].view(np.int64), aligned[:, 1].view(np.int64))   # (the SSIM sums: same tiles, same order)


def test_image_scores_are_the_means_and_refuse_what_has_no_window():
    c = SR.case('noise_40x52', 3)
    a, b = c['a'].to(DEV), c['b'].to(DEV)
    mse, ssim = ops.image_scores(a, b)
    out = c['host_out0']
    assert mse.is_cuda and mse.dtype == ssim.dtype == torch.float64
    assert torch.allclose(mse.cpu(), out[:, 0] / (3 * 40 * 52), rtol=1e-12) and torch.allclose(ssim.cpu(), out[:, 1] / (3 * 30 * 42), rtol=1e-12)
    cm, cs = ops.image_scores(c['a'], c['b'])                  # CPU tensors: metrics.ssim_map
    assert torch.allclose(cm, mse.cpu(), rtol=1e-12) and torch.allclose(cs, ssim.cpu(), atol=1e-6)
    ones = torch.full((2, 3, 20, 24), 0.3, device=DEV)
    _, _, m = ops.image_scores(ones, ones, return_map=True)
    assert torch.equal(m, torch.ones_like(m))
    with pytest.raises(ValueError, match='11 x 11'):
        ops.image_scores(a[:, :, :10].contiguous(), b[:, :, :10].contiguous())
    assert ops.image_scores(a[:, :, :10].contiguous(), b[:, :, :10].contiguous(), padding=True)[0].shape == (3,)
    assert ops.image_scores(a[:0], b[:0])[0].shape == (0,)


# ---- the meter ---------------------------------------------------------------------------------------------------------------------------
def _table(meter):
    return meter.table.cpu().numpy()


def test_meter_equals_numpy_s_sequential_accumulation_bit_for_bit():
    names = ['loss_a', 'loss_b', 'loss_c', 'loss_d', 'loss_total']
    rng = np.random.RandomState(4)
    vals = (rng.randn(50, 5) * np.array([1.0, 1e-3, 30.0, 1e-6, 5.0])).astype(np.float32)
    weights = [4, 4, 3] * 17
    dev = torch.from_numpy(vals).to(DEV)
    meter = DeviceMeter(names, DEV)
    want = np.zeros(7)
    want[6] = -1
    for s in range(50):
        meter.add({k: dev[s, i] for i, k in enumerate(names)}, weights[s], s + 1)
        for i in range(5):
            want[i] += np.float64(vals[s, i]) * np.float64(weights[s])
        want[5] += weights[s]
    assert np.array_equal(_table(meter).view(np.int64), want.view(np.int64))
    avg, bad = meter.read_reset()
    assert bad is None and all(avg[k] == want[i] / want[5] for i, k in enumerate(names))
    assert _table(meter).tolist() == [0.0] * 6 + [-1.0]

    # a NaN at step 17, another and an infinity at step 30: the flag keeps 17
    vals[16, 2], vals[29, 0], vals[29, 4] = np.nan, np.nan, np.inf
    dev = torch.from_numpy(vals).to(DEV)
    for s in range(50):
        meter.add({k: dev[s, i] for i, k in enumerate(names)}, weights[s], s + 1)
        if s == 15:
            assert _table(meter)[6] == -1
    t = _table(meter)
    assert t[6] == 17 and np.isnan(t[0]) and np.isnan(t[2]) and np.isfinite(t[1]) and t[5] == sum(weights[:50])
    avg, bad = meter.read_reset()
    assert bad == 17
    assert _table(meter).tolist() == [0.0] * 6 + [-1.0]
    # one value, sixteen values, and what the binding refuses
    one = DeviceMeter(['x'], DEV)
    one.add({'x': dev[0, 1]}, 2, 5)
    assert _table(one).tolist() == [float(np.float64(vals[0, 1]) * 2), 2.0, -1.0]
    many = DeviceMeter([f'v{i}' for i in range(16)], DEV)
    many.add({f'v{i}': dev[i % 10, i % 5] for i in range(16)}, 1, 0)
    assert _table(many)[:16].tolist() == [float(vals[i % 10, i % 5]) for i in range(16)] and _table(many)[16] == 1
    with pytest.raises(TypeError):
        one.add({'x': dev[0, 1].double()}, 1, 0)
    with pytest.raises(TypeError):
        one.add({'x': dev[0, 1].cpu()}, 1, 0)
    with pytest.raises(ValueError):
        DeviceMeter([f'v{i}' for i in range(17)], DEV)


def test_meter_accumulates_the_losses_of_a_real_c_step():
    """3 views of 48 x 64, 4 blocks (the smallest geometry of tests/test_gpu_c_step.py): five steps, the meter fed with the StepLosses as the
    recorder feeds it, against the floats StepLosses.host() returns for the same steps."""
    cfg = {'model': {'name': 'dbw', 'mesh': {'n_blocks': 4, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': 32},
                     'renderer': {'faces_per_pixel': 6, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                     'rend_optim': {'coarse_learning': 1500, 'decimate_txt': 750, 'decimate_factor': 8, 'kill_blocks': True,
                                    'decouple_rendering': True, 'opacity_noise': True},
                     'loss': {'rgb_weight': 1, 'perceptual_weight': 0, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}}}
    torch.manual_seed(227391)
    model = dbw_amd.create_model(cfg, (48, 64)).to(DEV).train()
    model.sync_free = True
    R, T, Km = O.synthetic_cameras(3, R_world=O.world_rotation(115, 0, 0))
    imgs = torch.rand(3, 3, 48, 64, generator=torch.Generator().manual_seed(2))
    inp = {k: v.to(DEV) for k, v in dict(imgs=imgs, R=R, T=T, K=Km).items()}
    step = ShardedTrainStep(model, lr=5e-3, lr_texture=5e-2, seed=7)
    assert step.cstep is not None and step.cstep.supported()
    meter = DeviceMeter(model.loss_names, DEV)
    assert model.loss_names == ['loss_rgb', 'loss_parsimony', 'loss_tv', 'loss_overlap', 'loss_total']
    want = np.zeros(5)
    for s in range(5):
        out = step(inp)
        meter.add({f'loss_{k}': v for k, v in out.items()}, 3, s + 1)
        host = out.host()
        for i, k in enumerate(model.loss_names):
            want[i] += np.float64(np.float32(host[k[5:]])) * 3.0
    t = _table(meter)
    assert np.array_equal(t[:5].view(np.int64), want.view(np.int64)) and t[5] == 15 and t[6] == -1
    avg, bad = meter.read_reset()
    assert bad is None and avg['loss_rgb'] > 0 and abs(avg['loss_total'] - sum(avg[k] for k in model.loss_names[:4])) < 1e-5 * avg['loss_total']
    assert step.cstep.sync_timeouts() == 0
