"""CPU tests of the host side of the exposure compensation: exposure.parse_config, ExposureRefiner on CPU tensors with a
torch Adam standing in through adam_fn (the kernel has no CPU form), the Trainer with and without training.exposure, the command-line
flag, exposures.tsv, and the refusals of ops.composite_mse_exposure and of the step under data parallelism."""
import math

import pytest
import torch

from dbw_amd import exposure, ops
from dbw_amd.parallel import ShardedTrainStep
from dbw_amd.trainer import Trainer
from test_parallel_cpu import ToyModel, torch_adam


def _refiner(n, **kw):
    return exposure.ExposureRefiner(n, 'cpu', adam_fn=torch_adam, **kw)


def test_parse_config_accepts_every_form():
    full = {'lr': 1e-3, 'start_epoch': 0, 'bias': True, 'center': True}
    for off in (None, False):
        assert exposure.parse_config(off) is None
    assert exposure.parse_config(True) == full and exposure.parse_config({}) == full
    assert exposure.parse_config(5e-3) == dict(full, lr=5e-3) and exposure.parse_config(1) == dict(full, lr=1.0)
    assert exposure.parse_config('2e-3') == dict(full, lr=2e-3)                          # (a YAML scalar that arrived as text)
    got = exposure.parse_config({'lr': 2e-2, 'start_epoch': 3, 'bias': False, 'center': False})
    assert got == {'lr': 2e-2, 'start_epoch': 3, 'bias': False, 'center': False}
    assert exposure.parse_config({'start_epoch': 2}) == dict(full, start_epoch=2)
    assert isinstance(got['lr'], float) and isinstance(got['start_epoch'], int)


def test_parse_config_refuses():
    with pytest.raises(ValueError, match=r"unknown keys \['learning_rate'\]"):
        exposure.parse_config({'learning_rate': 1.0})
    with pytest.raises(ValueError, match='unknown keys'):
        exposure.parse_config({'lr': 1e-3, 'rot': True})
    for bad in (0, 0.0, -1e-3, float('nan')):
        with pytest.raises(ValueError, match='must be positive'):
            exposure.parse_config({'lr': bad})
    with pytest.raises(ValueError, match='must be positive'):
        exposure.parse_config(-1.0)


def test_refiner_steps_like_dense_adam_and_clears_its_gradient():
    ref = _refiner(4, lr=1e-2, center=False)
    assert ref.theta.shape == (4, 6) and ref.theta.requires_grad and ref.theta.grad.data_ptr() == ref.grad.data_ptr()
    assert ref.theta.data_ptr() == ref.flat.data_ptr() and not ref.flat.any()
    gen = torch.Generator().manual_seed(3)
    for _ in range(3):
        ref.grad.copy_(torch.randn(24, generator=gen))
        ref.step()
        assert not ref.grad.any()
    p = torch.zeros(4, 6, requires_grad=True)
    opt = torch.optim.Adam([p], lr=1e-2)
    gen = torch.Generator().manual_seed(3)
    for _ in range(3):
        p.grad = torch.randn(24, generator=gen).view(4, 6)
        opt.step()
    assert torch.allclose(ref.flat.view(4, 6), p.detach(), rtol=1e-5, atol=1e-8) and ref.n_steps == 3


def test_bias_false_keeps_the_offsets_at_zero():
    for center in (False, True):
        ref = _refiner(5, lr=1e-2, bias=False, center=center)
        gen = torch.Generator().manual_seed(4)
        for _ in range(3):
            ref.grad.copy_(torch.randn(30, generator=gen))
            ref.step()
        t = ref.flat.view(5, 6)
        assert bool(t[:, :3].any()) and not t[:, 3:].any() and not ref.exp_avg.view(5, 6)[:, 3:].any()


def test_centring_zeroes_the_column_means_and_keeps_row_differences():
    gen = torch.Generator().manual_seed(5)
    grads = [torch.randn(30, generator=gen) for _ in range(3)]
    a, b = _refiner(5, lr=1e-2, center=True), _refiner(5, lr=1e-2, center=False)
    for g in grads:
        for r in (a, b):
            r.grad.copy_(g)
            r.step()
    ta, tb = a.flat.view(5, 6), b.flat.view(5, 6)
    assert float(ta.mean(0).abs().max()) <= 1e-8 and float(tb.mean(0).abs().max()) > 1e-4
    # Adam's update does not look at theta: the two tables differ by the means that were taken out, the same for every row
    assert torch.allclose(ta - ta[0:1], tb - tb[0:1], rtol=0, atol=1e-7)
    assert torch.allclose(ta, tb - tb.mean(0, keepdim=True), rtol=0, atol=1e-7)


def test_rows_outside_the_batch_keep_zero_gradient():
    """theta reaches the loss through its batch rows only (a gather stands in for the kernel): the backward accumulates into the flat
    gradient buffer in place, and only the batch's rows of it."""
    ref = _refiner(6, center=False)
    batch = ref.attach({'view_ids': torch.tensor([4, 1]), 'imgs': torch.rand(2, 3, 2, 2)})
    assert batch['exposure'] is ref.theta
    rows = batch['exposure'][batch['view_ids']]
    (rows * torch.arange(1.0, 13.0).view(2, 6)).sum().backward()
    g = ref.grad.view(6, 6)
    assert ref.theta.grad.data_ptr() == ref.grad.data_ptr()                              # still the flat buffer: accumulated in place
    assert torch.equal(g[4], torch.arange(1.0, 7.0)) and torch.equal(g[1], torch.arange(7.0, 13.0)) and not g[[0, 2, 3, 5]].any()
    with pytest.raises(KeyError, match='view_ids'):
        ref.attach({'imgs': torch.rand(2, 3, 2, 2)})


def test_state_dict_round_trip_and_a_state_of_another_size():
    ref = _refiner(5, lr=3e-3, bias=False)
    with torch.no_grad():
        ref.flat.copy_(torch.randn(30))
        ref.exp_avg.copy_(torch.randn(30))
        ref.exp_avg_sq.copy_(torch.rand(30))
    ref.n_steps = 11
    sd = ref.state_dict()
    assert set(sd) >= {'theta', 'exp_avg', 'exp_avg_sq', 'n_steps'} and sd['theta'].data_ptr() != ref.flat.data_ptr()
    other = _refiner(5)
    other.grad.fill_(1.0)
    other.load_state_dict(sd)
    assert torch.equal(other.flat, ref.flat) and torch.equal(other.exp_avg, ref.exp_avg) and torch.equal(other.exp_avg_sq, ref.exp_avg_sq)
    assert other.n_steps == 11 and not other.grad.any() and torch.equal(other.theta, ref.theta)
    with pytest.raises(ValueError, match='a state of 5 views for a refiner of 4'):
        _refiner(4).load_state_dict(sd)


def _cfg(**training):
    return {'training': dict({'batch_size': 2, 'n_epoches': 1, 'seed': 7, 'optimizer': {'name': 'adam', 'lr': 1e-2}}, **training)}


def _views():
    gen = torch.Generator().manual_seed(1)
    return {'imgs': torch.rand(5, 3, 4, 4, generator=gen), 'R': torch.eye(3).expand(5, 3, 3).contiguous(), 'T': torch.randn(5, 3, generator=gen)}


def _spy(tr):
    tr.step_fn.adam_fn = torch_adam
    seen, step = [], tr.run_single_batch_train
    tr.run_single_batch_train = lambda batch, count=None: (seen.append(batch), step(batch, count))[1]
    return seen


def test_trainer_without_the_key_builds_nothing():
    tr = Trainer(_cfg(), ToyModel(), _views())
    assert tr.exposure is None and tr.exposure_cfg is None and tr.view_ids is False and 'exposure' not in tr.state_dict()
    seen = _spy(tr)
    tr.run_epoch(shuffle=False)
    assert len(seen) == 3 and all('exposure' not in b and 'view_ids' not in b and 'view_ids_host' not in b for b in seen)
    for off in (None, False):
        assert Trainer(_cfg(exposure=off), ToyModel(), _views()).exposure is None


class _ExposedToy(ToyModel):
    """ToyModel whose prediction goes through the batch's rows of theta, so that the Trainer's backward reaches the refiner."""

    def forward(self, inp, labels=None):
        out = super().forward(inp, labels)
        if 'exposure' in inp:
            rows = inp['exposure'][inp['view_ids']]
            out['rgb'] = out['rgb'] + ((rows - 0.1) ** 2).sum()
            out['total'] = out['total'] + ((rows - 0.1) ** 2).sum()
        return out


def test_trainer_with_the_key_attaches_steps_saves_and_resumes(tmp_path):
    cfg = _cfg(exposure={'lr': 2e-2, 'start_epoch': 2, 'bias': False}, n_epoches=3)
    tr = Trainer(cfg, _ExposedToy(), _views())
    assert tr.exposure is not None and tr.view_ids and tr.exposure.lr == 2e-2 and not tr.exposure.bias and tr.exposure.center
    assert tr.exposure.n_views == 5 and tr.exposure_cfg['start_epoch'] == 2
    tr.exposure.adam_fn = torch_adam
    seen = _spy(tr)
    tr.run_epoch(shuffle=False)                                                          # epoch 1 < start_epoch: ids ride along, theta does not
    assert all('view_ids' in b and 'view_ids_host' in b and 'exposure' not in b for b in seen)
    assert tr.exposure.n_steps == 0 and not tr.exposure.flat.any()
    del seen[:]
    tr.run_epoch(shuffle=False)                                                          # epoch 2: attached, stepped behind the model
    assert all(b['exposure'] is tr.exposure.theta for b in seen) and tr.exposure.n_steps == 3
    t = tr.exposure.flat.view(5, 6)
    assert bool(t[:, :3].any()) and not t[:, 3:].any() and float(t.mean(0).abs().max()) <= 1e-8 and not tr.exposure.grad.any()
    sd = tr.state_dict()
    assert set(sd['exposure']) >= {'theta', 'exp_avg', 'exp_avg_sq', 'n_steps'} and 'pose_refine' not in sd
    tr2 = Trainer(cfg, _ExposedToy(), _views())
    tr2.load_state_dict(sd)
    assert torch.equal(tr2.exposure.flat, tr.exposure.flat) and torch.equal(tr2.exposure.exp_avg, tr.exposure.exp_avg)
    assert torch.equal(tr2.exposure.exp_avg_sq, tr.exposure.exp_avg_sq) and tr2.exposure.n_steps == 3
    # a checkpoint of a run without the option still loads: theta starts at 0
    tr3 = Trainer(cfg, _ExposedToy(), _views())
    tr3.load_state_dict({k: v for k, v in sd.items() if k != 'exposure'})
    assert not tr3.exposure.flat.any()
    with pytest.raises(ValueError, match='unknown keys'):
        Trainer(_cfg(exposure={'learning_rate': 1.0}), ToyModel(), _views())


class _EvalModel(ToyModel):
    def qualitative_eval(self, loader, device, path=None, **kw):
        self.quali = [sorted(inp) for inp, _ in loader]

    def quantitative_eval(self, loader, device, hard_inference=True):
        self.quanti = [sorted(inp) for inp, _ in loader]
        return {'PSNR': 1.0}


def test_evaluate_writes_exposures_and_renders_uncompensated(tmp_path):
    views = _views()
    tr = Trainer(_cfg(exposure=True), _EvalModel(), views)
    with torch.no_grad():
        tr.exposure.flat.copy_(0.2 * torch.randn(30, generator=torch.Generator().manual_seed(2)))
    loader = [({k: v[a:a + 2] for k, v in views.items()}, {}) for a in range(0, 5, 2)]
    assert tr.evaluate(loader, tmp_path)['PSNR'] == 1.0
    assert all('exposure' not in keys for keys in tr.model.quali + tr.model.quanti)      # canonical exposure: no batch carries theta
    lines = (tmp_path / 'exposures.tsv').read_text().splitlines()
    assert lines[0].split('\t') == ['view', 'gain_r', 'gain_g', 'gain_b', 'bias_r', 'bias_g', 'bias_b'] and len(lines) == 6
    t = tr.exposure.flat.view(5, 6).double()
    for i, line in enumerate(lines[1:]):
        cells = line.split('\t')
        assert cells[0] == str(i)
        want = [math.exp(v) for v in t[i, :3].tolist()] + t[i, 3:].tolist()
        assert all(abs(float(c) - w) <= 5.1e-7 for c, w in zip(cells[1:], want))
    # names, and their number
    path = exposure.write_exposures(tr.exposure, tmp_path, names=[f'frame_{i:03d}.png' for i in range(5)])
    assert [ln.split('\t')[0] for ln in open(path).read().splitlines()[1:]] == [f'frame_{i:03d}.png' for i in range(5)]
    with pytest.raises(ValueError, match='4 names for 5 views'):
        exposure.write_exposures(tr.exposure, tmp_path, names=['a'] * 4)
    plain = Trainer(_cfg(), _EvalModel(), views)
    plain.evaluate(loader, tmp_path / 'plain')
    assert not (tmp_path / 'plain' / 'exposures.tsv').exists()


def test_the_command_line_flag_sets_the_key(tmp_path):
    from dbw_amd import train
    cfg_file = tmp_path / 'c.yml'
    cfg_file.write_text('dataset: {name: custom, tag: x}\nmodel: {loss: {perceptual_weight: 0}}\ntraining: {exposure: {start_epoch: 3}}\n')
    (tmp_path / 'default.yml').write_text('training: {batch_size: 2}\n')
    base = ['-c', str(cfg_file), '-t', 't', '--data-root', 'd', '--runs-root', 'r']
    cfg = train.prepare_config(train.parse_args(base + ['--exposure', '2e-3']))
    assert cfg['training']['exposure'] == {'start_epoch': 3, 'lr': 2e-3} and 'pose_refine' not in cfg['training']
    assert train.prepare_config(train.parse_args(base))['training']['exposure'] == {'start_epoch': 3}
    cfg_file.write_text('dataset: {name: custom, tag: x}\nmodel: {loss: {perceptual_weight: 0}}\ntraining: {exposure: true}\n')
    assert train.prepare_config(train.parse_args(base + ['--exposure', '4e-3']))['training']['exposure'] == {'lr': 4e-3}


def test_the_example_config_parses():
    import os
    from dbw_amd import dataset
    here = os.path.dirname(os.path.abspath(__file__))
    cfg = dataset.load_config(os.path.join(here, '..', 'differentiable-blocksworld_amd', 'configs', 'custom_exposure.yml'))
    assert exposure.parse_config(cfg['training']['exposure']) == {'lr': 1e-3, 'start_epoch': 0, 'bias': True, 'center': True}
    assert cfg['model']['rend_optim']['decouple_rendering'] is True and cfg['dataset']['name'] == 'custom'


def test_ids_are_checked_on_the_host_copy():
    fg, theta = torch.zeros(2, 4, 3, 3), torch.zeros(4, 6)
    args = (fg, fg, torch.zeros(2, 3, 3, 3), None, 1.0, 54.0, theta)
    with pytest.raises(ValueError, match='distinct'):
        ops.composite_mse_exposure(*args, torch.tensor([1, 1]), ids_host=[1, 1])
    with pytest.raises(ValueError, match='outside'):
        ops.composite_mse_exposure(*args, torch.tensor([1, 4]), ids_host=torch.tensor([1, 4]))
    with pytest.raises(ValueError, match='outside'):
        ops.composite_mse_exposure(*args, torch.tensor([-1, 2]), ids_host=[-1, 2])
    with pytest.raises(ValueError, match='one per view'):
        ops.composite_mse_exposure(*args, torch.tensor([1]), ids_host=[1])
    with pytest.raises(ValueError, match='one per view'):
        ops.composite_mse_exposure(*args, torch.tensor([1, 2]), ids_host=[1])


def test_exposure_under_two_ranks_is_refused(monkeypatch):
    step = ShardedTrainStep(_ExposedToy(), adam_fn=torch_adam)
    v = _views()
    batch = {'imgs': v['imgs'], 'R': v['R'], 'T': v['T'], 'exposure': torch.zeros(5, 6, requires_grad=True), 'view_ids': torch.arange(5)}
    step(batch)                                                                          # one rank: the autograd iteration
    assert batch['exposure'].grad is not None
    step.world_size = 2
    with pytest.raises(NotImplementedError, match='exposure'):
        step(batch)
    # ... and the Trainer refuses the key before it builds anything
    import dbw_amd.trainer as T

    class TwoRanks(T.ShardedTrainStep):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.world_size = 2
    monkeypatch.setattr(T, 'ShardedTrainStep', TwoRanks)
    with pytest.raises(NotImplementedError, match='training.exposure under data parallelism'):
        Trainer(_cfg(exposure=True), ToyModel(), _views())
