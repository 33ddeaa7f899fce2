"""CPU tests of the host side of the intrinsics refinement: parse_config's refusals, IntrinsicsRefiner's Adam step with a
shared focal scale and with frozen parts, its state round trip, the refined fl_x, fl_y, cx, cy written back into a capture's own
transforms.json and read again through dataset.CustomScene, the refusal to write them for a capture with lens coefficients, the Trainer with
and without training.intrinsics_refine, and the refusal under data parallelism.  The kernels are not involved: the host build of
csrc/intrinsics_math.h (tests/intrinsics_ref.py), its torch restatement (where a gradient has to flow) and a torch Adam stand in through
IntrinsicsRefiner's adam_fn / apply_fn."""
import json
import os
import shutil

import pytest
import torch
import yaml

import intrinsics_ref as IR
import lens_ref as LR
from custom_fixture import write_capture
from dbw_amd import dataset as DS
from dbw_amd import intrinsics
from dbw_amd.parallel import ShardedTrainStep
from dbw_amd.trainer import Trainer
from test_parallel_cpu import ToyModel, torch_adam


def _torch_apply(K0, theta):
    return IR.refine_torch(K0, theta, torch.float32)


def _refiner(**kw):
    return intrinsics.IntrinsicsRefiner(IR.K0, 'cpu', adam_fn=torch_adam, apply_fn=IR.host_intrinsics_apply, **kw)


def test_parse_config_refusals():
    assert intrinsics.parse_config(None) is None and intrinsics.parse_config(False) is None
    assert intrinsics.parse_config(True) == {'lr': 1e-4, 'start_epoch': 0, 'focal': 'shared', 'principal': False}
    assert intrinsics.parse_config(3e-4)['lr'] == 3e-4
    assert intrinsics.parse_config({'focal': 'separate', 'principal': True, 'start_epoch': 5}) == {'lr': 1e-4, 'start_epoch': 5, 'focal': 'separate',
                                                                                                 'principal': True}
    assert intrinsics.parse_config({'focal': False})['focal'] is False
    with pytest.raises(ValueError, match='unknown keys'):
        intrinsics.parse_config({'learning_rate': 1.0})
    for lr in (0, -1e-4, float('nan')):
        with pytest.raises(ValueError, match='positive'):
            intrinsics.parse_config({'lr': lr})
    with pytest.raises(ValueError, match='focal'):
        intrinsics.parse_config({'focal': 'both'})
    with pytest.raises(ValueError, match='focal'):
        _refiner(focal='both')


def test_shared_keeps_the_two_scales_equal_bit_for_bit():
    ref = _refiner(lr=1e-2, focal='shared', principal=True)
    gen = torch.Generator().manual_seed(3)
    for k in range(5):
        g = torch.randn(4, generator=gen)
        ref.grad.copy_(g)
        ref.step()
        assert not ref.grad.any()                                          # step() leaves the gradient buffer cleared
        assert ref.flat[0] == ref.flat[1] and float(ref.flat[0]) != 0.0, k
    assert ref.n_steps == 5 and bool(ref.flat[2:].ne(0).all())
    K = ref.refined()
    assert not K.requires_grad and float(K[0, 0] / IR.K0[0, 0]) == pytest.approx(float(K[1, 1] / IR.K0[1, 1]), rel=1e-6)
    # the shared scale is Adam on the SUM of the two gradients
    p = torch.zeros(1, requires_grad=True)
    opt = torch.optim.Adam([p], lr=1e-2)
    gen = torch.Generator().manual_seed(3)
    for _ in range(5):
        g = torch.randn(4, generator=gen)
        p.grad = (g[0] + g[1]).reshape(1)
        opt.step()
    assert torch.allclose(ref.flat[0], p.detach()[0], rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize('focal,principal', [(False, True), ('separate', False), ('shared', False), (False, False), ('separate', True)])
def test_frozen_parts_stay_exactly_zero(focal, principal):
    ref = _refiner(lr=1e-2, focal=focal, principal=principal)
    gen = torch.Generator().manual_seed(4)
    for _ in range(4):
        ref.grad.copy_(torch.randn(4, generator=gen))
        ref.step()
    assert bool(ref.flat[:2].ne(0).all()) == bool(focal) and bool(ref.flat[2:].ne(0).all()) == principal
    if not focal:
        assert not ref.flat[:2].any() and not ref.exp_avg[:2].any()
    if not principal:
        assert not ref.flat[2:].any() and not ref.exp_avg[2:].any()
    if focal == 'separate':
        assert ref.flat[0] != ref.flat[1]
    if not focal and not principal:
        assert torch.equal(ref.refined(), IR.K0)                           # theta = 0: K0 bit for bit


def test_state_round_trip():
    ref = _refiner(lr=3e-4, focal='separate', principal=True)
    with torch.no_grad():
        ref.flat.copy_(torch.randn(4))
        ref.exp_avg.copy_(torch.randn(4))
        ref.exp_avg_sq.copy_(torch.rand(4))
    ref.n_steps = 7
    sd = ref.state_dict()
    assert set(sd) >= {'theta', 'exp_avg', 'exp_avg_sq', 'n_steps'}
    other = _refiner(focal='separate', principal=True)
    other.load_state_dict(sd)
    assert torch.equal(other.flat, ref.flat) and torch.equal(other.exp_avg, ref.exp_avg) and torch.equal(other.exp_avg_sq, ref.exp_avg_sq)
    assert other.n_steps == 7 and torch.equal(other.theta, ref.theta) and torch.equal(other.refined(), ref.refined())
    with pytest.raises(ValueError, match='4'):
        other.load_state_dict(dict(sd, theta=torch.zeros(6)))


# ---- the files ------------------------------------------------------------------------------------------------------------------------
def _capture(tmp_path, tag, dist=(0.0,) * 6, **kw):
    write_capture(tmp_path, tag, n=11, H=8, W=12, dist=dist, **kw)
    return DS.CustomScene(tmp_path, tag, 'train', normalize='none')


def _moved(scene, theta):
    ref = intrinsics.IntrinsicsRefiner(scene.K[0], 'cpu', adam_fn=torch_adam, apply_fn=IR.host_intrinsics_apply, focal='separate', principal=True)
    with torch.no_grad():
        ref.flat.copy_(torch.tensor(theta))
    return ref


def test_refined_file_read_back_gives_the_refined_matrix(tmp_path):
    s = _capture(tmp_path, 'a')
    assert intrinsics.file_level_refusal(s) is None
    ref = _moved(s, [0.02, -0.015, 0.01, -0.008])
    K1 = ref.refined()
    assert float((K1 - s.K[0]).abs().max()) > 5e-3
    paths = intrinsics.write_refined(s, ref, tmp_path, s.img_size)
    assert [os.path.basename(p) for p in paths] == ['intrinsics_refined.yml', 'transforms_refined.json']
    shutil.copytree(s.data_path, tmp_path / 'custom' / 'a2')
    shutil.copy(paths[1], tmp_path / 'custom' / 'a2' / 'transforms.json')
    s2 = DS.CustomScene(tmp_path, 'a2', 'train', normalize='none')
    err = float((s2.K[0] - K1).abs().max())
    print(f'K read back: err {err:.2e}')
    assert err <= 1e-5
    assert torch.equal(s2.R, s.R) and torch.equal(s2.T, s.T)               # the poses are the file's own
    with open(paths[0]) as f:
        y = yaml.safe_load(f)
    assert y['transforms_refined'] is True and y['image_size'] == list(s.img_size) and set(y['theta']) == {'a_x', 'a_y', 'c_x', 'c_y'}
    assert torch.allclose(torch.tensor(y['K']), K1, rtol=0, atol=1e-7) and torch.allclose(torch.tensor(y['K0']), s.K[0], rtol=0, atol=1e-7)
    # pixels of the training image size: the NDC unit is half the shorter side, the principal point's sign is the file's
    half = min(s.img_size) / 2.0
    assert y['pixels']['fl_x'] == pytest.approx(float(K1[0, 0]) * half, rel=1e-6)
    assert y['pixels']['cx'] == pytest.approx(s.img_size[1] / 2.0 - float(K1[0, 2]) * half, rel=1e-6)
    # zero refinement: the file's own values come back
    with open(s.data_path / 'transforms.json') as f:
        src = json.load(f)
    same = intrinsics.refined_transforms(s, s.K[0])
    for k in ('fl_x', 'fl_y', 'cx', 'cy'):
        assert same[k] == pytest.approx(src[k], abs=1e-4)
    assert same['frames'] == src['frames']


def test_the_file_pose_refinement_wrote_is_updated(tmp_path):
    s = _capture(tmp_path, 'b')
    ref = _moved(s, [0.02, 0.02, 0.0, 0.0])
    with open(s.data_path / 'transforms.json') as f:
        posed = json.load(f)
    posed['frames'][0]['transform_matrix'][0][3] += 0.125                   # what a pose refinement left in the run directory
    with open(tmp_path / 'transforms_refined.json', 'w') as f:
        json.dump(posed, f)
    paths = intrinsics.write_refined(s, ref, tmp_path, s.img_size, after_pose=True)
    with open(paths[1]) as f:
        out = json.load(f)
    assert out['frames'] == posed['frames'] and out['fl_x'] == pytest.approx(posed['fl_x'] * float(torch.exp(torch.tensor(0.02))), rel=1e-5)


def test_a_capture_with_lens_coefficients_gets_the_yml_only(tmp_path):
    s = _capture(tmp_path, 'c', dist=LR.COEFFS[0])
    why = intrinsics.file_level_refusal(s)
    assert why is not None and 'lens' in why
    ref = _moved(s, [0.01, 0.01, 0.0, 0.0])
    with pytest.raises(ValueError, match='lens'):
        intrinsics.refined_transforms(s, ref.refined())
    paths = intrinsics.write_refined(s, ref, tmp_path, s.img_size)
    assert [os.path.basename(p) for p in paths] == ['intrinsics_refined.yml'] and not (tmp_path / 'transforms_refined.json').exists()
    with open(paths[0]) as f:
        y = yaml.safe_load(f)
    assert y['transforms_refined'] is False and 'lens' in y['transforms_refined_reason']

    class Scan:
        name = 'dtu'
    assert 'dtu' in intrinsics.file_level_refusal(Scan())


# ---- the Trainer ----------------------------------------------------------------------------------------------------------------------
def _cfg(**training):
    return {'training': dict({'batch_size': 2, 'n_epoches': 1, 'seed': 7, 'optimizer': {'name': 'adam', 'lr': 1e-2}}, **training)}


def _views():
    gen = torch.Generator().manual_seed(1)
    return {'imgs': torch.rand(5, 3, 4, 4, generator=gen), 'R': torch.eye(3).expand(5, 3, 3).contiguous(), 'T': torch.randn(5, 3, generator=gen),
            'K': IR.K0.expand(5, 4, 4).contiguous()}


def _epoch(tr):
    tr.step_fn.adam_fn = torch_adam
    seen = []
    step = tr.run_single_batch_train
    tr.run_single_batch_train = lambda batch, count=None: (seen.append(batch), step(batch, count))[1]
    tr.run_epoch(shuffle=False)
    return seen


def test_trainer_without_the_key_builds_nothing():
    tr = Trainer(_cfg(), ToyModel(), _views())
    assert tr.intrinsics is None and tr.view_ids is False and 'intrinsics_refine' not in tr.state_dict()
    seen = _epoch(tr)
    assert len(seen) == 3 and all(set(b) == {'imgs', 'R', 'T', 'K'} for b in seen)            # no batch gains a key
    assert not any(t.requires_grad for b in seen for t in b.values())
    for off in (None, False):
        assert Trainer(_cfg(intrinsics_refine=off), ToyModel(), _views()).intrinsics is None


def test_trainer_with_the_key():
    cfg = _cfg(intrinsics_refine={'lr': 3e-4, 'start_epoch': 2, 'focal': 'separate', 'principal': True})
    tr = Trainer(cfg, ToyModel(), _views())
    ref = tr.intrinsics
    assert ref is not None and ref.lr == 3e-4 and ref.focal == 'separate' and ref.principal and tr.intrinsics_cfg['start_epoch'] == 2
    assert torch.equal(ref.K0, IR.K0) and tr.view_ids is False                                 # (theta is no per-view table: no view ids)
    ref.adam_fn, ref.apply_fn = torch_adam, _torch_apply
    # before start_epoch the batches are today's
    seen = _epoch(tr)
    assert all('K_live' not in b for b in seen) and ref.n_steps == 0 and tr.epoch == 2
    # from start_epoch on they carry the live matrix, with a gradient to theta, and the refiner steps once per batch
    tr.run_single_batch_train = Trainer.run_single_batch_train.__get__(tr)
    seen = _epoch(tr)
    assert len(seen) == 3 and all(b['K_live'].requires_grad and tuple(b['K_live'].shape) == (4, 4) for b in seen) and ref.n_steps == 3
    assert torch.equal(seen[0]['K_live'].detach(), IR.K0)                                      # theta = 0 at the first step
    assert not ref.flat.any()                                                                  # (the toy model does not read K: zero gradient, theta stays)
    # the state round trip through the Trainer's checkpoint
    with torch.no_grad():
        ref.flat.copy_(torch.tensor([0.01, -0.02, 0.003, 0.004]))
        ref.exp_avg.copy_(torch.randn(4))
    sd = tr.state_dict()
    assert set(sd['intrinsics_refine']) >= {'theta', 'exp_avg', 'exp_avg_sq', 'n_steps'}
    tr2 = Trainer(cfg, ToyModel(), _views())
    tr2.load_state_dict(sd)
    assert torch.equal(tr2.intrinsics.flat, ref.flat) and torch.equal(tr2.intrinsics.exp_avg, ref.exp_avg) and tr2.intrinsics.n_steps == 3
    # a checkpoint of a run without refinement still loads: the refiner starts at 0
    tr3 = Trainer(cfg, ToyModel(), _views())
    tr3.load_state_dict({k: v for k, v in sd.items() if k != 'intrinsics_refine'})
    assert not tr3.intrinsics.flat.any()
    with pytest.raises(ValueError, match='unknown keys'):
        Trainer(_cfg(intrinsics_refine={'learning_rate': 1.0}), ToyModel(), _views())
    with pytest.raises(KeyError, match="'K'"):
        Trainer(cfg, ToyModel(), {k: v for k, v in _views().items() if k != 'K'})


def test_a_gradient_reaches_theta_through_the_step():
    """A toy model that reads K_live: the autograd iteration leaves d loss / d theta in the refiner's flat gradient buffer, step() consumes it."""
    class KModel(ToyModel):
        def forward(self, inp, labels=None):
            out = super().forward(inp, labels)
            return dict(out, total=out['total'] + (inp['K_live'][0, 0] - 2.0) ** 2 + inp['K_live'][0, 2])
    ref = intrinsics.IntrinsicsRefiner(IR.K0, 'cpu', lr=1e-2, adam_fn=torch_adam, apply_fn=_torch_apply, focal='separate', principal=True)
    step = ShardedTrainStep(KModel(), adam_fn=torch_adam)
    v = _views()
    step(ref.apply({'imgs': v['imgs'], 'R': v['R'], 'T': v['T']}))
    want = torch.tensor([2 * (float(IR.K0[0, 0]) - 2.0) * float(IR.K0[0, 0]), 0.0, 1.0, 0.0])
    assert torch.allclose(ref.grad, want, rtol=1e-6, atol=1e-7)
    ref.step()
    assert not ref.grad.any() and float(ref.flat[0]) < 0 and float(ref.flat[2]) < 0 and not ref.flat[[1, 3]].any()


def test_refined_intrinsics_under_two_ranks_are_refused():
    step = ShardedTrainStep(ToyModel(), adam_fn=torch_adam)
    v = _views()
    live = IR.K0.clone().requires_grad_(True)
    step({'imgs': v['imgs'], 'R': v['R'], 'T': v['T'], 'K_live': live})                        # one rank: the autograd iteration
    step.world_size = 2
    with pytest.raises(NotImplementedError, match='intrinsics'):
        step({'imgs': v['imgs'], 'R': v['R'], 'T': v['T'], 'K_live': live})


def test_the_command_line_flag_sets_the_key(tmp_path):
    from dbw_amd import train
    cfg_file = tmp_path / 'c.yml'
    cfg_file.write_text('dataset: {name: custom, tag: x}\nmodel: {loss: {perceptual_weight: 0}}\ntraining: {intrinsics_refine: {start_epoch: 3}}\n')
    (tmp_path / 'default.yml').write_text('training: {batch_size: 2}\n')
    args = train.parse_args(['-c', str(cfg_file), '-t', 't', '--data-root', 'd', '--runs-root', 'r', '--intrinsics-refine', '2e-4'])
    assert train.prepare_config(args)['training']['intrinsics_refine'] == {'start_epoch': 3, 'lr': 2e-4}
    args = train.parse_args(['-c', str(cfg_file), '-t', 't', '--data-root', 'd', '--runs-root', 'r'])
    assert train.prepare_config(args)['training']['intrinsics_refine'] == {'start_epoch': 3}


class _EvalModel(ToyModel):
    """ToyModel with the evaluation members Trainer.evaluate calls and four renderers that record the K they are given."""

    class _R:
        def __init__(self):
            self.K = None

        def update_cameras(self, device=None, K=None):
            self.K = K

    def __init__(self):
        super().__init__()
        self.renderer, self.renderer_fine, self.renderer_env, self.renderer_light = (self._R() for _ in range(4))

    def qualitative_eval(self, loader, device, path=None, **kw):
        self.quali_K = self.renderer.K

    def quantitative_eval(self, loader, device, hard_inference=True):
        return {'PSNR': 1.0}


def test_evaluate_installs_the_refined_matrix_and_writes_the_yml(tmp_path):
    tr = Trainer(_cfg(intrinsics_refine={'lr': 1e-3, 'focal': 'separate'}), _EvalModel(), _views())
    tr.intrinsics.adam_fn, tr.intrinsics.apply_fn = torch_adam, IR.host_intrinsics_apply
    with torch.no_grad():
        tr.intrinsics.flat.copy_(torch.tensor([0.02, -0.01, 0.0, 0.0]))
    K1 = tr.intrinsics.refined()
    assert tr.evaluate([], tmp_path)['PSNR'] == 1.0
    m = tr.model
    for r in (m.renderer, m.renderer_fine, m.renderer_env, m.renderer_light):
        assert tuple(r.K.shape) == (1, 4, 4) and torch.equal(r.K[0], K1)
    assert m.quali_K is m.renderer.K                                       # installed BEFORE the first evaluation render
    with open(tmp_path / 'intrinsics_refined.yml') as f:
        y = yaml.safe_load(f)
    assert y['transforms_refined'] is False and y['theta']['a_x'] == pytest.approx(0.02) and not (tmp_path / 'transforms_refined.json').exists()
    # without the key evaluate writes nothing of this and touches no renderer
    plain = Trainer(_cfg(), _EvalModel(), _views())
    plain.evaluate([], tmp_path / 'plain')
    assert plain.model.renderer.K is None and not (tmp_path / 'plain' / 'intrinsics_refined.yml').exists()
