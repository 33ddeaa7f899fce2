"""CPU tests of the host side of the camera pose refinement: the refined poses written back into a capture's own
transforms.json (pose.refined_transforms) and read again through dataset.CustomScene, the refusal of duplicate view ids, the Trainer with
and without training.pose_refine, PoseRefiner's Adam step with half of delta frozen, and the refusal under data parallelism.  The kernels
are not involved: the host build of csrc/pose_math.h (tests/pose_ref.py) and a torch Adam stand in through PoseRefiner's adam_fn / apply_fn."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import pose_ref as PR
from custom_fixture import write_capture
from dbw_amd import dataset as DS
from dbw_amd import ops, pose
from dbw_amd.parallel import ShardedTrainStep
from dbw_amd.trainer import Trainer
from test_parallel_cpu import ToyModel, torch_adam

DATAPARSER = (np.array([[0, 1, 0, 0.5], [-1, 0, 0, -2.0], [0, 0, 1, 0.25]], dtype=np.float64), 0.125)


def _refiner(n, **kw):
    return pose.PoseRefiner(n, 'cpu', adam_fn=torch_adam, apply_fn=PR.host_pose_apply, **kw)


def _capture(tmp_path, tag, **kw):
    write_capture(tmp_path, tag, n=11, H=8, W=12, dist=(0.0,) * 6, **kw)
    return DS.CustomScene(tmp_path, tag, 'train', **({} if 'dataparser' in kw else {'normalize': 'none'}))


@pytest.mark.parametrize('frame', ['dataparser', 'none'])
def test_zero_refinement_writes_the_input_matrices(tmp_path, frame):
    s = _capture(tmp_path, 'a', **({'dataparser': DATAPARSER} if frame == 'dataparser' else {}))
    assert len(s) == 10                                             # 11 frames: 10 train, 1 test
    meta = pose.refined_transforms(s, torch.zeros(len(s), 6))
    with open(s.data_path / 'transforms.json') as f:
        src = json.load(f)
    for a, b in zip(meta['frames'], src['frames']):
        assert np.abs(np.asarray(a['transform_matrix']) - np.asarray(b['transform_matrix'])).max() <= 1e-6
    assert {k: v for k, v in meta.items() if k != 'frames'} == {k: v for k, v in src.items() if k != 'frames'}


@pytest.mark.parametrize('frame', ['dataparser', 'none'])
def test_refined_file_read_back_gives_the_refined_poses(tmp_path, frame):
    kw = {'dataparser': DATAPARSER} if frame == 'dataparser' else {}
    s = _capture(tmp_path, 'b', **kw)
    ids = s.ids()
    ref = _refiner(len(s))
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        ref.flat.copy_(torch.cat([0.03 * torch.randn(len(s), 3, generator=gen), 0.02 * torch.randn(len(s), 3, generator=gen)], 1).reshape(-1))
    R, T = ref.refined(s.R[ids], s.T[ids])
    assert float((R - s.R[ids]).abs().max()) > 1e-3 and float((T - s.T[ids]).abs().max()) > 1e-3
    # the file the Trainer writes, put in the place of the capture's transforms.json (same frames, same dataparser file)
    path = pose.write_refined(s, ref, tmp_path, s.R[ids], s.T[ids])
    assert os.path.basename(path) == 'transforms_refined.json'
    shutil.copytree(s.data_path, tmp_path / 'custom' / 'b2')
    shutil.copy(path, tmp_path / 'custom' / 'b2' / 'transforms.json')
    s2 = DS.CustomScene(tmp_path, 'b2', 'train', **({} if kw else {'normalize': 'none'}))
    eR, eT = float((s2.R[ids] - R).abs().max()), float((s2.T[ids] - T).abs().max())
    print(f'{frame}: R err {eR:.2e}, T err {eT:.2e}')
    assert eR <= 1e-5 and eT <= 1e-5
    test_id = [i for i in range(11) if i not in ids]
    assert torch.equal(s2.R[test_id], s.R[test_id]) and torch.equal(s2.T[test_id], s.T[test_id])       # only training frames change


def test_other_scenes_get_an_npz(tmp_path):
    ref = _refiner(3)
    R0, T0 = torch.eye(3).expand(3, 3, 3).contiguous(), torch.randn(3, 3)

    class Scan:
        name = 'dtu'
    path = pose.write_refined(Scan(), ref, tmp_path, R0, T0)
    z = np.load(path)
    assert os.path.basename(path) == 'poses_refined.npz' and z['R'].shape == (3, 3, 3) and z['T'].shape == (3, 3) and z['delta'].shape == (3, 6)
    assert np.array_equal(z['R'], R0.numpy()) and np.array_equal(z['T'], T0.numpy())


def test_duplicate_or_foreign_view_ids_are_refused():
    R0, T0, delta = torch.eye(3).expand(2, 3, 3).contiguous(), torch.zeros(2, 3), torch.zeros(4, 6)
    with pytest.raises(ValueError, match='distinct'):
        ops.pose_apply(R0, T0, delta, torch.tensor([1, 1]))
    with pytest.raises(ValueError, match='outside'):
        ops.pose_apply(R0, T0, delta, torch.tensor([1, 4]))
    with pytest.raises(ValueError, match='one per view'):
        ops.pose_apply(R0, T0, delta, torch.tensor([1]))
    with pytest.raises(KeyError, match='view_ids'):
        _refiner(4).apply({'R': R0, 'T': T0})


def _cfg(**training):
    return {'training': dict({'batch_size': 2, 'n_epoches': 1, 'seed': 7, 'optimizer': {'name': 'adam', 'lr': 1e-2}}, **training)}


def _views():
    gen = torch.Generator().manual_seed(1)
    return {'imgs': torch.rand(5, 3, 4, 4, generator=gen), 'R': torch.eye(3).expand(5, 3, 3).contiguous(), 'T': torch.randn(5, 3, generator=gen)}


def test_trainer_without_the_key_builds_nothing():
    tr = Trainer(_cfg(), ToyModel(), _views())
    assert tr.pose is None and tr.view_ids is False and 'pose_refine' not in tr.state_dict()
    tr.step_fn.adam_fn = torch_adam
    seen = []
    step = tr.run_single_batch_train
    tr.run_single_batch_train = lambda batch, count=None: (seen.append(batch), step(batch, count))[1]
    tr.run_epoch(shuffle=False)
    assert all('view_ids' not in b and not b['R'].requires_grad for b in seen)
    for off in (None, False):
        assert Trainer(_cfg(pose_refine=off), ToyModel(), _views()).pose is None


def test_trainer_state_round_trips_with_the_key():
    cfg = _cfg(pose_refine={'lr': 3e-4, 'start_epoch': 2, 'trans': False})
    tr = Trainer(cfg, ToyModel(), _views())
    assert tr.pose is not None and tr.view_ids and tr.pose.lr == 3e-4 and tr.pose.rot and not tr.pose.trans and tr.pose_cfg['start_epoch'] == 2
    with torch.no_grad():
        tr.pose.flat.copy_(torch.randn(30))
        tr.pose.exp_avg.copy_(torch.randn(30))
        tr.pose.exp_avg_sq.copy_(torch.rand(30))
    tr.pose.n_steps = 11
    sd = tr.state_dict()
    assert set(sd['pose_refine']) >= {'delta', 'exp_avg', 'exp_avg_sq', 'n_steps'}
    tr2 = Trainer(cfg, ToyModel(), _views())
    tr2.load_state_dict(sd)
    assert torch.equal(tr2.pose.flat, tr.pose.flat) and torch.equal(tr2.pose.exp_avg, tr.pose.exp_avg)
    assert torch.equal(tr2.pose.exp_avg_sq, tr.pose.exp_avg_sq) and tr2.pose.n_steps == 11
    assert torch.equal(tr2.pose.delta, tr.pose.delta)                      # (delta is a view of the flat buffer)
    # a checkpoint of a run without refinement still loads: the refiner starts at 0
    plain = {k: v for k, v in sd.items() if k != 'pose_refine'}
    tr3 = Trainer(cfg, ToyModel(), _views())
    tr3.load_state_dict(plain)
    assert not tr3.pose.flat.any()
    # before start_epoch the batches carry view_ids but their poses are data
    tr.step_fn.adam_fn = torch_adam
    seen = []
    step = tr.run_single_batch_train
    tr.run_single_batch_train = lambda batch, count=None: (seen.append(batch), step(batch, count))[1]
    tr.run_epoch(shuffle=False)
    assert all('view_ids' in b and not b['R'].requires_grad for b in seen) and tr.pose.n_steps == 11
    with pytest.raises(ValueError, match='unknown keys'):
        Trainer(_cfg(pose_refine={'learning_rate': 1.0}), ToyModel(), _views())


@pytest.mark.parametrize('rot,trans', [(False, True), (True, False), (True, True)])
def test_a_frozen_half_stays_at_zero(rot, trans):
    ref = _refiner(4, lr=1e-2, rot=rot, trans=trans)
    gen = torch.Generator().manual_seed(3)
    for _ in range(3):
        ref.grad.copy_(torch.randn(24, generator=gen))
        ref.step()
        assert not ref.grad.any()                                          # step() leaves the gradient buffer cleared
    d = ref.flat.view(4, 6)
    assert bool(d[:, :3].any()) == rot and bool(d[:, 3:].any()) == trans and ref.n_steps == 3
    # dense Adam like torch.optim.Adam on the tensor
    if rot and trans:
        p = torch.zeros(4, 6, requires_grad=True)
        opt = torch.optim.Adam([p], lr=1e-2)
        gen = torch.Generator().manual_seed(3)
        for _ in range(3):
            p.grad = torch.randn(24, generator=gen).view(4, 6)
            opt.step()
        assert torch.allclose(d, p.detach(), rtol=1e-5, atol=1e-8)


def test_refined_poses_under_two_ranks_are_refused():
    step = ShardedTrainStep(ToyModel(), adam_fn=torch_adam)
    v = _views()
    step({'imgs': v['imgs'], 'R': v['R'].clone().requires_grad_(True), 'T': v['T']})         # one rank: the autograd iteration
    step.world_size = 2
    with pytest.raises(NotImplementedError, match='pose'):
        step({'imgs': v['imgs'], 'R': v['R'].clone().requires_grad_(True), 'T': v['T']})
    with pytest.raises(NotImplementedError, match='pose'):
        step({'imgs': v['imgs'], 'R': v['R'], 'T': v['T'].clone().requires_grad_(True)})


def test_the_command_line_flag_sets_the_key(tmp_path):
    from dbw_amd import train
    cfg_file = tmp_path / 'c.yml'
    cfg_file.write_text('dataset: {name: custom, tag: x}\nmodel: {loss: {perceptual_weight: 0}}\ntraining: {pose_refine: {start_epoch: 3}}\n')
    (tmp_path / 'default.yml').write_text('training: {batch_size: 2}\n')
    args = train.parse_args(['-c', str(cfg_file), '-t', 't', '--data-root', 'd', '--runs-root', 'r', '--pose-refine', '2e-4'])
    cfg = train.prepare_config(args)
    assert cfg['training']['pose_refine'] == {'start_epoch': 3, 'lr': 2e-4}
    args = train.parse_args(['-c', str(cfg_file), '-t', 't', '--data-root', 'd', '--runs-root', 'r'])
    assert train.prepare_config(args)['training']['pose_refine'] == {'start_epoch': 3}


class _EvalModel(ToyModel):
    """ToyModel with the two evaluation members Trainer.evaluate calls: they record the poses every batch arrives with."""

    def qualitative_eval(self, loader, device, path=None, **kw):
        self.quali = [(inp['R'].clone(), inp['T'].clone()) for inp, _ in loader]

    def quantitative_eval(self, loader, device, hard_inference=True):
        self.quanti = [(inp['R'].clone(), inp['T'].clone()) for inp, _ in loader]
        return {'PSNR': 1.0}


class _Loader:
    def __init__(self, dataset, views, batch_size):
        self.dataset, self.views, self.batch_size = dataset, views, batch_size

    def __len__(self):
        return -(-len(self.views['R']) // self.batch_size)

    def __iter__(self):
        for a in range(0, len(self.views['R']), self.batch_size):
            yield {k: v[a:a + self.batch_size] for k, v in self.views.items()}, {}


def test_evaluate_on_the_training_views_uses_the_refined_poses(tmp_path):
    """5 views in batches of 2 (2, 2, 1): every batch of the train scene's loader arrives with its own slice of the refined poses, in order,
    in both walks of the loader; a loader over another scene keeps its poses; the refined poses are written to the run directory."""
    class Scan:
        name = 'dtu'
    views = _views()
    views['R'] = torch.stack([PR.pose_case(1.0, s)[0] for s in range(5)])               # five different rotations
    tr = Trainer(_cfg(pose_refine={'lr': 1e-3}), _EvalModel(), views)
    tr.pose.apply_fn, tr.pose.adam_fn = PR.host_pose_apply, torch_adam
    with torch.no_grad():
        tr.pose.flat.copy_(0.05 * torch.randn(30, generator=torch.Generator().manual_seed(2)))
    tr.scene = Scan()
    R, T = tr.pose.refined(views['R'], views['T'])
    assert float((R - views['R']).abs().max()) > 1e-3 and float((T - views['T']).abs().max()) > 1e-3
    scores = tr.evaluate(_Loader(tr.scene, views, 2), tmp_path)
    assert scores['PSNR'] == 1.0
    for seen in (tr.model.quali, tr.model.quanti):
        assert [len(r) for r, _ in seen] == [2, 2, 1]
        assert torch.equal(torch.cat([r for r, _ in seen]), R) and torch.equal(torch.cat([t for _, t in seen]), T)
    z = np.load(tmp_path / 'poses_refined.npz')
    assert np.array_equal(z['R'], R.numpy()) and np.array_equal(z['T'], T.numpy()) and np.array_equal(z['delta'], tr.pose.flat.view(5, 6).numpy())
    # another scene's loader (a test split): its poses are left as they are
    tr.evaluate(_Loader(Scan(), views, 2), tmp_path)
    assert torch.equal(torch.cat([r for r, _ in tr.model.quanti]), views['R']) and torch.equal(torch.cat([t for _, t in tr.model.quanti]), views['T'])
    # without the key evaluate writes nothing of this and changes no pose
    plain = Trainer(_cfg(), _EvalModel(), views)
    plain.scene = Scan()
    plain.evaluate(_Loader(plain.scene, views, 2), tmp_path / 'plain')
    assert torch.equal(torch.cat([r for r, _ in plain.model.quanti]), views['R']) and not (tmp_path / 'plain' / 'poses_refined.npz').exists()
