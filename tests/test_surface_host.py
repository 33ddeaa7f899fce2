"""CPU tests of the host side of the surface term: the configuration and its refusals, the loss names, the gate of the fast
training paths, the cloud's way into the model, the command-line flag, the shipped config, and eval3d.surface_term_torch -- the float64
gradient reference of tests/test_gpu_surface.py -- against torch.autograd.gradcheck and the numpy reference of tests/surface_ref.py."""
import os
import types

import numpy as np
import pytest
import torch

import custom_fixture as CF
import surface_ref as SR
from dbw_amd import create_model, dataset as DS, eval3d, phase, train
from dbw_amd.dbw import SURFACE_DEFAULTS, parse_surface_config
from dbw_amd.trainer import Trainer
from test_parallel_cpu import ToyModel

LOSS = {'rgb_weight': 1, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}


def _model(loss, n_blocks=2):
    cfg = {'model': {'name': 'dbw', 'mesh': {'n_blocks': n_blocks, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': 16},
                     'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                     'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True, 'opacity_noise': False},
                     'loss': loss}}
    torch.manual_seed(1)
    return create_model(cfg, (16, 24))


def test_the_configuration_and_its_refusals():
    assert parse_surface_config(None) == SURFACE_DEFAULTS == {'points': 16384, 'tau': 0.1, 'back': 0.5, 'ground': True, 'start_epoch': 1, 'max_cloud': 262144}
    got = parse_surface_config({'points': 0, 'tau': '0.05', 'ground': False})
    assert got == dict(SURFACE_DEFAULTS, points=0, tau=0.05, ground=False) and isinstance(got['tau'], float)
    with pytest.raises(ValueError, match=r'model\.loss\.surface\.radius: not one of points, tau, back, ground, start_epoch, max_cloud'):
        parse_surface_config({'radius': 0.1})
    with pytest.raises(ValueError, match='a mapping of'):
        parse_surface_config(0.1)
    for bad in ({'tau': 0}, {'tau': -1}, {'back': -0.1}, {'points': -1}, {'max_cloud': 0}, {'tau': float('inf')}):
        with pytest.raises(ValueError, match=r'model\.loss\.surface\.'):
            parse_surface_config(bad)
    with pytest.raises(ValueError, match='not one of'):
        _model(dict(LOSS, surface_weight=1, surface={'weight': 2}))
    assert 'NOT measured' in parse_surface_config.__doc__


def test_loss_names_and_the_gate_of_the_fast_paths():
    plain, zero, on = _model(dict(LOSS)), _model(dict(LOSS, surface_weight=0, surface={'tau': 0.2})), _model(dict(LOSS, surface_weight=0.5))
    assert plain.loss_names == zero.loss_names == ['loss_rgb', 'loss_parsimony', 'loss_tv', 'loss_overlap', 'loss_total']
    assert 'surface' not in plain.loss_weights and 'surface' not in zero.loss_weights and zero.surface_cfg['tau'] == 0.2
    assert on.loss_names == ['loss_rgb', 'loss_parsimony', 'loss_tv', 'loss_overlap', 'loss_surface', 'loss_total']
    assert on.loss_weights['surface'] == 0.5 and on.surface_cfg == SURFACE_DEFAULTS
    assert phase.fast_path_refusal(plain) is None and phase.fast_path_refusal(zero) is None
    assert phase.fast_path_refusal(on) == 'a surface term'
    from dbw_amd.native_step import NativeStep
    on.sync_free = plain.sync_free = True
    assert NativeStep.supported(types.SimpleNamespace(m=plain)) and not NativeStep.supported(types.SimpleNamespace(m=on))


def test_a_weight_without_points_raises_when_a_loss_is_asked_for():
    m = _model({'rgb_weight': 1, 'surface_weight': 1})
    imgs = torch.rand(1, 3, 16, 24)
    with pytest.raises(RuntimeError, match=r'surface_weight > 0 needs the capture.s point cloud: model\.set_surface_points'):
        m.compute_losses(imgs, imgs.clone())
    assert set(_model({'rgb_weight': 1}).compute_losses(imgs, imgs.clone())) == {'rgb', 'total'}
    m.world_size = 2
    with pytest.raises(NotImplementedError, match='the surface term under data parallelism'):
        m.compute_losses(imgs, imgs.clone())


def test_the_cloud_is_thinned_and_stays_out_of_checkpoints():
    m = _model(dict(LOSS, surface_weight=1, surface={'max_cloud': 100}))
    p = torch.randn(1000, 3)
    p[5, 1] = float('nan')
    assert m.set_surface_points(p) == 100 and m._surface_points.shape == (100, 3) and m._surface_points.dtype == torch.float32
    first = m._surface_points.clone()
    assert bool(torch.isfinite(first).all()) and not torch.equal(first, p[:100])
    rows = {tuple(r.tolist()) for r in p[torch.isfinite(p).all(1)]}
    assert all(tuple(r.tolist()) in rows for r in first)
    assert m.set_surface_points(p.numpy()) == 100 and torch.equal(m._surface_points, first)       # the same permutation every time
    assert m.set_surface_points(p[:50]) == 49
    assert not any('surface' in k for k in m.state_dict())
    with pytest.raises(ValueError, match='no finite point'):
        m.set_surface_points(torch.full((3, 3), float('nan')))


def test_data_parallel_training_is_refused(monkeypatch):
    import dbw_amd.trainer as T
    from test_exposure_host import _cfg, _views

    class TwoRanks(T.ShardedTrainStep):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.world_size = 2
    monkeypatch.setattr(T, 'ShardedTrainStep', TwoRanks)
    toy = ToyModel()
    Trainer(_cfg(), toy, _views())                                                       # without the weight: nothing is refused
    toy.loss_weights = {'rgb': 1.0, 'surface': 1.0}
    with pytest.raises(NotImplementedError, match=r'model\.loss\.surface_weight under data parallelism'):
        Trainer(_cfg(), toy, _views())


def test_the_scene_hands_its_cloud_over_or_is_refused(tmp_path, capsys):
    CF.write_capture(tmp_path, 'with', with_points=True)
    CF.write_capture(tmp_path, 'without')
    m = _model(dict(LOSS, surface_weight=2))
    assert train.resolve_surface(DS.CustomScene(tmp_path, 'without', 'train'), _model(dict(LOSS)), 'cpu') is None      # no weight: nothing is asked
    scene = DS.CustomScene(tmp_path, 'with', 'train')
    assert train.resolve_surface(scene, m, 'cpu') == 30 and torch.equal(m._surface_points, scene.cloud('cpu').float())
    assert 'surface: weight 2 on 30 of 30 points, 16384 a step, tau 0.1, back 0.5, from epoch 1' in capsys.readouterr().out
    with pytest.raises(SystemExit, match=r"model\.loss\.surface_weight: 'without': no point cloud \(ply_file_path of transforms\.json, or points\.ply"):
        train.resolve_surface(DS.CustomScene(tmp_path, 'without', 'train'), m, 'cpu')
    for name in ('dtu', 'bmvs'):
        with pytest.raises(SystemExit, match=f"surface_weight is for custom scenes: the cloud of a '{name}' scene is the ground truth"):
            train.resolve_surface(types.SimpleNamespace(name=name, cloud=lambda d: torch.zeros(3, 3)), m, 'cpu')


def test_the_flag_and_the_shipped_config(tmp_path):
    cfg_file = tmp_path / 'c.yml'
    cfg_file.write_text('dataset: {name: custom, tag: x}\nmodel: {loss: {perceptual_weight: 0, surface: {tau: 0.05}}}\n')
    (tmp_path / 'default.yml').write_text('training: {batch_size: 2}\n')
    base = ['-c', str(cfg_file), '-t', 't', '--data-root', 'd', '--runs-root', 'r']
    assert 'surface_weight' not in train.prepare_config(train.parse_args(base))['model']['loss']
    cfg = train.prepare_config(train.parse_args(base + ['--surface', '0.25']))
    assert cfg['model']['loss']['surface_weight'] == 0.25 and cfg['model']['loss']['surface'] == {'tau': 0.05}
    here = os.path.dirname(os.path.abspath(__file__))
    cfg = DS.load_config(os.path.join(here, '..', 'differentiable-blocksworld_amd', 'configs', 'custom_surface.yml'))
    assert cfg['dataset']['name'] == 'custom' and cfg['model']['loss']['surface_weight'] == 1
    assert parse_surface_config(cfg['model']['loss']['surface']) == SURFACE_DEFAULTS
    assert train.wants_world_frame(cfg) and train.blocks_init_options(cfg) == {}


def _two_blocks():
    sc = SR.scene(2, ground=True, seed=2)
    rng = np.random.default_rng(8)
    v = sc['verts'].astype(np.float64)
    blk = np.nonzero(sc['vert_group'] >= 0)[0]
    centre = np.stack([v[sc['vert_group'] == k].mean(0) for k in range(2)])
    # 20 points pushed outwards from face centroids of the blocks: well inside tau, away from it, and away from the sides of their faces
    f = sc['faces'][8:][rng.choice(160, 20, replace=False)].astype(np.int64)
    w = rng.dirichlet(np.full(3, 6.0), 20)
    c = (w[:, :, None] * v[f]).sum(1)
    out = c - centre[sc['vert_group'][f[:, 0]]]
    pts = c + 0.03 * out / np.linalg.norm(out, axis=1, keepdims=True)
    return sc, pts, blk


def test_the_torch_formulation_passes_gradcheck_and_is_the_numpy_reference():
    sc, pts, blk = _two_blocks()
    near = SR.nearest_on_surface(pts, sc['verts'], sc['faces'])
    assert SR.kept_for_gradients(near, 0.1).all() and (near['d2'] < 0.5 * 0.01).all() and (near['bary'].min(1) > 1e-3).all()      # away from tau and from ties
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))        # noqa: E731
    P, faces, fg, vg = t(pts), t(sc['faces']), t(sc['face_group']), t(sc['vert_group'])
    v0 = t(sc['verts']).double()
    a0 = torch.tensor([0.8, 0.3], dtype=torch.float64)
    kw = dict(n_points=0, tau=0.1, back=0.5, seed=1, step=2, weight=1.5, back_count=2.0 * SR.BNV)

    def fn(v, a):
        return eval3d.surface_term_torch(P, v, faces, fg, None, a, vg, **kw)
    assert torch.autograd.gradcheck(fn, (v0.clone().requires_grad_(), a0.clone().requires_grad_()), eps=1e-7, atol=1e-7, rtol=1e-5)
    fwd, bk = SR.term_value(pts, sc['verts'], sc['faces'], None, 0.1, pts, a0.numpy(), sc['vert_group'], 0.5, 2.0 * SR.BNV)
    assert abs(fn(v0, a0).item() - 1.5 * (fwd + 0.5 * bk)) <= 1e-15
    assert fn(v0, a0).item() == eval3d.surface_term_torch(P, v0, faces, fg, None, a0, vg, **{k: v for k, v in kw.items() if k != 'back_count'}).item()
    # (the default back_count is the number of block vertices, n_blocks * BNV, not V)
    # the stated gradient: -2 b_m (p - c) / M on the corners of the winning face
    v = v0.clone().requires_grad_()
    eval3d.surface_term_torch(P, v, faces, fg, None, None, vg, **dict(kw, back=0.0)).backward()
    want = np.zeros_like(sc['verts'], dtype=np.float64)
    for i in range(len(pts)):
        for m in range(3):
            want[sc['faces'][near['face'][i], m]] += -2.0 * near['bary'][i, m] * (pts[i] - near['c'][i]) * 1.5 / len(pts)
    assert np.abs(v.grad.numpy() - want).max() <= 1e-12
    # the draw takes the rows the kernels take, and a dropped group is no part of the surface
    idx = eval3d.surface_draw(7, 3, 64, 20)
    assert np.array_equal(idx.numpy(), SR.draw_indices(7, 3, 64, 20))
    keep = torch.tensor([1, 0, 1], dtype=torch.int32)
    got = eval3d.surface_term_torch(P, v0, faces, fg, keep, None, vg, **dict(kw, back=0.0, n_points=64, seed=7, step=3)).item()
    fk = np.ones(len(sc['faces']), bool)
    fk[sc['face_group'][1]:sc['face_group'][2]] = False
    assert abs(got - 1.5 * SR.term_value(pts[idx.numpy()], sc['verts'], sc['faces'], fk, 0.1)[0]) <= 1e-15
