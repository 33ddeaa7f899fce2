"""CPU tests of the host side of the free-space term: ops.freespace_term_torch -- the float64 gradient reference of
tests/test_gpu_freespace.py -- against finite differences of its own value, the closed-form gradient against its autograd, the numpy
reference of tests/freespace_ref.py, the configuration and its refusals, the loss names, the gate of the fast training paths, the rays' way
from the scene into the model, the command-line flag, the shipped config, the rays of the analytic capture of tests/depth_fixture.py, and
ops.depth_rays_host against the host build of csrc/depth_math.h byte for byte."""
import os
import types

import numpy as np
import pytest
import torch

import custom_fixture as CF
import depth_fixture as DF
import depth_ref as DR
import freespace_ref as FR
from dbw_amd import create_model, dataset as DS, ops, phase, train
from dbw_amd.dbw import FREESPACE_DEFAULTS, parse_freespace_config
from dbw_amd.trainer import Trainer
from test_parallel_cpu import ToyModel

LOSS = {'rgb_weight': 1, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}
TAU, MARGIN = 0.1, 0.02


def _model(loss, n_blocks=2):
    cfg = {'model': {'name': 'dbw', 'mesh': {'n_blocks': n_blocks, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': 16},
                     'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                     'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True, 'opacity_noise': False},
                     'loss': loss}}
    torch.manual_seed(1)
    return create_model(cfg, (16, 24))


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _torch_term(sc, origins, ends, frame, verts, alpha, **kw):
    kw = dict(dict(n_rays=0, tau=TAU, margin=MARGIN, seed=1, step=2, weight=1.5), **kw)
    return ops.freespace_term_torch(_t(ends), _t(frame), _t(origins), verts, _t(sc['faces']), _t(sc['face_group']), _t(sc['group_keep']),
                                    _t(sc['group_alpha']), alpha, **kw)


def test_the_torch_formulation_against_finite_differences_on_one_face():
    sc, origins = FR.scene('one_face')
    ends, frame = FR.rays_through(sc, origins, 400, seed=2)
    h = FR.first_hits(ends, frame, origins, sc['verts'], sc['faces'], None, TAU, MARGIN)
    keep = ~h['flagged']
    ends, frame = ends[keep], frame[keep]
    h = FR.first_hits(ends, frame, origins, sc['verts'], sc['faces'], None, TAU, MARGIN)
    assert (h['face'] >= 0).sum() > 50 and ((h['g'] > 0) & (h['g'] < TAU)).sum() > 5 and (h['g'] > TAU).sum() > 5      # both branches of the penalty
    v0, a0 = _t(sc['verts']).double(), torch.tensor([0.7], dtype=torch.float64)

    def fn(v, a):
        return _torch_term(sc, origins, ends, frame, v, a)
    assert torch.autograd.gradcheck(fn, (v0.clone().requires_grad_(), a0.clone().requires_grad_()), eps=1e-7, atol=1e-7, rtol=1e-5)
    assert abs(fn(v0, a0).item() - 1.5 * FR.term_value(ends, frame, origins, sc, [0.7], TAU, MARGIN)) <= 1e-15
    assert fn(v0, None).item() > fn(v0, a0).item() > 0                                   # without opacities every a is 1


@pytest.mark.parametrize('name', ['one_face', 'blocks', 'dropped', 'degenerate', 'inside'])
def test_the_closed_form_gradient_is_the_autograd_of_the_definition(name):
    """dL/dvert_m = -(w/M) a psi'(g) l wts_m n / (n . e) and dL/da_k = (w/M) sum psi, accumulated in numpy from the float64 first hits,
    against autograd through the intersection itself -- on every fixture of the GPU tests, whose flagged share is checked here against the
    reference alone."""
    sc, origins = FR.scene(name)
    ends, frame = FR.rays_through(sc, origins, 1000, seed=5)
    h = FR.first_hits(ends, frame, origins, sc['verts'], sc['faces'], FR.face_keep_of(sc), TAU, MARGIN)
    print(f'{name}: {100 * h["flagged"].mean():.2f} % flagged, {100 * (h["face"] >= 0).mean():.1f} % hit, {100 * (h["g"] > 0).mean():.1f} % penalised')
    assert h['flagged'].mean() <= FR.FLAG_CAP
    va = np.linspace(0.9, 0.3, sc['n_blocks'])
    v, a = _t(sc['verts']).double().requires_grad_(), _t(va).requires_grad_()
    out = _torch_term(sc, origins, ends, frame, v, a, weight=1.7)
    out.backward()
    gv, ga = FR.closed_form_grads(ends, frame, origins, sc, va, TAU, MARGIN, 1.7)
    assert abs(out.item() - 1.7 * FR.term_value(ends, frame, origins, sc, va, TAU, MARGIN)) <= 1e-14
    assert np.abs(gv).max() > 0 and FR.bars(v.grad.numpy(), gv) <= 1e-6 and FR.bars(a.grad.numpy(), ga) <= 1e-6
    # the draw takes the rays the kernels take
    idx = FR.draw_indices(7, 3, 64, len(ends))
    got = _torch_term(sc, origins, ends, frame, v.detach(), a.detach(), n_rays=64, seed=7, step=3).item()
    assert abs(got - 1.5 * FR.term_value(ends[idx], frame[idx], origins, sc, va, TAU, MARGIN)) <= 1e-15


def test_the_configuration_and_its_refusals():
    assert parse_freespace_config(None) == FREESPACE_DEFAULTS == {'rays': 16384, 'tau': 0.1, 'margin': 0.02, 'ground': True, 'start_epoch': 1,
                                                                  'max_rays': 1048576}
    got = parse_freespace_config({'rays': 0, 'tau': '0.05', 'ground': False})
    assert got == dict(FREESPACE_DEFAULTS, rays=0, tau=0.05, ground=False) and isinstance(got['tau'], float)
    with pytest.raises(ValueError, match=r'model\.loss\.freespace\.radius: not one of rays, tau, margin, ground, start_epoch, max_rays'):
        parse_freespace_config({'radius': 0.1})
    with pytest.raises(ValueError, match=r'model\.loss\.freespace: a mapping of rays, tau, margin'):
        parse_freespace_config(0.1)
    for bad, text in (({'tau': 0}, 'tau: positive'), ({'tau': -1}, 'tau: positive'), ({'tau': float('inf')}, 'tau: positive'),
                      ({'margin': -0.1}, 'margin: non-negative'), ({'margin': float('inf')}, 'margin: non-negative'),
                      ({'rays': -1}, r'rays: in \[0, 2\^24\]'), ({'rays': (1 << 24) + 1}, r'rays: in \[0, 2\^24\]'),
                      ({'max_rays': 0}, r'max_rays: in \[1, 2\^24\]')):
        with pytest.raises(ValueError, match=r'model\.loss\.freespace\.' + text):
            parse_freespace_config(bad)
    with pytest.raises(ValueError, match='not one of'):
        _model(dict(LOSS, freespace_weight=1, freespace={'weight': 2}))
    assert 'NOT' in parse_freespace_config.__doc__ and 'design choices' in parse_freespace_config.__doc__


def test_loss_names_and_the_gate_of_the_fast_paths():
    plain, zero, on = _model(dict(LOSS)), _model(dict(LOSS, freespace_weight=0, freespace={'tau': 0.2})), _model(dict(LOSS, freespace_weight=0.5))
    assert plain.loss_names == zero.loss_names == ['loss_rgb', 'loss_parsimony', 'loss_tv', 'loss_overlap', 'loss_total']
    assert 'freespace' not in plain.loss_weights and 'freespace' not in zero.loss_weights and zero.freespace_cfg['tau'] == 0.2
    assert on.loss_names == ['loss_rgb', 'loss_parsimony', 'loss_tv', 'loss_overlap', 'loss_freespace', 'loss_total']
    assert on.loss_weights['freespace'] == 0.5 and on.freespace_cfg == FREESPACE_DEFAULTS
    both = _model(dict(LOSS, surface_weight=1, freespace_weight=0.5))
    assert both.loss_names[-3:] == ['loss_surface', 'loss_freespace', 'loss_total']
    assert phase.fast_path_refusal(plain) is None and phase.fast_path_refusal(zero) is None
    assert phase.fast_path_refusal(on) == 'a free-space term' and phase.fast_path_refusal(both) == 'a surface term'
    from dbw_amd.native_step import NativeStep
    on.sync_free = plain.sync_free = True
    assert NativeStep.supported(types.SimpleNamespace(m=plain)) and not NativeStep.supported(types.SimpleNamespace(m=on))


def test_a_weight_without_rays_raises_when_a_loss_is_asked_for():
    m = _model({'rgb_weight': 1, 'freespace_weight': 1})
    imgs = torch.rand(1, 3, 16, 24)
    with pytest.raises(RuntimeError, match=r'freespace_weight > 0 needs the capture.s depth rays: model\.set_freespace_rays'):
        m.compute_losses(imgs, imgs.clone())
    assert set(_model({'rgb_weight': 1}).compute_losses(imgs, imgs.clone())) == {'rgb', 'total'}
    m.set_freespace_rays(torch.rand(10, 3), torch.zeros(10, dtype=torch.int32), torch.ones(1, 3))
    with pytest.raises(RuntimeError, match='the free-space term reads the vertices of the scene the forward built'):
        m.compute_losses(imgs, imgs.clone())
    m.eval()
    ev = m.compute_losses(imgs, imgs.clone())
    assert list(ev) == ['rgb', 'freespace', 'total'] and float(ev['freespace']) == 0.0       # an evaluation does not count the term
    m.train()
    m.world_size = 2
    with pytest.raises(NotImplementedError, match='the free-space term under data parallelism'):
        m.compute_losses(imgs, imgs.clone())


def test_the_rays_are_thinned_and_stay_out_of_checkpoints():
    m = _model(dict(LOSS, freespace_weight=1, freespace={'max_rays': 100}))
    p = torch.randn(1000, 3)
    f = (torch.arange(1000) % 4).to(torch.int32)
    o = torch.randn(4, 3)
    p[5, 1] = float('nan')
    f[7] = 4
    f[9] = -1
    assert m.set_freespace_rays(p, f, o) == 100
    assert m._freespace_ends.shape == (100, 3) and m._freespace_ends.dtype == torch.float32 and m._freespace_frame.dtype == torch.int32
    first, first_f = m._freespace_ends.clone(), m._freespace_frame.clone()
    assert bool(torch.isfinite(first).all()) and not torch.equal(first, p[:100]) and int(first_f.min()) >= 0 and int(first_f.max()) <= 3
    rows = {tuple(r.tolist()) + (int(k),) for r, k in zip(p, f)}
    assert all(tuple(r.tolist()) + (int(k),) in rows for r, k in zip(first, first_f))           # an end keeps its frame
    assert m.set_freespace_rays(p.numpy(), f.numpy(), o.numpy()) == 100 and torch.equal(m._freespace_ends, first)    # the same permutation every time
    assert m.set_freespace_rays(p[:50], f[:50], o) == 47
    assert torch.equal(m._freespace_origins, o) and not any('freespace' in k for k in m.state_dict())
    with pytest.raises(ValueError, match='no finite ray'):
        m.set_freespace_rays(torch.full((3, 3), float('nan')), torch.zeros(3, dtype=torch.int32), o)
    with pytest.raises(ValueError, match='2 frames for 3 ends'):
        m.set_freespace_rays(torch.zeros(3, 3), torch.zeros(2, dtype=torch.int32), o)


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
    toy.loss_weights = {'rgb': 1.0, 'freespace': 1.0}
    with pytest.raises(NotImplementedError, match=r'model\.loss\.freespace_weight under data parallelism'):
        Trainer(_cfg(), toy, _views())


def test_the_flag_and_the_shipped_config(tmp_path):
    cfg_file = tmp_path / 'c.yml'
    cfg_file.write_text('dataset: {name: custom, tag: x}\nmodel: {loss: {perceptual_weight: 0, freespace: {tau: 0.05}}}\n')
    (tmp_path / 'default.yml').write_text('training: {batch_size: 2}\n')
    base = ['-c', str(cfg_file), '-t', 't', '--data-root', 'd', '--runs-root', 'r']
    assert 'freespace_weight' not in train.prepare_config(train.parse_args(base))['model']['loss']
    cfg = train.prepare_config(train.parse_args(base + ['--freespace', '0.25']))
    assert cfg['model']['loss']['freespace_weight'] == 0.25 and cfg['model']['loss']['freespace'] == {'tau': 0.05}
    here = os.path.dirname(os.path.abspath(__file__))
    cfg = DS.load_config(os.path.join(here, '..', 'differentiable-blocksworld_amd', 'configs', 'custom_freespace.yml'))
    assert cfg['dataset']['name'] == 'custom' and cfg['dataset']['cloud'] == 'depth' and cfg['model']['loss']['freespace_weight'] == 1
    assert parse_freespace_config(cfg['model']['loss']['freespace']) == FREESPACE_DEFAULTS
    assert train.wants_world_frame(cfg) and train.blocks_init_options(cfg) == {}
    m = _model(cfg['model']['loss'])
    assert m.loss_names[-3:] == ['loss_surface', 'loss_freespace', 'loss_total']


@pytest.fixture(scope='module')
def capture(tmp_path_factory):
    root = tmp_path_factory.mktemp('rays')
    depth, metres, c2w = DF.write_depth_capture(root, 'cap')                                # a pinhole: target pixel and source pixel coincide
    CF.write_capture(root, 'file', with_points=True)
    return root, depth, c2w


def test_the_scene_hands_its_rays_over_or_is_refused(capture, capsys):
    root, depth, _ = capture
    m = _model(dict(LOSS, freespace_weight=2))
    plain = DS.CustomScene(root, 'file', 'train')
    assert train.resolve_freespace(plain, _model(dict(LOSS)), 'cpu') is None               # no weight: nothing is asked
    with pytest.raises(ValueError, match=r"'file': no depth rays \(dataset\.cloud: depth"):
        plain.rays()
    with pytest.raises(SystemExit, match=r"model\.loss\.freespace_weight: 'file': no depth rays \(dataset\.cloud: depth"):
        train.resolve_freespace(plain, m, 'cpu')
    for name in ('dtu', 'bmvs'):
        with pytest.raises(SystemExit, match=f"freespace_weight is for custom scenes with depth maps: a '{name}' scene ships none"):
            train.resolve_freespace(types.SimpleNamespace(name=name, rays=lambda d: None), m, 'cpu')
    scene = DS.CustomScene(root, 'cap', 'train', cloud='depth')
    n = train.resolve_freespace(scene, m, 'cpu')
    assert scene._rays == {} and scene.rays_info['rays'] == n                             # the scene's own copy is given back
    ends, frame, origins = scene.rays('cpu')
    assert n == len(ends) == scene.rays_info['rays'] and torch.equal(m._freespace_ends, ends) and torch.equal(m._freespace_frame, frame)
    assert torch.equal(m._freespace_origins, origins) and scene.rays()[0] is scene.rays()[0]                       # built once
    assert f'freespace: weight 2 on {n} of {n} rays of 6 frames, 16384 a step, tau 0.1, margin 0.02, from epoch 1' in capsys.readouterr().out
    assert origins.shape == (6, 3) and torch.equal(origins, scene.cam2world[:, :3, 3].float())                        # the camera centres


def test_the_rays_of_the_analytic_capture_end_on_its_surfaces_and_cross_no_box(capture):
    """Every ray end lies on the ground plane or a box face within the depth quantum -- half a depth step along the optical axis, which is
    l / z of it along the ray (plus 1e-5 m for the fp32 of the poses) --, and no ray's first hit with the two analytic boxes, as meshes,
    lies more than that in front of its end."""
    root, depth, c2w = capture
    scene = DS.CustomScene(root, 'cap', 'train', cloud={'edge': 0.0})
    ends, frame, origins = (t.numpy() for t in scene.rays())
    # without the edge rule every measurement inside the default range of 0.1 .. 10 m is a ray
    assert len(ends) == int(((depth >= 100) & (depth <= 10000)).sum()) and set(frame.tolist()) == set(range(6))
    S = scene.scale_mat.double().numpy()
    to_file = lambda p: np.asarray(p, np.float64) @ S[:3, :3].T + S[:3, 3]        # noqa: E731
    P, O = to_file(ends), to_file(origins)
    assert np.abs(O - c2w[:, :3, 3]).max() < 1e-5
    e = P - O[frame]
    l = np.linalg.norm(e, axis=1)
    z = -(e * c2w[frame, :3, 2]).sum(1)                                                    # along the optical axis (OpenGL: -z)
    quantum = 0.5 * DF.UNIT * l / z + 1e-5
    off = DF.surface_distance(P)
    print(f'{len(P)} rays: off the surfaces by at most {off.max():.2e} m ({(off / quantum).max():.3f} of the quantum)')
    assert (z > 0).all() and (off <= quantum).all()
    # the two boxes as meshes of 12 faces each, in the normalised frame; margin 0
    F = np.linalg.inv(S)
    s = float(np.cbrt(np.linalg.det(F[:3, :3])))
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    verts, faces = [], []
    for lo, hi in DF.BOXES:
        c = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
        faces += [[len(verts) * 8 + q[a], len(verts) * 8 + q[b], len(verts) * 8 + q[c_]] for q in quads for a, b, c_ in ((0, 1, 2), (0, 2, 3))]
        verts.append(c @ F[:3, :3].T + F[:3, 3])
    verts, faces = np.concatenate(verts), np.array(faces, np.int32)
    h = FR.first_hits(ends, frame, origins, verts, faces, None, tau=0.1, margin=0.0)
    hit = h['face'] >= 0
    in_front = np.where(hit, h['g'], 0.0) / s                                              # metres in front of the end
    print(f'{hit.sum()} of the rays meet a box before their end, at most {in_front.max():.2e} m in front of it')
    assert hit.sum() > 100 and (in_front <= quantum).all()
    sc = dict(verts=verts.astype(np.float32), faces=faces, face_group=np.array([0, 12, 24], np.int32), group_keep=None)
    rec, psi = FR.host_records(ends, frame, origins, sc, 0, 1, 2, 0.1, 0.0, cull=1)
    t32, face32 = rec[:, 0].view(np.float32), rec[:, 1].astype(np.int32)
    g32 = np.where(face32 >= 0, (1 - np.nan_to_num(t32)) * np.linalg.norm(ends - origins[frame], axis=1), 0.0) / s
    assert (g32 <= quantum + 1e-5).all()                                                   # the host build of the kernel's header agrees


@pytest.mark.parametrize('kind', DR.KINDS)
def test_the_numpy_path_gives_the_bytes_of_the_host_build(kind):
    for N, H, W, stride, permille in ((17, 37, 67, 1, 0), (3, 24, 32, 3, 50), (2, 1, 1, 1, 0), (2, 5, 7, 3, 50)):
        depth, cams, target, poses = DR.case(N, H, W, kind)
        bx = DR.box(-2.0, 2.0, 8)
        want, cell = FR.host_depth_rays(depth, cams, target, poses, 1, 65535, stride, permille, box=bx, G=8)
        got = ops.depth_rays_host(depth, cams, target, poses, stride=stride, edge=permille / 1000)
        assert got.dtype == np.int32 and got.shape == want.shape and got.view(np.uint32).tobytes() == want.tobytes(), (kind, N, H, W)
        frame = got[..., 3]
        assert np.array_equal(frame >= 0, cell != -1)                                     # dropped exactly where depth_sample drops before its cube
        # ... and inside the cube the end is the point depth_sample quantises: the same cell
        cell2, q = DR.samples_host(depth, cams, target, poses, bx, 8, 1, 65535, stride, permille)
        inside = cell2 >= 0
        p = got[..., :3].view(np.float32)[inside]
        f = np.floor((p - bx[:3]) * bx[3]).astype(np.int64)
        assert np.array_equal(f, q[inside])
        ends, fr = ops.depth_rays_compact(got)
        assert ends.shape == (int((frame >= 0).sum()), 3) and torch.equal(fr, torch.from_numpy(frame[frame >= 0]))
    with pytest.raises(TypeError, match='uint16'):
        ops.depth_rays_host(np.zeros((1, 2, 2), np.float32), cams[:1], target, poses[:1])
