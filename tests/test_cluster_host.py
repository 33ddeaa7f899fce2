"""CPU: eval3d.cluster_points_torch against the numpy restatement of tests/cluster_ref.py round for round, worldfit.blocks_from_points
through the torch path on the three-box fixture, model.init_blocks, the refusals, and the training.blocks_init logic of dbw_amd/train.py as
far as it runs without a device."""
import types

import numpy as np
import pytest
import torch
import yaml

import cluster_ref as CR
import dbw_amd
from dbw_amd import eval3d, mesh, train, worldfit as W


def _np(res):
    return {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in res._asdict().items()}


@pytest.mark.parametrize('cloud', ['lattice', 'random'])
def test_torch_path_equals_the_restatement_round_for_round(cloud):
    if cloud == 'lattice':
        p, init = CR.lattice_cloud(4)
        p = p.copy()
        p[5, 0], p[9, 2] = np.nan, np.inf
    else:
        p = CR.random_cloud(2000, 6)
        init = p[::300][:7].copy()
    K = len(init)
    ref = CR.np_fit(p, K, n_iter=3, init=init)
    for r, want in enumerate(ref):
        got = _np(eval3d.cluster_points(torch.from_numpy(p), K, n_iter=r, init=init))
        assert np.array_equal(got['labels'], want['labels']) and np.array_equal(got['counts'], want['counts']), r
        assert got['labels'].dtype == np.int32 and int(got['rounds']) == r and int(got['n_nonempty']) == int((want['counts'] > 0).sum())
        assert int(got['changed']) == (len(p) if r == 0 else int((ref[r - 1]['labels'] != want['labels']).sum()))
        if cloud == 'lattice':
            assert (got['labels'][[5, 9]] == -1).all() and got['counts'].sum() == len(p) - 2
            if r == 0:                                             # integer terms about integer centres: every sum is exact
                assert np.array_equal(got['mean'], want['mean'])
        assert CR.ulp_diff(got['centres'], want['centres']).max() <= (0 if r <= 1 and cloud == 'lattice' else 1)
        assert np.abs(got['mean'] - want['mean']).max() <= 1e-12
        assert np.abs(got['cov'] - want['cov']).max() <= 1e-12
        for k in range(K):
            if want['counts'][k] >= 2 and np.linalg.norm(want['cov'][k]) > 0:
                A = want['cov'][k][[0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(3, 3)
                for i in range(3):
                    assert np.linalg.norm(A @ got['axes'][k, i] - got['evals'][k, i] * got['axes'][k, i]) <= 1e-12 * max(1, np.linalg.norm(A))
                assert abs(np.linalg.det(got['axes'][k]) - 1) <= 1e-12
            elif want['counts'][k] < 2:
                assert np.array_equal(got['axes'][k], np.eye(3)) and not got['evals'][k].any()


def test_seeding_order_is_exact():
    for p, K in ((CR.lattice_cloud(2)[0], 12), (CR.random_cloud(777, 8), 16)):
        p = p.copy()
        p[3] = np.nan
        want, _ = CR.np_seed(p, K)
        got = eval3d.cluster_points(torch.from_numpy(p), K, n_iter=0)
        assert np.array_equal(got.centres.numpy(), want) and np.array_equal(CR.host_seed(p, K)[0], want)
    p = np.repeat(np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0]], np.float32), 5, axis=0)
    got = eval3d.cluster_points(torch.from_numpy(p), 5, n_iter=2)
    assert got.counts.tolist() == [5, 5, 5, 0, 0] and np.array_equal(got.centres.numpy(), CR.host_fit(p, 5, n_iter=2)['centres'])
    with pytest.raises(ValueError, match='1 <= k <= 256'):
        eval3d.cluster_points(torch.zeros(5, 3), 6)
    with pytest.raises(ValueError, match='1 <= k <= 256'):
        eval3d.cluster_points(torch.zeros(500, 3), 257)
    with pytest.raises(ValueError, match='n_iter'):
        eval3d.cluster_points(torch.zeros(5, 3), 2, n_iter=65)
    with pytest.raises(ValueError, match=r'init \(k,3\)'):
        eval3d.cluster_points(torch.zeros(5, 3), 2, init=torch.zeros(3, 3))


def _fit_boxes(fx, n_blocks=3, **kw):
    w = CR.BOX_WORLD
    return W.blocks_from_points(torch.from_numpy(fx['points']), w['S_world'], fx['matrix'], w['T_world'], n_blocks,
                                cluster=eval3d.cluster_points_torch, **kw)


def check_boxes(init, fx, order=(0, 1, 2), lam_rel=1e-6):
    """a BlockInit against the three-box fixture: block i is box order[i]"""
    tol = CR.scene_rounding(fx['points'])
    ratio, scale_min = 0.25, 0.2
    assert init.index.tolist() == list(range(len(order))) and init.counts.tolist() == [CR.BOX_M[b] ** 3 for b in order]
    for i, b in enumerate(order):
        err = np.abs(init.T[i].double().cpu().numpy() - CR.BOX_CENTRES[b]).max()
        assert err <= tol, (i, err, tol)                           # the mean of a symmetric grid is its centre
        R = mesh.rotation_6d_to_matrix(init.R_6d[i:i + 1])[0].double().cpu().numpy()
        # axes up to sign: |R rot^T| is the identity (the largest extent on block axis 0); the slack is that of an eigenvector of a covariance
        # perturbed by tol * extent, over the smallest eigenvalue gap
        gap = min(fx['lam'][b][0] - fx['lam'][b][1], fx['lam'][b][1] - fx['lam'][b][2])
        turn = 8 * tol * CR.BOX_HALF[b].max() / gap + 8 * 2.0 ** -24
        assert np.abs(np.abs(R @ fx['rot'][b].T) - np.eye(3)).max() <= turn, (i, turn)
        assert abs(np.linalg.det(R) - 1) <= 1e-5
        # S encodes the half-extent sqrt(3 lambda) with the analytic lambda = a^2 / 3 (m + 1) / (m - 1)
        half = ratio * (np.exp(init.S[i].double().cpu().numpy()) + scale_min)
        want = np.sqrt(3 * fx['lam'][b])
        assert np.abs(half / want - 1).max() <= lam_rel + 8 * tol * CR.BOX_HALF[b].max() / fx['lam'][b].min(), (i, half, want)


def test_blocks_from_three_boxes():
    fx = CR.three_boxes()
    init = _fit_boxes(fx, oversample=1)
    assert init.n_points_used == len(fx['points']) and init.n_blocks == 3 and len(init) == 3
    check_boxes(init, fx)
    d = yaml.safe_load(init.yaml())
    assert d['index'] == [0, 1, 2] and d['counts'] == [512, 343, 216] and np.allclose(d['T'], init.T.numpy()) and len(d['S']) == 3
    # the fit is a function of the cloud alone
    again = _fit_boxes(fx, oversample=1)
    assert all(torch.equal(getattr(init, k), getattr(again, k)) for k in ('T', 'R_6d', 'S', 'index', 'counts'))
    # fewer good clusters than blocks: the tail is not in index
    two = _fit_boxes(fx, oversample=1, min_points=300)
    assert two.index.tolist() == [0, 1] and two.counts.tolist() == [512, 343] and torch.equal(two.T, init.T[:2])
    # the clamp of the size: a range that no box fits
    big = _fit_boxes(fx, oversample=1, size_range=(2.0, 3.0))
    assert torch.equal(big.S, torch.full((3, 3), float(np.float32(np.log(2.0 - 0.2)))))


def test_stray_points_take_the_spare_centres():
    fx = CR.three_boxes(n_outliers=3)
    init = _fit_boxes(fx, oversample=2)
    assert init.n_points_used == len(fx['points'])
    check_boxes(init, fx)
    # without the spare centres the stray points cost a box its centre
    bare = _fit_boxes(fx, oversample=1)
    assert bare.counts.tolist() != [512, 343, 216]
    # points below the ground margin or outside the bound are not clustered
    w = CR.BOX_WORLD
    junk = np.array([[0.0, -0.88, 0.0], [2.5, 0.0, 0.0], [0.0, 3.5, 0.0], [0.0, 0.0, -2.5]])
    pts = np.concatenate([fx['points'], ((junk * w['S_world']) @ fx['matrix'] + np.array(w['T_world'])).astype(np.float32)])
    more = W.blocks_from_points(torch.from_numpy(pts), w['S_world'], fx['matrix'], w['T_world'], 3, oversample=2, cluster=eval3d.cluster_points_torch)
    assert more.n_points_used == len(fx['points']) and torch.equal(more.T, init.T)


def _cfg(n_blocks=5, **training):
    return {'model': {'name': 'dbw', 'mesh': dict(n_blocks=n_blocks, txt_size=8, **CR.BOX_WORLD),
                      'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                      'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True, 'opacity_noise': False},
                      'loss': {'rgb_weight': 1, 'perceptual_weight': 0, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}},
            'training': dict(training)}


def _model(n_blocks=5, seed=7):
    torch.manual_seed(seed)
    return dbw_amd.create_model(_cfg(n_blocks), (16, 24))


def test_model_init_blocks():
    fx = CR.three_boxes(n_outliers=2)
    plain, model = _model(), _model()
    assert model.T_range == (1.0, 1.0, 1.0) and all(torch.equal(a, b) for a, b in zip(plain.state_dict().values(), model.state_dict().values()))
    ptrs = [p.data_ptr() for p in (model.T, model.R_6d, model.S)]
    init = model.init_blocks_from_points(torch.from_numpy(fx['points']), oversample=1, cluster=eval3d.cluster_points_torch)
    check_boxes(init, fx)                                          # five centres: one box each, one stray point each
    assert ptrs == [p.data_ptr() for p in (model.T, model.R_6d, model.S)]                  # in place
    for name in ('T', 'R_6d', 'S'):
        got, was = getattr(model, name).detach(), getattr(plain, name).detach()
        assert torch.equal(got[:3], getattr(init, name)) and torch.equal(got[3:], was[3:]) and not torch.equal(got[:3], was[:3])
    others = [k for k in plain.state_dict() if k not in ('T', 'R_6d', 'S')]
    assert all(torch.equal(plain.state_dict()[k], model.state_dict()[k]) for k in others)
    # given rows, other slots
    model.init_blocks(init.T[:1], init.R_6d[:1], init.S[:1], index=[4])
    assert torch.equal(model.T.detach()[4], init.T[0]) and torch.equal(model.T.detach()[3], plain.T.detach()[3])
    with pytest.raises(ValueError, match='outside'):
        model.init_blocks(init.T[:1], init.R_6d[:1], init.S[:1], index=[5])
    with pytest.raises(ValueError, match='expected'):
        model.init_blocks(init.T, init.R_6d[:2], init.S)


def test_refusals(tmp_path):
    import worldfit_fixture as WF
    from dbw_amd import dataset as DS
    fx = CR.three_boxes()
    w = CR.BOX_WORLD
    with pytest.raises(ValueError, match=f'at least {W.MIN_POINTS} points above the ground'):
        W.blocks_from_points(torch.from_numpy(fx['points'][:50]), w['S_world'], fx['matrix'], w['T_world'], 3)
    with pytest.raises(ValueError, match=f'at least {W.MIN_POINTS} points above the ground'):      # all of them under the ground
        W.blocks_from_points(torch.from_numpy(fx['points']), w['S_world'], fx['matrix'], w['T_world'], 3, ground_margin=5.0)
    with pytest.raises(ValueError, match=r'points \(N,3\)'):
        W.blocks_from_points(torch.zeros(10, 2), 1.0, np.eye(3), [0, 0, 0], 3)
    cap = WF.capture(2)
    WF.write_capture(tmp_path, 'bare', cap, with_points=False)
    with pytest.raises(ValueError, match='no point cloud'):
        DS.CustomScene(tmp_path, 'bare', 'train').block_init(_model())
    # a capture with a cloud: the scene hands its own cloud to the model
    WF.write_capture(tmp_path, 'cap', cap)
    scene = DS.CustomScene(tmp_path, 'cap', 'train')
    fr = scene.world_frame()
    torch.manual_seed(1)
    cfg = _cfg(4)
    cfg['model']['mesh'].update(fr.mesh_kwargs())
    model = dbw_amd.create_model(cfg, scene.img_size)
    init = scene.block_init(model, min_points=20, cluster=eval3d.cluster_points_torch)
    assert 1 <= len(init) <= 4 and torch.equal(model.T.detach()[:len(init)], init.T)
    # the box of the capture stands on the ground under the cameras: the first block starts inside the scene
    assert float(init.T[0].abs().max()) <= 2.0 and init.n_points_used >= W.MIN_POINTS


def test_blocks_init_of_a_config(tmp_path, capsys):
    assert train.blocks_init_options({}) is None and train.blocks_init_options(_cfg()) is None
    assert train.blocks_init_options(_cfg(blocks_init=None)) is None and train.blocks_init_options(_cfg(blocks_init=False)) is None
    assert train.blocks_init_options(_cfg(blocks_init='points')) == {}
    opts = dict(oversample=3, min_points=10, n_iter=5, ground_margin=0.1, extent_scale=1.5)
    assert train.blocks_init_options(_cfg(blocks_init=opts)) == opts
    with pytest.raises(SystemExit, match="neither 'points' nor a mapping"):
        train.blocks_init_options(_cfg(blocks_init='cloud'))
    with pytest.raises(SystemExit, match='blocks_init.bound: not one of'):
        train.blocks_init_options(_cfg(blocks_init={'bound': 3}))
    # the command line sets the key, and leaves a mapping of the config alone
    args = train.parse_args(['-c', 'x.yml', '-t', 't', '--data-root', 'd', '--runs-root', 'r', '--blocks-init', 'points'])
    assert args.blocks_init == 'points'
    with pytest.raises(SystemExit):
        train.parse_args(['-c', 'x.yml', '-t', 't', '--data-root', 'd', '--runs-root', 'r', '--blocks-init', 'random'])
    # absent: nothing happens, the scene is not asked
    untouched = types.SimpleNamespace(name='custom', block_init=lambda *a, **k: pytest.fail('fitted without being asked'))
    assert train.resolve_blocks_init(_cfg(), untouched, None, 'cpu') is None
    # DTU / BlendedMVS: refused with the reason
    with pytest.raises(SystemExit, match="cloud of a 'dtu' scene is the ground truth"):
        train.resolve_blocks_init(_cfg(blocks_init='points'), types.SimpleNamespace(name='dtu'), None, 'cpu')
    # a scene without a cloud: the reason is passed on
    def no_cloud(model, device, **kw):
        raise ValueError("'x': no point cloud")
    with pytest.raises(SystemExit, match='training.blocks_init: .*no point cloud'):
        train.resolve_blocks_init(_cfg(blocks_init='points'), types.SimpleNamespace(name='custom', block_init=no_cloud), None, 'cpu')
    # the fit is applied, printed and written; the options of the mapping reach it
    fx = CR.three_boxes(n_outliers=2)
    asked = {}

    def block_init(model, device, **kw):
        asked.update(device=device, **kw)
        return model.init_blocks_from_points(torch.from_numpy(fx['points']), cluster=eval3d.cluster_points_torch, **kw)
    model, plain = _model(), _model()
    scene = types.SimpleNamespace(name='custom', block_init=block_init)
    init = train.resolve_blocks_init(_cfg(blocks_init={'oversample': 1, 'n_iter': 10}), scene, model, 'cpu', str(tmp_path))
    assert asked == dict(device='cpu', oversample=1, n_iter=10) and len(init) == 3
    assert torch.equal(model.T.detach()[:3], init.T) and torch.equal(model.T.detach()[3:], plain.T.detach()[3:])
    written = yaml.safe_load((tmp_path / 'blocks_init.yml').read_text())
    assert written == init.as_dict() and written['index'] == [0, 1, 2] and written['n_blocks'] == 5
    assert 'blocks_init: points -> 3 of 5 blocks seeded from 1073 points' in capsys.readouterr().out
    # a resumed or pretrained start does not fit again
    model2 = _model()
    assert train.resolve_blocks_init(_cfg(blocks_init='points'), untouched, model2, 'cpu', str(tmp_path / 'none'), start='runs/x/model.pkl') is None
    assert torch.equal(model2.T, plain.T) and 'skipped, runs/x/model.pkl carries the blocks' in capsys.readouterr().out
