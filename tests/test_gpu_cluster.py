"""GPU tests of the k-means / PCA fit (csrc/cluster_fit.hip, dbw_eval_cluster_fit of include/dbw_eval.h) and of the block initialisation on top
of it.  `-m gpu`.

Bounds.  Labels, counts and the seeding order are integer results of fp32 arithmetic that the kernels and the host build
(tests/host_cluster_math.cpp) compile from one header with one rounding per operation: they are compared for equality.  The ten sums of a
cluster add the same exact terms in another order than the host does (the device: lane by lane, by shuffle tree, by wave, by workgroup); they
are held to 8 eps64 sum|term| per sum against fp64 numpy (cluster_ref.np_moments), through the mean and the covariance the call reports: see
_moment_bounds.  A centre is the fp64 mean rounded once to fp32: equal bytes after one round from the same centres, where the two means differ
by far less than an fp32 ulp (the one-round test asserts equality, as the host-build comparison does elsewhere in this project); the chained
test allows the one ulp of a rounding boundary."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cluster_ref as CR                                        # noqa: E402
import worldfit_fixture as WF                                   # noqa: E402
from dbw_amd import create_model, eval3d, mesh, train          # noqa: E402
from dbw_amd import worldfit as W                               # noqa: E402
from test_cluster_host import _cfg, check_boxes                 # noqa: E402

DEV = 'cuda'
TILE = 1024                                                      # csrc/cluster_fit.hip: CL_TILE, the points of one workgroup's tile
OUTPUTS = ('centres', 'labels', 'counts', 'mean', 'cov', 'evals', 'axes', 'info')


def _device_fit(pts, K, n_iter=0, init=None):
    o = eval3d.cluster_fit(torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).to(DEV), K, n_iter,
                           None if init is None else torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32)).to(DEV))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _moment_bounds(p, c, labels):
    """fp64 numpy mean and covariance of every cluster about the centres c, and what the device's may differ by: with b = 8 eps64 sum|term|
    the bound of each of the ten sums and n the count, m = sum d / n is within b / n, the mean c + m within that plus one rounding, and
    cov = sum d d^T / n - m_a m_b within b_dd / n + (|m_a| b_b + |m_b| b_a) / n plus the roundings of the three operations."""
    sums, b = CR.np_moments(p, c, labels)
    _, mean, cov, counts = CR.np_finish(sums, c)
    n = np.maximum(sums[:, :1], 1)
    m, bm = sums[:, 1:4] / n, b[:, 1:4] / n
    mean_b = bm + 2 * CR.EPS64 * (np.abs(c.astype(np.float64)) + np.abs(m))
    cov_b = np.stack([b[:, 4 + i] / n[:, 0] + np.abs(m[:, a_]) * bm[:, b_] + np.abs(m[:, b_]) * bm[:, a_]
                      + 4 * CR.EPS64 * (np.abs(sums[:, 4 + i]) / n[:, 0] + np.abs(m[:, a_] * m[:, b_])) for i, (a_, b_) in enumerate(CR.PAIRS)], 1)
    return mean, mean_b, cov, cov_b, counts


def _check_against_host(d, h, p, tag):
    assert h['rc'] == 0
    assert np.array_equal(d['labels'], h['labels']) and np.array_equal(d['counts'], h['counts']), tag
    assert d['centres'].tobytes() == h['centres'].tobytes(), tag
    assert d['info'].tolist() == h['info'].tolist(), tag
    mean, mean_b, cov, cov_b, counts = _moment_bounds(p, d['centres'], d['labels'])
    assert np.array_equal(counts, d['counts']), tag
    e_mean, e_cov = np.abs(d['mean'] - mean), np.abs(d['cov'] - cov)
    assert (e_mean <= mean_b).all() and (e_cov <= cov_b).all(), (tag, float((e_mean / mean_b).max()), float(np.max(e_cov / np.maximum(cov_b, 1e-300))))
    for k in np.flatnonzero(d['counts'] >= 2)[:8]:
        CR.check_eigen(d['cov'][k], d['evals'][k], d['axes'][k], tag)
    few = d['counts'] < 2
    assert not d['cov'][few].any() and not d['evals'][few].any() and (d['axes'][few] == np.eye(3)).all(), tag


@pytest.mark.parametrize('N', [1, 63, 64, 65, 255, 257, TILE - 1, TILE, TILE + 1, 5000])
def test_one_round_equals_the_host_build(N):
    """The wave (64), the workgroup (256), the tile and the group of 64 centres; n_iter = 0 is the final pass alone, n_iter = 1 one round."""
    rng = np.random.RandomState(N)
    p = CR.random_cloud(N, 100 + N)
    for K in (1, 2, 63, 64, 65, 256):
        if K > N:
            continue
        init = (p[rng.choice(N, K, replace=False)] + rng.randn(K, 3).astype(np.float32) * 0.05).astype(np.float32)
        for n_iter in (0, 1):
            d, h = _device_fit(p, K, n_iter, init), CR.host_fit(p, K, n_iter, init)
            _check_against_host(d, h, p, (N, K, n_iter))
            if n_iter == 0:
                assert d['centres'].tobytes() == init.tobytes() and d['info'].tolist()[:2] == [0, N]


def test_ties_and_non_finite_points_on_the_lattice():
    p, c = CR.lattice_cloud(3, n=3000, K=9)
    p = p.copy()
    bad = [0, 63, 64, 1023, 1024, 2999]
    p[bad, [0, 1, 2, 0, 1, 2]] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan]
    d, h = _device_fit(p, len(c), 0, c), CR.host_fit(p, len(c), 0, c)
    ref = CR.np_fit(p, len(c), 0, c)[-1]
    assert np.array_equal(d['labels'], ref['labels']) and (d['labels'][bad] == -1).all() and (np.delete(d['labels'], bad) >= 0).all()
    assert d['counts'].sum() == len(p) - len(bad) and np.array_equal(d['counts'], ref['counts'])
    assert not (d['labels'] == len(c) - 1).any()                   # the duplicated centre loses every tie
    # integer terms about integer centres: every sum is exact whatever its order, so the whole result is the host build's, byte for byte
    for k in OUTPUTS:
        assert d[k].tobytes() == h[k].tobytes(), k
    # after two rounds: the non-finite points are still out, and the labels are those of the device's own centres
    d = _device_fit(p, len(c), 2, c)
    h = CR.host_fit(p, len(c), 0, d['centres'])
    assert np.array_equal(d['labels'], h['labels']) and np.array_equal(d['counts'], h['counts']) and (d['labels'][bad] == -1).all()
    assert d['counts'].sum() == len(p) - len(bad) and d['info'][0] == 2
    D = CR.np_dist2(p, c)[CR.np_finite(p)]
    assert int(((D == D.min(1, keepdims=True)).sum(1) > 1).sum()) > 100      # ties really occur


def test_seeding_order_equals_the_host_reference():
    clouds = [(CR.lattice_cloud(2, n=3000)[0], 12), (CR.random_cloud(5000, 8), 64), (CR.random_cloud(1500, 9), 256),
              (np.repeat(np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0]], np.float32), 400, axis=0), 5)]
    for p, K in clouds:
        p = p.copy()
        p[3] = np.nan
        d = _device_fit(p, K, 0)
        want, order = CR.host_seed(p, K)
        assert d['centres'].tobytes() == want.tobytes() and np.array_equal(want, CR.np_seed(p, K)[0]), K
        h = CR.host_fit(p, K, 0)
        assert np.array_equal(d['labels'], h['labels']) and np.array_equal(d['counts'], h['counts']) and d['labels'][3] == -1
    # fewer distinct points than centres: the later centres repeat the first and stay empty
    assert order.tolist()[3:] == [0, 0] and d['counts'].tolist() == [399, 400, 400, 0, 0] and d['info'][2] == 3
    # no finite point: zero centres, no label
    d = _device_fit(np.full((70, 3), np.nan, np.float32), 3, 2)
    assert not d['centres'].any() and (d['labels'] == -1).all() and not d['counts'].any() and d['info'].tolist() == [2, 0, 0, 0]


def test_the_run_of_R_rounds_is_R_chained_single_rounds():
    """No comparison of two independently iterated trajectories: every link starts from the DEVICE's centres."""
    p, K, R = CR.random_cloud(5000, 12), 16, 5
    c = _device_fit(p, K, 0)['centres']                            # the seeding
    full = _device_fit(p, K, R)
    worst = 0
    for r in range(R):
        link = _device_fit(p, K, 1, c)
        h = CR.host_fit(p, K, 1, c)                                # one host round from the device's centres
        ulp = CR.ulp_diff(link['centres'], h['centres']).max()
        worst = max(worst, int(ulp))
        assert ulp <= 1, r                                         # the fp64 means differ within the bound of the sums, before the one rounding
        h0 = CR.host_fit(p, K, 0, link['centres'])                 # the labels of the link's last pass, against the device's new centres
        assert np.array_equal(link['labels'], h0['labels']) and np.array_equal(link['counts'], h0['counts']), r
        c = link['centres']
    print(f'chained run: worst centre difference device vs host over {R} links: {worst} ulp')
    for k in OUTPUTS:
        if k != 'info':
            assert full[k].tobytes() == link[k].tobytes(), k
    assert full['info'].tolist() == [R, link['info'][1], link['info'][2], 0]
    assert not np.array_equal(full['centres'], _device_fit(p, K, 0)['centres'])      # the rounds moved the centres


def test_the_same_call_gives_the_same_bytes():
    p = torch.from_numpy(CR.random_cloud(5000, 13)).to(DEV)
    first = {k: v.cpu().numpy().tobytes() for k, v in eval3d.cluster_fit(p, 65, 4).items()}
    again = {k: v.cpu().numpy().tobytes() for k, v in eval3d.cluster_fit(p, 65, 4).items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o = eval3d.cluster_fit(p, 65, 4)
    side.synchronize()
    other = {k: v.cpu().numpy().tobytes() for k, v in o.items()}
    for k in OUTPUTS:
        assert first[k] == again[k] == other[k], k
    res = eval3d.cluster_points(p, 65, n_iter=4)
    assert all(t.device.type == 'cuda' for t in res) and res.labels.cpu().numpy().tobytes() == first['labels'] and int(res.rounds) == 4
    with pytest.raises(ValueError, match='are refused'):            # sizes are refused before anything is launched
        eval3d.cluster_fit(p, 257)
    with pytest.raises(RuntimeError, match='n_iter must be in'):
        eval3d.cluster_fit(p, 8, 65)


def test_blocks_from_points_on_the_device_equals_the_torch_path():
    fx = CR.three_boxes()
    w = CR.BOX_WORLD
    pts = torch.from_numpy(fx['points'])
    ref = W.blocks_from_points(pts, w['S_world'], fx['matrix'], w['T_world'], 3, oversample=1, cluster=eval3d.cluster_points_torch)
    check_boxes(ref, fx)                                           # the reference side: every cluster is one whole box, so no label can differ
    dev = W.blocks_from_points(pts.to(DEV), w['S_world'], fx['matrix'], w['T_world'], 3, oversample=1)
    assert dev.T.device.type == 'cuda' and dev.counts.tolist() == ref.counts.tolist() == [512, 343, 216]
    check_boxes(dev, fx)
    tol = CR.scene_rounding(fx['points'])                          # the scene frame is computed in fp32 on either device
    assert float((dev.T.cpu() - ref.T).abs().max()) <= 2 * tol
    half = lambda b: 0.25 * (b.S.double().cpu().exp() + 0.2)       # noqa: E731
    rel = float((half(dev) / half(ref) - 1).abs().max())
    lam_slack = max(8 * tol * CR.BOX_HALF[b].max() / fx['lam'][b].min() for b in range(3))
    print(f'device vs torch path: centres {float((dev.T.cpu() - ref.T).abs().max()):.2e} (bound {2 * tol:.2e}), extents {rel:.2e} relative')
    assert rel <= 1e-6 + 2 * lam_slack
    # the device path on the same scene-frame points as the torch path: lambda within 1e-6 relative, means within fp32 rounding
    q = torch.from_numpy(fx['scene'].astype(np.float32))
    a, b = eval3d.cluster_points(q.to(DEV), 3, n_iter=20), eval3d.cluster_points_torch(q, 3, n_iter=20)
    assert torch.equal(a.labels.cpu(), b.labels) and torch.equal(a.centres.cpu(), b.centres)
    assert float((a.evals.cpu() / b.evals - 1).abs().max()) <= 1e-6 and float((a.mean.cpu() - b.mean).abs().max()) <= 2.0 ** -24


def _model(n_blocks=5, seed=7):
    torch.manual_seed(seed)
    return create_model(_cfg(n_blocks), (16, 24)).to(DEV)


def test_the_seeded_model_is_what_the_clusters_say():
    import oracle as O
    from dbw_amd.trainer import Trainer
    fx = CR.three_boxes(n_outliers=2)
    plain, model = _model(), _model()
    init = model.init_blocks_from_points(torch.from_numpy(fx['points']).to(DEV), oversample=1)
    check_boxes(init, fx)
    assert init.index.tolist() == [0, 1, 2]
    verts, faces = model.blocks_mesh(filter_transparent=False)
    V = verts.double().cpu().numpy().reshape(5, -1, 3)
    S_w, R_w, T_w = model._world_consts()
    R_w, T_w = R_w.double().cpu().numpy(), T_w.double().cpu().numpy()
    for i in range(3):
        T, S = init.T[i].double().cpu().numpy(), init.S[i].double().cpu().numpy()
        R = mesh.rotation_6d_to_matrix(init.R_6d[i:i + 1])[0].double().cpu().numpy()
        centre = (T * S_w) @ R_w + T_w
        half = 0.25 * (np.exp(S) + 0.2) * S_w
        # fp32: a posed vertex is a dozen operations on numbers below |T_world| + S_world (|T| + half-extent) -> 32 eps32 of that
        bound = 32 * 2.0 ** -24 * (np.abs(T_w).max() + S_w * (np.abs(T).max() + 1))
        # the icosphere's vertices come in antipodal pairs and the surface is symmetric: the centroid is the block's centre
        assert np.abs(V[i].mean(0) - centre).max() <= bound, i
        local = (V[i] - centre) @ R_w.T @ R.T                      # along the fitted axes
        ext = local.max(0) - local.min(0)
        # the level-1 icosphere has a vertex on each of the six axis directions, where the parametric surface reaches +-1 * ratio
        assert np.abs(ext - 2 * half).max() <= 2 * bound, (i, ext, 2 * half)
    for name in ('T', 'R_6d', 'S'):                                # unseeded blocks: bit-equal to the model of the same seed without the feature
        assert torch.equal(getattr(model, name).detach()[3:], getattr(plain, name).detach()[3:])
        assert torch.equal(getattr(model, name).detach()[:3], getattr(init, name))
    Vp = plain.blocks_mesh(filter_transparent=False)[0].reshape(5, -1, 3)
    assert torch.equal(verts.reshape(5, -1, 3)[3:], Vp[3:]) and not torch.equal(verts.reshape(5, -1, 3)[:3], Vp[:3])
    for k, v in plain.state_dict().items():
        if k not in ('T', 'R_6d', 'S'):
            assert torch.equal(v, model.state_dict()[k]), k
    # a Trainer built afterwards starts from the seeded parameters, and a step runs
    R, T, K = O.synthetic_cameras(2, R_world=model.R_world[0].cpu())
    g = torch.Generator().manual_seed(0)
    views = {'imgs': torch.rand(2, 3, 16, 24, generator=g).to(DEV), 'R': R.to(DEV), 'T': T.to(DEV), 'K': K.to(DEV)}
    cfg = {'training': {'batch_size': 2, 'n_epoches': 1, 'seed': 3, 'optimizer': {'name': 'adam', 'lr': 1e-3}, 'scheduler': {'name': 'multi_step'}}}
    tr = Trainer(cfg, model, views)
    flat = tr.step_fn.params
    for name, off, k in flat.names:
        if name in ('T', 'R_6d', 'S'):
            got = flat.flat[off:off + k].reshape(5, -1)
            assert torch.equal(got[:3], getattr(init, name)) and torch.equal(got[3:], getattr(plain, name).detach()[3:]), name
            assert getattr(model, name).data_ptr() == flat.flat[off:off + k].data_ptr()
    out = tr.run_epoch()
    torch.cuda.synchronize()
    assert np.isfinite(float(out['total'])) and not torch.equal(model.T.detach()[:3], init.T)       # the step moved the seeded blocks


def test_the_command_line_seeds_the_blocks(tmp_path, capsys):
    import yaml
    cap = WF.capture(2)
    WF.write_capture(tmp_path, 'cap', cap)
    cfg = {'dataset': {'name': 'custom', 'tag': 'cap'},
           'model': {'name': 'dbw', 'mesh': {'n_blocks': 3, 'R_world': 'auto', 'T_world': 'auto', 'S_world': 'auto', 'txt_size': 16},
                     'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                     'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True,
                                    'opacity_noise': False},
                     'loss': {'rgb_weight': 1, 'perceptual_weight': 0.1, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}},
           'training': {'batch_size': 2, 'n_epoches': 3, 'seed': 3, 'optimizer': {'name': 'adam', 'lr': 1e-3}, 'scheduler': {'name': 'multi_step'}}}
    path = tmp_path / 'cap.yml'
    with open(path, 'w') as f:
        yaml.safe_dump(cfg, f)
    common = ['--config', str(path), '--tag', 'run', '--data-root', str(tmp_path), '--runs-root', str(tmp_path / 'runs'), '--no-perceptual',
              '--blocks-init', 'points', '--device', DEV]
    scores = train.main(common + ['--epochs', '2'])
    out = capsys.readouterr().out
    run_dir = tmp_path / 'runs' / 'custom' / 'run'
    written = yaml.safe_load((run_dir / 'blocks_init.yml').read_text())
    n = len(written['index'])
    assert np.isfinite(float(scores['PSNR'])) and 1 <= n <= 3 and written['n_blocks'] == 3 and written['index'] == list(range(n))
    assert f'blocks_init: points -> {n} of 3 blocks seeded' in out and all(c >= 30 for c in written['counts'])
    last = [ln for ln in out.splitlines() if ln.startswith('last step: ')]
    assert last and np.isfinite(float(last[-1].split('total=')[1].split(',')[0]))
    # the fit is deterministic: the scene and a model of its own give the file's poses again
    from dbw_amd import dataset as DS
    scene = DS.CustomScene(tmp_path, 'cap', 'train')
    kept = torch.load(run_dir / 'model.pkl', map_location='cpu', weights_only=False)['model_kwargs']
    kept.pop('img_size')
    again = scene.block_init(create_model({'model': dict(kept, name='dbw')}, scene.img_size).to(DEV), DEV)
    assert again.as_dict() == written
    # a resumed run does not fit again
    stamp = (run_dir / 'blocks_init.yml').stat().st_mtime_ns
    train.main(common + ['--epochs', '3', '--resume'])
    out = capsys.readouterr().out
    assert 'blocks_init: points -> skipped' in out and 'blocks seeded' not in out and (run_dir / 'blocks_init.yml').stat().st_mtime_ns == stamp
    assert torch.load(run_dir / 'model.pkl', map_location='cpu', weights_only=False)['epoch'] == 3
