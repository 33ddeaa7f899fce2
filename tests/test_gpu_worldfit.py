"""GPU tests of the plane RANSAC (csrc/plane_fit.hip, dbw_eval_plane_fit of include/dbw_eval.h) and of the world-frame estimate on top of it.
`-m gpu`.

Bounds.  Hypotheses, counts, the best hypothesis and the inlier mask are integer results of fp32 arithmetic that the kernels and the host
build (tests/host_plane_math.cpp) compile from one header with one rounding per operation: they are compared for equality.  The refined
plane goes through fp64 sums whose order differs between the two (the host adds in index order, the device lane by lane, by shuffle tree,
by wave, by workgroup): see _refine_bound."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import plane_ref as PR                                          # noqa: E402
import worldfit_fixture as WF                                   # noqa: E402
from dbw_amd import create_model, eval3d, ops, train           # noqa: E402
from dbw_amd import dataset as DS                               # noqa: E402
from test_worldfit_host import BOUND_FOOT_R0, BOUND_NORMAL_DEG, BOUND_OFFSET_R0      # noqa: E402

DEV = 'cuda'
COS60 = float(np.float32(math.cos(math.radians(60))))


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype).contiguous()


def _device_fit(pts, H, mode, thresh2, **kw):
    o = eval3d.plane_fit(_dev(pts), H, mode, thresh2, seed=kw.get('seed', 0), triples=_dev(kw.get('triples'), torch.int32), up=_dev(kw.get('up')),
                         cos_tilt=kw.get('cos_tilt', 0.0), cams=_dev(kw.get('cams')), tau=kw.get('tau', 0.0), min_cams=kw.get('min_cams', 0),
                         refine=kw.get('refine', 0))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _same_integers(d, h):
    assert h['rc'] == 0
    assert np.array_equal(d['triples'], h['triples']) and np.array_equal(d['counts'], h['counts'])
    assert d['info'][:2].tolist() == h['info'][:2].tolist()


@pytest.mark.parametrize('N', [3, 63, 64, 65, 1000, 4097])
def test_device_equals_host_build(N):
    pts, cams, up = WF.plane_cloud(N, 10 + N)
    tau = np.float32(0.02)
    cases = [(PR.ORTHOGONAL, float(tau * tau), {}),
             (PR.ORTHOGONAL, float(tau * tau), dict(up=up, cos_tilt=COS60, cams=cams, tau=float(tau), min_cams=5)),
             (PR.VERTICAL, float(np.float32(0.001)), {})]
    for H in (1, 7, 64, 513):
        for mode, thresh2, kw in cases:
            d = _device_fit(pts, H, mode, thresh2, seed=N + H, **kw)
            h = PR.host_fit(pts, H, mode, thresh2, seed=N + H, **kw)
            _same_integers(d, h)
            assert np.array_equal(d['mask'], h['mask']) and d['info'].tolist() == h['info'].tolist(), (N, H, mode)
            assert np.array_equal(d['plane'], h['plane'])                    # refine = 0: the fp32 hypothesis itself, or zeros
            if N >= 1000 and H >= 64:
                assert d['info'][0] >= 0 and d['info'][1] > 0.5 * N * 0.6    # the test is not vacuous: the ground is found


def test_degenerate_and_inadmissible_triples_are_marked():
    pts, cams, up = WF.plane_cloud(200, 4)
    pts[10] = pts[0] + 2.5 * (pts[5] - pts[0])                               # 0, 5, 10 collinear
    wall = np.array([[0.3, -1, 0], [0.3, 1, 0], [0.3, 0, 1]], np.float32)    # a vertical triangle: tilt 90 degrees against up
    pts[20:23] = wall
    good = PR.host_fit(pts, 64, PR.ORTHOGONAL, 4e-4, seed=1, up=up, cos_tilt=COS60, cams=cams, tau=0.02, min_cams=5)
    g = good['triples'][int(good['info'][0])].tolist()
    triples = [g, [3, 3, 7], g, [0, 5, 10], [20, 21, 22], g, [1, 2, 200], [-1, 2, 3]]
    kw = dict(triples=triples, up=up, cos_tilt=COS60, cams=cams, tau=0.02, min_cams=5)
    d, h = _device_fit(pts, 8, PR.ORTHOGONAL, 4e-4, **kw), PR.host_fit(pts, 8, PR.ORTHOGONAL, 4e-4, **kw)
    _same_integers(d, h)
    assert (d['counts'] == -1).tolist() == [False, True, False, True, True, False, True, True] and d['info'][0] == 0
    # the vertical triangle is degenerate in the vertical mode too (m.z == 0), and admissible without the priors
    d = _device_fit(pts, 8, PR.VERTICAL, 1e-3, triples=triples)
    assert (d['counts'] == -1).tolist() == [False, True, False, True, True, False, True, True]
    d = _device_fit(pts, 8, PR.ORTHOGONAL, 4e-4, triples=triples)
    assert (d['counts'] == -1).tolist() == [False, True, False, True, False, False, True, True]
    # nothing admissible: the call succeeds, the plane is zero
    d = _device_fit(pts, 2, PR.ORTHOGONAL, 4e-4, triples=[[3, 3, 7], [0, 5, 10]], refine=2)
    assert d['info'].tolist() == [-1, 0, 0, 0] and not d['plane'].any() and not d['mask'].any()


def _refine_bound(pts, h, N):
    """What the device's refined plane may differ by from the host's.  Both add the same N terms q, q q^T (q = p - a0, |q| <= D) in fp64 in
    another order: a sum of k terms differs by at most k eps sum|terms|, so every entry of the covariance (sum / count - mean mean^T) by at
    most 4 N eps D^2.  The smallest eigenvector of C + E turns by at most |E|_F / gap (Davis-Kahan; gap = lambda_1 - lambda_0), and the
    fixed-sweep Jacobi adds 96 eps |C|_F / gap on each side (tests/test_host_plane_math.py).  d = n . (a0 + mean) moves by the turn times
    |a0 + mean| plus the rounding of the mean.  Round 2 starts from the SAME inlier set on both sides (the margin asserted by the caller), so
    the error of round 1 is not carried over.  -> (bound on a component of n, bound on d)"""
    eps = 2.0 ** -52
    inl = pts[h['mask'].astype(bool)].astype(np.float64)
    D = np.linalg.norm(inl.max(0) - inl.min(0))
    C = np.cov(inl.T, bias=True)
    w = np.linalg.eigvalsh(C)
    turn = (3 * 4 * N * eps * D * D + 2 * 96 * eps * np.linalg.norm(C)) / (w[1] - w[0])
    return turn, turn * (np.abs(inl).max() * 2 + D) + 4 * N * eps * D


def _margin(pts, plane, tau):
    r = np.abs(pts.astype(np.float64) @ np.float32(plane[:3]).astype(np.float64) - float(np.float32(plane[3])))
    return np.abs(r - tau).min()


def test_refined_plane_and_repeatability():
    N, H = 4097, 64
    pts, cams, up = WF.plane_cloud(N, 21)
    tau = np.float32(0.02)
    kw = dict(seed=2, up=up, cos_tilt=COS60, cams=cams, tau=float(tau), min_cams=5)
    h1 = PR.host_fit(pts, H, PR.ORTHOGONAL, float(tau * tau), refine=1, **kw)
    h = PR.host_fit(pts, H, PR.ORTHOGONAL, float(tau * tau), refine=2, **kw)
    assert h['info'][3] == 2
    # the fixture's margin, on the CPU: no point within 1e-6 tau of the threshold of the plane after either round
    assert min(_margin(pts, h1['plane'], float(tau)), _margin(pts, h['plane'], float(tau))) >= 1e-6 * float(tau)
    d = _device_fit(pts, H, PR.ORTHOGONAL, float(tau * tau), refine=2, **kw)
    _same_integers(d, h)
    bn, bd = _refine_bound(pts, h, N)
    err_n, err_d = np.abs(d['plane'][:3] - h['plane'][:3]).max(), abs(d['plane'][3] - h['plane'][3])
    print(f'refined plane, device vs host: normal {err_n:.3e} (bound {bn:.3e}), d {err_d:.3e} (bound {bd:.3e})')
    assert err_n <= bn and err_d <= bd
    assert np.array_equal(d['mask'], h['mask']) and d['info'].tolist() == h['info'].tolist()
    again = _device_fit(pts, H, PR.ORTHOGONAL, float(tau * tau), refine=2, **kw)
    for k in d:
        assert d[k].tobytes() == again[k].tobytes(), k
    # the refinement moved the plane towards the truth
    n = np.array([-0.2, 0.1, 1.0]) / np.linalg.norm([-0.2, 0.1, 1.0])
    assert np.degrees(np.arccos(d['plane'][:3] @ n)) < 0.2


def test_reference_ransac_fixture_and_filter_ground():
    g = PR.golden()
    d = _device_fit(g['points'], 100, PR.VERTICAL, float(np.float32(g['thresh'])), triples=g['triples'])
    PR.check_golden(g, d['counts'], int(d['info'][0]), int(d['info'][1]))
    p = np.array([d['plane'][3], -d['plane'][0], -d['plane'][1]])
    assert d['plane'][2] == 1.0 and np.abs(p - g['params']).max() <= 1e-4 * max(1.0, np.abs(g['params']).max())
    pts = torch.from_numpy(g['points']).to(DEV)
    kept, params = eval3d.filter_ground(pts, triples=g['triples'])
    assert torch.equal(kept.cpu(), torch.from_numpy(g['points'][~g['mask']])) and np.array_equal(params.cpu().numpy(), p)
    kept, _ = eval3d.filter_ground(pts, seed=1)                              # its own draw: the same ground, give or take the band's edge
    assert abs(kept.shape[0] - int((~g['mask']).sum())) < 60


def test_plane_ransac_against_the_torch_path():
    cap = WF.capture(3)
    C = cap['cam2world'][:, :3, 3]
    pts = torch.from_numpy(cap['points']).to(DEV)
    kw = dict(n_hyp=512, thresh=0.03 * cap['scale'], up=cap['n'], cams=C, seed=4, return_counts=True, return_mask=True)
    a, b = eval3d.plane_ransac(pts, **kw), eval3d.plane_ransac_torch(pts, **kw)
    assert all(t.device.type == 'cuda' for t in a if t is not None)
    assert torch.equal(a.counts, b.counts) and int(a.best) == int(b.best) >= 0 and torch.equal(a.triples, b.triples)
    assert int((a.counts >= 0).sum()) > 50 and int(a.rounds) == 2 == int(b.rounds)
    assert torch.equal(a.mask, b.mask) and int(a.n_inliers) == int(b.n_inliers)
    assert float((a.normal - b.normal).abs().max()) < 1e-9 and abs(float(a.offset - b.offset)) < 1e-9
    with pytest.raises(ValueError, match='are refused'):                     # sizes are refused before anything is launched
        eval3d.plane_fit(pts, 5000, 0, 1e-3)
    with pytest.raises(RuntimeError, match='refine must be in'):
        eval3d.plane_fit(pts, 8, 0, 1e-3, refine=9)


@pytest.fixture(scope='module')
def scene_root(tmp_path_factory):
    root = tmp_path_factory.mktemp('worldfit')
    cap = WF.capture(2)
    WF.write_capture(root, 'cap', cap)
    return root, cap


def test_world_frame_of_a_custom_scene_and_the_model_built_from_it(scene_root):
    root, cap = scene_root
    scene = DS.CustomScene(root, 'cap', 'train')
    Tr = 0.5
    fr = scene.world_frame(DEV, T_range=(1, Tr, 1))
    F = np.linalg.inv(scene.scale_mat.double().numpy())
    s = np.cbrt(np.linalg.det(F[:3, :3]))
    n_true = F[:3, :3] @ cap['n'] / s
    foot = F[:3, :3] @ cap['foot'] + F[:3, 3]
    ang, off, ft = WF.errors(fr, dict(n=n_true, d=float(n_true @ foot), foot=foot))
    print(f'device: normal {ang:.5f} deg, offset {off:.5f} r0, foot {ft:.5f} r0; {fr}')
    assert ang <= BOUND_NORMAL_DEG and off <= BOUND_OFFSET_R0 and ft <= BOUND_FOOT_R0
    cpu = scene.world_frame(None, T_range=(1, Tr, 1))
    assert np.abs(np.array(cpu.T_world) - np.array(fr.T_world)).max() < 1e-9 and abs(cpu.S_world - fr.S_world) < 1e-9

    torch.manual_seed(11)
    cfg = {'model': {'name': 'dbw', 'mesh': dict(n_blocks=8, txt_size=16, T_range=[1, Tr, 1], **fr.mesh_kwargs()),
                     'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                     'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True, 'opacity_noise': False},
                     'loss': {'rgb_weight': 1, 'perceptual_weight': 0, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}}}
    model = create_model(cfg, scene.img_size).to(DEV)
    S_w, R_w, T_w = model._world_consts()
    n, d = fr.plane
    with torch.no_grad():
        ground = ops.posed_mesh(model.R_6d_ground, model.T_ground, model._ground_base, S_w, R_w, T_w).double().cpu().numpy()
    # fp32: the vertices reach 10 sqrt(2) S_world from T_world, the rotation is made of fp32 sines of degrees (a few 1e-7 on that lever),
    # the posed vertex is a dozen fp32 operations on numbers of that size: 32 eps (15 S_world + |T_world| + |d|)
    bound = 32 * 2.0 ** -24 * (15 * fr.S_world + np.abs(fr.T_world).max() + abs(d))
    dist = np.abs(ground.reshape(-1, 3) @ n - d).max()
    print(f'ground vertices off the fitted plane by at most {dist:.3e} (bound {bound:.3e})')
    assert dist <= bound
    centres = (model.T.detach().double().cpu().numpy() * S_w) @ R_w.double().cpu().numpy() + T_w.double().cpu().numpy()
    target = fr.c + n * 0.9 * Tr * fr.S_world
    assert np.linalg.norm(centres.mean(0) - target) <= fr.S_world


def test_the_command_line_fits_the_world_frame(scene_root, tmp_path, capsys):
    import yaml
    root, _ = scene_root
    cfg = {'dataset': {'name': 'custom', 'tag': 'cap'},
           'model': {'name': 'dbw', 'mesh': {'n_blocks': 2, 'R_world': 'auto', 'T_world': 'auto', 'S_world': 'auto', 'txt_size': 16},
                     'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                     'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True,
                                    'opacity_noise': False},
                     'loss': {'rgb_weight': 1, 'perceptual_weight': 0.1, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}},
           'training': {'batch_size': 2, 'n_epoches': 3, 'seed': 3, 'optimizer': {'name': 'adam', 'lr': 1e-3}, 'scheduler': {'name': 'multi_step'}}}
    path = tmp_path / 'cap.yml'
    with open(path, 'w') as f:
        yaml.safe_dump(cfg, f)
    scores = train.main(['--config', str(path), '--tag', 'run', '--data-root', str(root), '--runs-root', str(tmp_path / 'runs'),
                         '--no-perceptual', '--epochs', '1', '--device', DEV])
    assert np.isfinite(float(scores['PSNR'])) and 'R_world: auto -> WorldFrame(' in capsys.readouterr().out
    run_dir = tmp_path / 'runs' / 'custom' / 'run'
    written = yaml.safe_load((run_dir / 'world_frame.yml').read_text())
    expect = DS.CustomScene(root, 'cap', 'train').world_frame(DEV).mesh_kwargs()
    assert written == expect
    kept = torch.load(run_dir / 'model.pkl', map_location='cpu', weights_only=False)['model_kwargs']['mesh']
    assert {k: kept[k] for k in train.WORLD_KEYS} == expect
