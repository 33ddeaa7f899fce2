"""CPU: dbw_amd/worldfit.py through eval3d.plane_ransac_torch on the seeded captures of tests/worldfit_fixture.py, the refusals, and the
`R_world: auto` logic of dbw_amd/train.py as far as it runs without a device."""
import functools
import types

import numpy as np
import pytest
import torch
import yaml

import worldfit_fixture as WF
from dbw_amd import eval3d, mesh, train, worldfit as W

# 4 x the worst error of the fp64 torch path (plane_ransac_torch, dtype=torch.float64) over the eight captures, measured on the CPU:
#   normal 0.04715 degrees, plane offset 0.00199 r0, foot 0.01201 r0
BOUND_NORMAL_DEG, BOUND_OFFSET_R0, BOUND_FOOT_R0 = 4 * 0.04715, 4 * 0.00199, 4 * 0.01201


def _proper(rng):
    Q, _ = np.linalg.qr(rng.randn(3, 3))
    if np.linalg.det(Q) < 0:
        Q[:, 0] *= -1
    return Q


def test_rotation_to_euler_round_trips():
    rng = np.random.RandomState(0)
    mats = [_proper(rng) for _ in range(200)]
    # the gimbal lock, exactly: R[0] = (0, 0, +-1)
    for sa in (1.0, -1.0):
        for ang in (0.0, 0.7, -2.9):
            c, s = np.cos(ang), np.sin(ang)
            mats.append(np.array([[0, 0, sa], [sa * s, c, 0], [-sa * c, s, 0]]))
    mats += [np.eye(3), mesh.world_rotation(-90, 20, 0).double().numpy(), mesh.world_rotation(10, 90, 30).double().numpy()]
    for R in mats:
        assert abs(np.linalg.det(R) - 1) < 1e-6
        e = W.rotation_to_euler(R)
        assert np.abs(mesh.world_rotation(*e).double().numpy() - R).max() <= 1e-6, (R, e)
        assert W.rotation_to_euler(W.plane_rotation(R[1]))[0] is not None and np.allclose(W.plane_rotation(R[1])[1], R[1])


@pytest.mark.parametrize('seed', range(WF.N_CAPTURES))
def test_estimate_world_frame_on_synthetic_captures(seed):
    cap = WF.capture(seed)
    pts = torch.from_numpy(cap['points'])
    f64 = W.estimate_world_frame(pts, cap['cam2world'], ransac=functools.partial(eval3d.plane_ransac_torch, dtype=torch.float64))
    f32 = W.estimate_world_frame(pts, cap['cam2world'], T_range=(1, 0.5, 1))
    for fr in (f64, f32):
        ang, off, foot = WF.errors(fr, cap)
        print(f'capture {seed}: normal {ang:.5f} deg, offset {off:.5f} r0, foot {foot:.5f} r0')
        assert ang <= BOUND_NORMAL_DEG and off <= BOUND_OFFSET_R0 and foot <= BOUND_FOOT_R0
    fr, Tr = f32, 0.5
    n, d = fr.plane
    Rw = mesh.world_rotation(*fr.R_world).double().numpy()
    assert np.abs(Rw - fr.matrix).max() <= 1e-6 and np.abs(Rw[1] - n).max() <= 1e-6 and abs(np.linalg.det(fr.matrix) - 1) < 1e-9
    assert abs(n @ fr.c - d) <= 1e-9 * max(1, abs(d))                                     # the foot is on the plane
    # the model's initial ground, y = -0.9 T_range[1], lands in the plane; every camera is inside the sky dome
    g = (np.array([[0.3, -0.9 * Tr, -0.2], [-1.0, -0.9 * Tr, 2.0]]) * fr.S_world) @ Rw + np.array(fr.T_world)
    assert np.abs(g @ n - d).max() <= 1e-5 * fr.r0
    C = cap['cam2world'][:, :3, 3]
    assert np.linalg.norm(C - np.array(fr.T_world), axis=1).max() < W.SKY_DOME * fr.S_world
    assert fr.S_world >= 0.5 * fr.r and 0.15 * cap['scale'] < fr.r < 0.6 * cap['scale'] and 3000 < fr.n_inliers < 4000
    assert yaml.safe_load(fr.yaml()) == fr.mesh_kwargs() and set(fr.mesh_kwargs()) == {'S_world', 'R_world', 'T_world'}


def test_refusals():
    cap = WF.capture(0)
    pts = torch.from_numpy(cap['points'])
    with pytest.raises(ValueError, match='at least 100 points'):
        W.estimate_world_frame(pts[:50], cap['cam2world'])
    with pytest.raises(ValueError, match='at least 100 points'):
        W.estimate_world_frame(torch.zeros(1, 3), cap['cam2world'])
    par = cap['cam2world'].copy()
    par[:, :3, :3] = par[0, :3, :3]
    with pytest.raises(ValueError, match='parallel'):
        W.estimate_world_frame(pts, par)
    wall = WF.single_wall()
    with pytest.raises(ValueError, match='none of the 512 plane hypotheses is admissible'):
        W.estimate_world_frame(torch.from_numpy(wall['points']), wall['cam2world'])


def test_custom_scene_world_frame(tmp_path):
    from dbw_amd import dataset as DS
    cap = WF.capture(2)
    WF.write_capture(tmp_path, 'cap', cap)
    scene = DS.CustomScene(tmp_path, 'cap', 'train')
    fr = scene.world_frame()
    F = np.linalg.inv(scene.scale_mat.double().numpy())                                 # the file's frame -> the normalised one
    s = np.cbrt(np.linalg.det(F[:3, :3]))
    n = F[:3, :3] @ cap['n'] / s
    foot = F[:3, :3] @ cap['foot'] + F[:3, 3]
    ang, off, ft = WF.errors(fr, dict(n=n, d=float(n @ foot), foot=foot))
    print(f'scene of 6 cameras: normal {ang:.5f} deg, offset {off:.5f} r0, foot {ft:.5f} r0')
    assert ang <= BOUND_NORMAL_DEG and off <= BOUND_OFFSET_R0 and ft <= BOUND_FOOT_R0
    WF.write_capture(tmp_path, 'bare', cap, with_points=False)
    with pytest.raises(ValueError, match='no point cloud'):
        DS.CustomScene(tmp_path, 'bare', 'train').world_frame()


def _cfg(**mesh_kw):
    return {'model': {'mesh': dict(n_blocks=4, T_range=[1, 0.5, 1], **mesh_kw)}}


def test_auto_entries_of_a_config(tmp_path, capsys):
    assert not train.wants_world_frame(_cfg(R_world=[-90, 20, 0], T_world=[0, 0, 0], S_world=0.5)) and not train.wants_world_frame({})
    assert train.wants_world_frame(_cfg(R_world='auto')) and train.wants_world_frame(_cfg(R_world='auto', T_world='auto', S_world='auto'))
    with pytest.raises(SystemExit, match='goes with R_world: auto'):
        train.wants_world_frame(_cfg(R_world=[0, 0, 0], T_world='auto'))
    with pytest.raises(SystemExit, match="neither numbers nor 'auto'"):
        train.wants_world_frame(_cfg(R_world='automatic'))
    # numbers stay as they are
    cfg = _cfg(R_world=[1, 2, 3])
    assert train.resolve_world_frame(cfg, None, None) is None and cfg['model']['mesh']['R_world'] == [1, 2, 3]
    # DTU / BlendedMVS: refused with the reason
    with pytest.raises(SystemExit, match="'dtu' scene is normalised by its scale_mat"):
        train.resolve_world_frame(_cfg(R_world='auto'), types.SimpleNamespace(name='dtu'), 'cpu')
    # a scene without a cloud: the estimator's reason is passed on
    def no_cloud(device, T_range):
        raise ValueError("'x': no point cloud")
    with pytest.raises(SystemExit, match='R_world: auto: .*no point cloud'):
        train.resolve_world_frame(_cfg(R_world='auto'), types.SimpleNamespace(name='custom', world_frame=no_cloud), 'cpu')
    # the estimate replaces the three entries, is printed and written
    cap = WF.capture(1)
    asked = {}

    def world_frame(device, T_range):
        asked.update(device=device, T_range=T_range)
        return W.estimate_world_frame(torch.from_numpy(cap['points']), cap['cam2world'], T_range=T_range)
    cfg = _cfg(R_world='auto', S_world='auto')
    fr = train.resolve_world_frame(cfg, types.SimpleNamespace(name='custom', world_frame=world_frame), 'cpu', str(tmp_path))
    m = cfg['model']['mesh']
    assert asked == dict(device='cpu', T_range=[1, 0.5, 1]) and {k: m[k] for k in train.WORLD_KEYS} == fr.mesh_kwargs()
    assert yaml.safe_load((tmp_path / 'world_frame.yml').read_text()) == fr.mesh_kwargs()
    assert 'R_world: auto -> WorldFrame(' in capsys.readouterr().out
    # a resumed run takes the numbers of its checkpoint and does not fit again
    torch.save({'model_kwargs': {'mesh': dict(m)}}, tmp_path / 'model.pkl')
    cfg2 = _cfg(R_world='auto', T_world='auto')
    scene = types.SimpleNamespace(name='custom', world_frame=lambda *a, **k: pytest.fail('a resumed run fitted again'))
    assert train.resolve_world_frame(cfg2, scene, 'cpu', None, resume=str(tmp_path / 'model.pkl')) is None
    assert {k: cfg2['model']['mesh'][k] for k in train.WORLD_KEYS} == fr.mesh_kwargs()


def test_plane_ransac_torch_matches_the_host_build():
    import plane_ref as PR
    pts, cams, up = WF.plane_cloud(1000, 1)
    for mode, kw in (('orthogonal', dict(thresh=0.02, up=up, cams=cams, min_side=1.0)), ('orthogonal', dict(thresh=0.02)), ('vertical', {})):
        r = eval3d.plane_ransac(torch.from_numpy(pts), n_hyp=65, residual=mode, seed=9, return_counts=True, return_mask=True, refine=2, **kw)
        n_hyp, m, th2, tau, u, ct, cm, minc, refine, _ = eval3d._plane_args(torch.from_numpy(pts), 65, kw.get('thresh'), mode, kw.get('up'), 60.0,
                                                                              kw.get('cams'), kw.get('min_side', 0.9), 2, None)
        o = PR.host_fit(pts, 65, m, th2, seed=9, up=None if u is None else u.numpy(), cos_tilt=ct, cams=None if cm is None else cm.numpy(), tau=tau,
                        min_cams=minc, refine=refine)
        assert np.array_equal(o['counts'], r.counts.numpy()) and np.array_equal(o['triples'], r.triples.numpy()) and int(r.best) == o['info'][0]
        assert np.array_equal(o['mask'].astype(bool), r.mask.numpy()) and int(r.n_inliers) == o['info'][2] and int(r.rounds) == o['info'][3]
        assert np.abs(torch.cat([r.normal, r.offset[None]]).numpy() - o['plane']).max() <= 1e-12
    # filter_ground: the reference's use of its Ransac, on the reference's triples
    g = PR.golden()
    res = eval3d.plane_ransac(torch.from_numpy(g['points']), residual='vertical', triples=g['triples'], return_counts=True, return_mask=True)
    PR.check_golden(g, res.counts.numpy(), int(res.best), int(res.counts.max()))
    kept, params = eval3d.filter_ground(torch.from_numpy(g['points']), seed=1)
    assert kept.shape[0] < 0.55 * 4096 and params.shape == (3,) and np.abs(params.numpy() - g['params']).max() < 0.02
