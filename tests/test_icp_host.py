"""CPU tests of the ICP-aligned evaluation (dbw_amd/eval3d.py, dbw_amd/metrics.py, include/dbw_icp.h), no GPU needed:
  * the C ABI of include/dbw_icp.h: validation before any launch (prototypes, revision, symbols: tests/test_abi_families.py);
  * gradient_icp on CPU tensors recovers the transform of the ellipsoid pair; fp32 and fp64 agree as measured when the input was chosen;
  * the refusals; normalize_mesh; the Metrics TSV bytes; MeshEvaluator on a sphere pair; ProxyEvaluator on two masks."""
import ctypes

import numpy as np
import pytest
import torch

from dbw_amd import _lib, eval3d, mesh, metrics
import icp_fixture as fx


def test_icp_entry_points_validate_before_any_launch():
    lib = _lib.load()
    P = ctypes.c_void_p
    ok = [P(64)] * 2 + [2, 100, 90, 1, 1, 0.01, 10, 0, P(64)] + [P(64)] * 5 + [None, None]

    def run(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.dbw_icp_run(*a)

    assert run(a0=None) == -1 and b'null pointer' in lib.dbw_last_error()
    assert run(a10=None) == -1 and b'null pointer' in lib.dbw_last_error()
    assert run(a15=None) == -1 and b'null pointer' in lib.dbw_last_error()
    for k, v in (('a2', 0), ('a3', 0), ('a4', -1), ('a8', -1), ('a9', -1), ('a2', 65536)):
        assert run(**{k: v}) == -1 and b'bad size' in lib.dbw_last_error(), k
    assert run(a5=2) == -1 and b'flags' in lib.dbw_last_error()
    assert run(a7=0.0) == -1 and b'lr' in lib.dbw_last_error()
    assert run(a7=float('nan')) == -1 and b'lr' in lib.dbw_last_error()
    assert run(a10=P(72)) == -1 and b'16-byte' in lib.dbw_last_error()
    assert run(a11=P(66)) == -1 and b'misaligned' in lib.dbw_last_error()
    assert run(a16=P(68)) == -1 and b'misaligned' in lib.dbw_last_error()
    assert lib.dbw_icp_workspace_bytes(0, 10, 10, 5) == 0 and lib.dbw_icp_workspace_bytes(1, 10, 0, 5) == 0
    assert lib.dbw_icp_workspace_bytes(1, 10, 10, -1) == 0
    # keys of both searches, q, at least one workgroup's partials: the workspace grows with the clouds, not with n_iter
    small, large = lib.dbw_icp_workspace_bytes(2, 100, 90, 10), lib.dbw_icp_workspace_bytes(2, 100000, 90000, 10)
    assert small >= 2 * (100 * 8 + 90 * 8 + 100 * 12) and large >= 2 * (100000 * 8 + 90000 * 8 + 100000 * 12)
    assert small % 16 == 0 and lib.dbw_icp_workspace_bytes(2, 100, 90, 1000) == small


def test_gradient_icp_on_cpu_recovers_the_transform():
    pp, pg = fx.ellipsoid_pair()
    upd, (R, T, s) = eval3d.gradient_icp(pp.double(), pg.double(), True, True, lr=0.01, n_iter=100)
    assert upd.shape == pp.shape and R.shape == (2, 3, 3) and T.shape == (2, 3) and s.shape == (2, 3) and upd.dtype == torch.float64
    # the figures the input was chosen with, T ~ (0.030, -0.020, 0.040) and s ~ 1.10: to one unit of the last digit quoted
    assert (T - torch.tensor(fx.SHIFT, dtype=torch.float64)).abs().max() < 1e-3 and (s - fx.SCALE).abs().max() < 1e-2
    assert torch.allclose(R @ R.transpose(1, 2), torch.eye(3, dtype=torch.float64).expand(2, 3, 3), atol=1e-12)
    before = eval3d.chamfer_distance(pp.double(), pg.double())[0].item()
    after = eval3d.chamfer_distance(upd, pg.double())[0].item()
    assert after < 0.25 * before                   # (the noise of 0.01 per coordinate leaves a floor of ~7e-4)
    assert torch.equal(upd, s[:, None] * pp.double() @ R + T[:, None])


@pytest.mark.parametrize('anisotropic', [False, True])
def test_fp32_and_fp64_torch_loops_agree_on_the_chosen_input(anisotropic):
    """what makes the input fit for the device comparison: the figures of the fp32 / fp64 spread (1.3e-7, 2.6e-8, 1.7e-7 in R, T, s for the
    anisotropic run) stay below 1e-5, and both runs keep iteration 30"""
    assert fx.reference_spread(anisotropic) < 1e-5
    for dt in (torch.float32, torch.float64):
        _, (R, T, s), trace = fx.torch_run(dt, anisotropic)
        assert trace['best_iter'] == 30 and s.shape == (2, 3 if anisotropic else 1)
        assert trace['R'].shape == (31, 2, 3, 3) and torch.equal(trace['R'][30], R) and torch.equal(trace['T'][30], T)
        assert eval3d.keep_best_history(trace['loss'].tolist(), 2)[:2] == (trace['best_loss'], 30)


def test_keep_best_inputs_reach_the_no_update_branch():
    pp, pg = fx.ellipsoid_pair()
    tr = eval3d.gradient_icp_torch(pp, pg, True, True, lr=0.3, n_iter=41, return_trace=True)[2]
    kept = [c[0] for c in eval3d.keep_best_history(tr['loss'].tolist(), 2)[2] if c[2]]
    assert kept[0] == 0 and 0 < len(kept) < 5
    pa, ga = fx.aligned_pair()
    tr = eval3d.gradient_icp_torch(pa, ga, True, True, lr=0.01, n_iter=41, return_trace=True)[2]
    kept = [c[0] for c in eval3d.keep_best_history(tr['loss'].tolist(), 1)[2] if c[2]]
    assert kept[0] == 0 and 0 < len(kept) < 5


def test_gradient_icp_edges_and_refusals(capsys):
    pp, pg = fx.ellipsoid_pair()
    pp, pg = pp[:1, :200], pg[:1, :150]
    upd, (R, T, s) = eval3d.gradient_icp(pp, pg, n_iter=0)
    assert torch.equal(upd, pp) and torch.equal(R, torch.eye(3)[None]) and torch.equal(T, torch.zeros(1, 3)) and torch.equal(s, torch.ones(1, 1))
    upd, (R, T, s) = eval3d.gradient_icp(pp, pg, estimate_scale=False, n_iter=3)
    assert torch.equal(s, torch.ones(1, 3)) and not torch.equal(T, torch.zeros(1, 3))
    with pytest.raises(NotImplementedError, match='mini-batch'):
        eval3d.gradient_icp(pp, pg, batch_size=4, shared_params=True)
    with pytest.raises(NotImplementedError, match='shared_params'):
        eval3d.gradient_icp(pp, pg, shared_params=True)
    with pytest.raises(ValueError):
        eval3d.gradient_icp(pp, pg[0])
    with pytest.raises(ValueError, match='cuda'):
        eval3d.icp_run(pp, pg)
    eval3d.gradient_icp(pp, pg, n_iter=11, verbose=True)
    lines = capsys.readouterr().out.strip().split('\n')
    assert len(lines) == 2 and lines[0].endswith('save checkpoint') and float(lines[0].split()[0]) > float(lines[1].split()[0])


def test_normalize_mesh():
    verts, faces = mesh.get_icosphere(1)
    v = verts * torch.tensor([2., 1., 0.5]) + torch.tensor([3., -1., 0.2])
    nv, nf = eval3d.normalize_mesh(v, faces)
    assert nf is faces and abs(float(nv.abs().max()) - 0.5) < 1e-6
    assert torch.allclose(nv.max(0).values + nv.min(0).values, torch.zeros(3), atol=1e-6)
    assert torch.allclose(nv, (v - torch.tensor([3., -1., 0.2])) / (2 * float((v - torch.tensor([3., -1., 0.2])).abs().max())), atol=1e-6)
    ns, _ = eval3d.normalize_mesh(v, faces, scale_mode='unit_sphere')
    assert abs(float(ns.norm(dim=1).max()) - 0.5) < 1e-6
    nn_, _ = eval3d.normalize_mesh(v, faces, scale_mode=None)
    assert torch.allclose(nn_, v - 0.5 * (v.max(0).values + v.min(0).values))
    nc, _ = eval3d.normalize_mesh(v, faces, center=False)
    assert torch.allclose(nc, v / (2 * v.abs().max()))
    with pytest.raises(NotImplementedError, match='use_center_mass'):
        eval3d.normalize_mesh(v, faces, use_center_mass=True)
    with pytest.raises(NotImplementedError):
        eval3d.normalize_mesh(v, faces, scale_mode='cylinder')


def test_metrics_tsv_bytes(tmp_path):
    """utils/metrics.py:41-59 byte for byte: the header, `it epoch batch` as Python prints them, the averages as '{:.6f}'"""
    log = tmp_path / 'm.tsv'
    m = metrics.Metrics('loss', 'psnr', log_file=log)
    m.update('loss', 0.123456789, N=2)
    m.update('loss', torch.tensor(0.5), N=2)
    m.update({'psnr': (21.5, 4)})
    assert m['loss'].avg == (0.123456789 * 2 + 0.5 * 2) / 4 and len(m) == 2 and repr(m) == 'loss=0.3117, psnr=21.5000'
    m.log_and_reset(it=10, epoch=1, batch=3)
    assert m.values == [0.0, 0.0]
    m.update('psnr', 1 / 3)
    m.log_and_reset('psnr', it=None, epoch=2, batch=None)
    assert log.read_bytes() == b'iteration\tepoch\tbatch\tloss\tpsnr\n10\t1\t3\t0.311728\t21.500000\nNone\t2\tNone\t0.000000\t0.333333\n'
    assert m.read_log() == {'iteration': [10, 'None'], 'epoch': [1, 2], 'batch': [3, 'None'], 'loss': [0.311728, 0.0], 'psnr': [21.5, 0.333333]}
    with pytest.raises(KeyError):
        m.update('ssim', 1.0)
    m2 = metrics.Metrics('loss', 'psnr', log_file=log, append=True)
    m2.log(11, 1, 4)
    assert log.read_bytes().endswith(b'0.333333\n11\t1\t4\t0.000000\t0.000000\n') and log.read_bytes().startswith(b'iteration')
    metrics.Metrics('loss', log_file=log)
    assert log.read_bytes() == b'iteration\tepoch\tbatch\tloss\n'
    assert metrics.Metrics('a').read_log() == {} and metrics.Metrics('a', 'b').get_named_values(lambda n: n == 'b') == [('b', 0.0)]


def test_mesh_evaluator_on_a_sphere_pair(tmp_path):
    (vp, faces), pc_gt, norm_gt, ev, samples = fx.sphere_case()
    assert ev.N == 5000 and ev.n_iter == 30 and metrics.MeshEvaluator().N == 100000 and metrics.MeshEvaluator().n_iter == 100
    assert metrics.MeshEvaluator(fast_cpu=True).N == 50000
    res = ev.evaluate((vp, faces), pc_gt, norm_gt, samples=samples)
    assert list(res) == ['chamfer-L1', 'normal-cos', 'chamfer-L1-ICP', 'normal-cos-ICP']
    assert res['chamfer-L1-ICP'] < 0.5 * res['chamfer-L1']
    # (like the reference, the normals of the aligned samples are those of the normalised mesh, not rotated by the alignment)
    assert 0.5 < res['normal-cos-ICP'] <= 1 and 0.5 < res['normal-cos'] <= 1
    # the recorded scores of this case (the yardstick of the GPU test) are this path's: same draw, the fp64 scores within the recorded
    # fp32 / fp64 spread times 8
    g = fx.sphere_golden()
    assert fx.sphere_checksum() == pytest.approx(g['checksum'], rel=1e-9)      # the same draw as recorded
    spread = max(abs(g['fp32'][k] - g['fp64'][k]) for k in g['fp64'])
    assert 0 < spread <= 1e-5 * metrics.CHAMFER_FACTOR and max(abs(res[k] - g['fp64'][k]) for k in res) <= 8 * spread
    ev = metrics.MeshEvaluator(names=fx.SPHERE_NAMES, fast_cpu=True, n_points=1000, log_file=tmp_path / 'mesh.tsv')
    pc_gt, norm_gt = pc_gt[:, :1500], norm_gt[:, :1500]
    pc_gt = pc_gt / (2 * pc_gt.abs().max())
    # the same samples, the same scores; without normals only the Chamfer scores
    samples = ev.draw_samples((vp, faces), True, torch.Generator().manual_seed(4))
    a = ev.evaluate((vp, faces), pc_gt, norm_gt, samples=samples, generator=torch.Generator().manual_seed(5))
    b = ev.evaluate((vp, faces), pc_gt, norm_gt, samples=samples, generator=torch.Generator().manual_seed(5))
    assert a == b
    c = ev.evaluate((vp, faces), pc_gt[0], samples=samples, generator=torch.Generator().manual_seed(5))
    assert list(c) == ['chamfer-L1', 'chamfer-L1-ICP'] and c['chamfer-L1'] == a['chamfer-L1']
    ev.update((vp, faces), {'points': pc_gt, 'normals': norm_gt})
    ev.log_and_reset(it=1, epoch=0, batch=0)
    assert (tmp_path / 'mesh.tsv').read_text().split('\n')[0] == 'iteration\tepoch\tbatch\tchamfer-L1\tchamfer-L1-ICP\tnormal-cos\tnormal-cos-ICP'
    assert len(ev.read_log()['chamfer-L1-ICP']) == 1
    # the refusals
    with pytest.raises(ValueError, match='unit cube'):
        ev.evaluate((vp, faces), pc_gt * 1.5, norm_gt)
    with pytest.raises(NotImplementedError, match='iterative_closest_point'):
        metrics.MeshEvaluator(icp_type='normal')
    with pytest.raises(ValueError):
        metrics.MeshEvaluator(icp_type='rigid')
    with pytest.raises(NotImplementedError, match='batch processing'):
        metrics.MeshEvaluator().evaluate((vp, faces), pc_gt, norm_gt, vox_gt=torch.zeros(1, 4, 4, 4))
    no_icp = metrics.MeshEvaluator(names=['chamfer-L1', 'chamfer-L1-ICP'], run_icp=False, n_points=500).evaluate((vp, faces), pc_gt)
    assert list(no_icp) == ['chamfer-L1']


def test_unit_cube_frame():
    pts = torch.tensor([[1., 2., 3.], [3., 2.5, 3.5], [2., 2.2, 3.1]])
    off, sc = eval3d.unit_cube_frame(pts)
    assert torch.equal(off, torch.tensor([2., 2.25, 3.25])) and float(sc) == 2.0
    assert float(((pts - off) / sc).abs().max()) == 0.5


def test_proxy_evaluator_on_two_masks():
    a = torch.zeros(2, 8, 8)
    b = torch.zeros(2, 8, 8)
    a[0, :4], b[0, 2:6] = 1, 1                      # 16 of 48
    a[1, :, :4], b[1, :, :4] = 1, 1                 # identical
    ev = metrics.ProxyEvaluator()
    assert ev.evaluate(a[0], b[0]) == {'mask_iou': pytest.approx(1 / 3)}
    ev.update(a, b)
    assert ev.compute() == [pytest.approx((1 / 3 + 1) / 2)] and repr(ev) == 'mask_iou=0.6667'
    assert metrics.ProxyEvaluator(names=['other']).evaluate(a[0], b[0]) == {}
