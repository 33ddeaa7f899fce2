"""GPU tests of the gradient ICP (csrc/icp_align.hip, include/dbw_icp.h) and of the ICP-aligned evaluation on top of it.

The value comparisons use the ellipsoid pair of tests/icp_fixture.py at lr = 0.01, where the torch loop in fp32 and in fp64 agree to ~1e-7;
the bar of the device is computed from that reference alone (8 x the fp32 / fp64 spread: the device differs from either in the same way,
another summation order and an fp32 chain).  lr = 0.3 and the aligned clouds are only used for the keep-best logic, on the device's own
loss history: there Adam amplifies rounding noise and no two implementations agree in value."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dbw_amd                                                  # noqa: E402
from dbw_amd import eval3d, metrics                             # noqa: E402
import icp_fixture as fx                                        # noqa: E402
from test_host_icp_math import lib as host_lib, _p              # noqa: E402

DEV = 'cuda'
ILL_CONDITIONED = 1e-5


def _run(pp, pg, **kw):
    o = eval3d.icp_run(pp.to(DEV), pg.to(DEV), with_trace=True, **kw)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu()) for k, v in o.items()}


def _rts(trace, it, N):
    """R (N,3,3), T (N,3), s (N,3) of iteration `it` of a device trace, as fp32"""
    r = trace[it, 1:].reshape(N, 15).float()
    return r[:, :9].reshape(N, 3, 3), r[:, 9:12], r[:, 12:15]


def test_one_iteration_against_fp64_from_the_devices_own_pairs():
    """What is independent of the device here are the 26 sums and the loss: fp64 torch from the device's own q and neighbour indices.  The
    step from those sums to the parameters goes through host_icp_step, the host build of the SAME icp_math.h chain and Adam the update kernel
    compiles, so the 2 ulp compare the two builds of that header; that the header is right rests on tests/test_host_icp_math.py (the chain
    against fp64 autograd, Adam against torch.optim.Adam) and, end to end, on the trajectory test below."""
    pp, pg = fx.ellipsoid_pair()
    N, P1, P2 = 2, pp.shape[1], pg.shape[1]
    # q of iteration 0 is the transform by the identity block: n_iter = 0 writes it out
    q = _run(pp, pg, estimate_scale=True, anisotropic_scale=True, n_iter=0)['cloud']
    assert torch.equal(q, pp)
    o = _run(pp, pg, estimate_scale=True, anisotropic_scale=True, lr=0.01, n_iter=1)
    assert o['best'].tolist() == [o['trace'][0, 0].item(), 0.0]
    # the cloud under the kept parameters, bit for bit the host build of icp_math.h
    rts = np.ascontiguousarray(torch.cat([o['R'].reshape(N, 9), o['T'], o['s']], 1).numpy())
    for n in range(N):
        ref, pn, rn = np.zeros((P1, 3), np.float32), np.ascontiguousarray(pp[n].numpy()), np.ascontiguousarray(rts[n])
        host_lib().host_icp_transform(_p(rn), _p(pn), P1, _p(ref))
        assert np.array_equal(o['cloud'][n].numpy(), ref)
    # the sums in fp64 torch from the device's q and neighbour indices
    i1 = eval3d.nn_points(q.to(DEV), pg.to(DEV))[1].cpu()
    i2 = eval3d.nn_points(pg.to(DEV), q.to(DEV))[1].cpu()
    q64, g64, p64 = q.double(), pg.double(), pp.double()
    loss, loss_abs = 0.0, 0.0
    for n in range(N):
        r1, r2 = q64[n] - g64[n][i1[n]], q64[n][i2[n]] - g64[n]
        pa, pb = p64[n], p64[n][i2[n]]
        sums = np.concatenate([[float((r1 * r1).sum())], r1.sum(0).numpy(), (pa.t() @ r1).reshape(-1).numpy(),
                               [float((r2 * r2).sum())], r2.sum(0).numpy(), (pb.t() @ r2).reshape(-1).numpy()])
        loss += (sums[0] / P1 + sums[13] / P2) / N
        loss_abs += (sums[0] / P1 + sums[13] / P2) / N                  # (every term of the loss is a square: the sum of absolute terms)
        # one fp32 Adam step from these sums (the host build of the same header): 2 ulp
        param = np.array([1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1], np.float32)
        m, v, blk, ref = np.zeros(12, np.float32), np.zeros(12, np.float32), np.zeros(12, np.float32), np.zeros(15, np.float32)
        sums = np.ascontiguousarray(sums, dtype=np.float64)
        host_lib().host_icp_step(_p(param), _p(m), _p(v), _p(sums), N, P1, P2, 1, 1, 0.01, 1, _p(blk), _p(ref))
        dev = torch.cat([x[n].reshape(-1) for x in _rts(o['trace'], 0, N)]).numpy()
        # (T and s are parameters: their own ulp; the entries of R are products of the unit vectors made from R6: the ulp of 1)
        floor = np.concatenate([np.ones(9), np.zeros(6)]).astype(np.float32)
        err, ulp = np.abs(dev.astype(np.float64) - ref), np.spacing(np.maximum(np.abs(ref), floor))
        print('instance', n, 'largest parameter difference in ulp:', float((err / ulp).max()))
        assert (err <= 2 * ulp).all()
        assert np.array_equal(dev, rts[n])                              # iteration 0 is kept: the outputs are the trace's parameters
    print('loss', o['trace'][0, 0].item(), 'fp64 torch', loss, 'relative', abs(o['trace'][0, 0].item() - loss) / loss_abs)
    assert abs(o['trace'][0, 0].item() - loss) <= 1e-11 * loss_abs


@pytest.mark.parametrize('anisotropic', [False, True])
def test_trajectory_against_the_fp64_torch_loop(anisotropic):
    pp, pg = fx.ellipsoid_pair()
    spread = fx.reference_spread(anisotropic)
    assert spread <= ILL_CONDITIONED, f'ill-conditioned input: the fp32 and fp64 torch runs differ by {spread}'
    cloud, (R, T, s), trace = fx.torch_run(torch.float64, anisotropic)
    upd, (dR, dT, ds), dtrace = eval3d.gradient_icp(pp.to(DEV), pg.to(DEV), True, anisotropic, lr=0.01, n_iter=31, return_trace=True)
    assert ds.shape == s.shape and upd.dtype == torch.float32 and upd.device.type == 'cuda'
    errs = {k: float((a.cpu().double() - b).abs().max()) for k, a, b in (('R', dR, R), ('T', dT, T), ('s', ds, s), ('cloud', upd, cloud))}
    print('reference spread', spread, 'device differences', errs)
    assert max(errs.values()) <= 8 * spread
    assert dtrace['best_iter'] == 30 == trace['best_iter']
    assert abs(dtrace['best_loss'] - trace['best_loss']) <= 8 * spread


@pytest.mark.parametrize('case', ['lr0.3', 'aligned'])
def test_keep_best_rule_on_the_device(case):
    (pp, pg), lr = (fx.ellipsoid_pair(), 0.3) if case == 'lr0.3' else (fx.aligned_pair(), 0.01)
    N = len(pp)
    o = _run(pp, pg, estimate_scale=True, anisotropic_scale=True, lr=lr, n_iter=41)
    best_loss, best_iter, checks = eval3d.keep_best_history(o['trace'][:, 0].tolist(), N)
    print(case, 'checks (iteration, average, kept):', checks)
    assert [c[0] for c in checks] == [0, 10, 20, 30, 40] and checks[0][2]
    assert not all(c[2] for c in checks), 'the input no longer reaches the no-update branch'
    assert o['best'].tolist() == [best_loss, float(best_iter)]
    R, T, s = _rts(o['trace'], best_iter, N)
    assert torch.equal(o['R'], R) and torch.equal(o['T'], T) and torch.equal(o['s'], s)


def test_run_to_run_identity_and_independence_of_splits():
    pp, pg = fx.ellipsoid_pair()
    runs = [_run(pp, pg, estimate_scale=True, anisotropic_scale=True, lr=0.01, n_iter=11, splits=sp) for sp in (0, 0, 1, 3)]
    for o in runs[1:]:
        for k in ('cloud', 'R', 'T', 's', 'best', 'trace'):
            assert torch.equal(o[k], runs[0][k]), k


@pytest.mark.parametrize('N', [1, 3])
def test_batch_sizes(N):
    """N = 1 and N = 3 against the fp64 torch loop, with the bar of the trajectory test computed for this input"""
    pp, pg = fx.ellipsoid_pair()
    pp, pg = pp[[0, 1, 0][:N], :700], pg[[0, 1, 1][:N], :500]
    ref32 = eval3d.gradient_icp_torch(pp, pg, True, True, lr=0.01, n_iter=11)
    ref64 = eval3d.gradient_icp_torch(pp.double(), pg.double(), True, True, lr=0.01, n_iter=11)
    spread = max(float((a.double() - b).abs().max()) for a, b in zip([ref32[0]] + ref32[1], [ref64[0]] + ref64[1]))
    assert spread <= ILL_CONDITIONED
    upd, prm = eval3d.gradient_icp(pp.to(DEV), pg.to(DEV), True, True, lr=0.01, n_iter=11)
    err = max(float((a.cpu().double() - b).abs().max()) for a, b in zip([upd] + prm, [ref64[0]] + ref64[1]))
    print('N', N, 'reference spread', spread, 'device difference', err)
    assert err <= 8 * spread


def test_edges():
    pp, pg = fx.ellipsoid_pair()
    # fewer pred points than one workgroup, one ground-truth point: every pred point pairs with it, and it with its nearest pred point
    a, b = pp[:1, :200], pg[:1, :1]
    o = _run(a, b, estimate_scale=True, anisotropic_scale=False, lr=0.01, n_iter=3)
    d = (a.double() - b.double()).pow(2).sum(2)
    assert abs(o['trace'][0, 0].item() - float(d.mean() + d.min())) <= 1e-11 * float(d.mean() + d.min())
    assert torch.isfinite(o['cloud']).all() and o['trace'][2, 0] < o['trace'][0, 0] and o['best'][1] == 0
    assert torch.equal(o['s'][:, 0], o['s'][:, 1]) and torch.equal(o['s'][:, 0], o['s'][:, 2])
    # n_iter = 0: the identity and the input cloud, nothing kept
    o = _run(pp, pg, estimate_scale=True, anisotropic_scale=True, n_iter=0)
    assert torch.equal(o['cloud'], pp) and torch.equal(o['R'], torch.eye(3).expand(2, 3, 3)) and not o['T'].any() and (o['s'] == 1).all()
    assert o['best'].tolist() == [1e6, -1.0] and o['trace'].shape == (0, 31)
    upd, (R, T, s) = eval3d.gradient_icp(pp.to(DEV), pg.to(DEV), n_iter=0)
    assert torch.equal(upd.cpu(), pp) and s.shape == (2, 1)
    # estimate_scale = False leaves s at 1 in every iteration
    o = _run(pp, pg, estimate_scale=False, anisotropic_scale=True, lr=0.01, n_iter=11)
    assert (o['trace'][:, 1:].reshape(11, 2, 15)[..., 12:] == 1).all() and (o['s'] == 1).all() and o['T'].abs().min() > 0
    upd, (R, T, s) = eval3d.gradient_icp(pp.to(DEV), pg.to(DEV), estimate_scale=False, n_iter=1)
    assert s.shape == (2, 3)


def test_mesh_evaluator_against_the_cpu_path():
    """the sphere pair at the fast_cpu settings cut to 5 000 points: the same samples, drawn once on the CPU, scored on the device and held
    against the CPU path's fp64 scores (recorded: tests/golden/icp_sphere_scores.json, tests/test_icp_host.py holds the CPU path to them);
    the bar is the trajectory test's, 8 x the difference of the recorded fp32 and fp64 CPU scores"""
    (vp, faces), pc_gt, norm_gt, ev, samples = fx.sphere_case()
    g = fx.sphere_golden()
    assert fx.sphere_checksum() == pytest.approx(g['checksum'], rel=1e-9)      # the same draw as recorded
    c64 = g['fp64']
    spread = max(abs(g['fp32'][k] - c64[k]) for k in c64)
    assert spread <= ILL_CONDITIONED * metrics.CHAMFER_FACTOR
    dev = ev.evaluate((vp.to(DEV), faces.to(DEV)), pc_gt, norm_gt, samples=samples)
    print('cpu fp64', c64, 'device', dict(dev), 'reference spread', spread)
    assert sorted(dev) == sorted(c64) and max(abs(dev[k] - c64[k]) for k in c64) <= 8 * spread
    assert dev['chamfer-L1-ICP'] < 0.5 * dev['chamfer-L1']


def test_evaluate_aligned_end_to_end(tmp_path):
    """a small model's live blocks against a ground truth in another frame and scale, 5 000 points: evaluate_aligned on the device, with the
    recorded samples (tests/golden/icp_blocks_inputs.npz, drawn once on the CPU from these blocks), held against the CPU path's fp64 scores
    (tests/golden/icp_blocks_scores.json) with the bar of the trajectory test: 8 x the difference of the recorded fp32 and fp64 CPU scores"""
    model = fx.blocks_model(DEV)
    verts_unit, gt, gt_n, samples = fx.blocks_case()
    g = fx.blocks_golden()
    c64 = g['fp64']
    spread = max(abs(g['fp32'][k] - c64[k]) for k in c64)
    assert 0 < spread <= ILL_CONDITIONED * metrics.CHAMFER_FACTOR
    # the recorded samples belong to this model's blocks: the same mesh in the ground truth's unit-cube frame (a few fp32 operations per
    # coordinate of size <= 1 on another processor: 1e-5 tells the same mesh from another one, it is no precision claim)
    verts, faces = model.blocks_mesh(filter_transparent=True)
    off, sc = eval3d.unit_cube_frame(gt.to(DEV))
    assert verts.shape == verts_unit.shape and float((((verts.detach() - off) / sc).cpu() - verts_unit).abs().max()) <= 1e-5
    s = eval3d.evaluate_aligned(model, gt, gt_n, eval_dir=tmp_path / 'run', samples=samples, fast_cpu=True, n_points=5000)
    print('cpu fp64', c64, 'device', dict(s), 'reference spread', spread)
    assert list(s) == ['chamfer-L1', 'normal-cos', 'chamfer-L1-ICP', 'normal-cos-ICP']
    assert max(abs(s[k] - c64[k]) for k in c64) <= 8 * spread
    # the same scores as the evaluator called by hand on the same frame and samples
    ev = fx.blocks_evaluator()
    by_hand = ev.evaluate(((verts.detach() - off) / sc, faces), (gt.to(DEV) - off) / sc, gt_n, samples=samples)
    assert dict(by_hand) == dict(s)
    head, vals, end = (tmp_path / 'run' / 'aligned_scores.tsv').read_text().split('\n')
    assert head == 'chamfer-L1\tnormal-cos\tchamfer-L1-ICP\tnormal-cos-ICP' and end == ''
    assert vals.split('\t') == ['{:.5f}'.format(v) for v in s.values()]
    # without normals and without a directory: the Chamfer scores alone, no file
    s2 = eval3d.evaluate_aligned(model, gt, samples=samples, fast_cpu=True, n_points=5000)
    assert list(s2) == ['chamfer-L1', 'chamfer-L1-ICP'] and s2['chamfer-L1'] == s['chamfer-L1']


def test_trainer_evaluate_with_and_without_aligned(tmp_path):
    """Trainer.evaluate(aligned=dict(...)) adds the scores of evaluate_aligned under 'aligned' and writes aligned_scores.tsv next to
    final_scores.tsv; with aligned left at None neither appears and the other scores are the same set"""
    from dbw_amd.trainer import Trainer
    from test_gpu_export import _loader, _scenes
    model, blocks, full, inp = _scenes(views=4, kill=True)
    cfg = {'training': {'batch_size': 2, 'n_epoches': 1, 'seed': 3, 'optimizer': {'name': 'adam', 'lr': 1e-3}, 'scheduler': {'name': 'multi_step'}}}
    tr = Trainer(cfg, model, inp)
    loader = _loader(inp)
    gen = torch.Generator().manual_seed(2)
    gt = torch.rand(800, 3, generator=gen) * torch.tensor([30., 20., 10.]) + torch.tensor([5., -3., 2.])
    gt_n = torch.nn.functional.normalize(torch.randn(800, 3, generator=gen), dim=1)
    kw = dict(points=gt, normals=gt_n, fast_cpu=True, n_points=600, generator=torch.Generator(device=DEV).manual_seed(4))
    plain = tr.evaluate(loader, tmp_path / 'plain')
    assert 'aligned' not in plain and not (tmp_path / 'plain' / 'aligned_scores.tsv').exists()
    scores = tr.evaluate(loader, tmp_path / 'run', aligned=kw)
    # (the image scores themselves are not compared between the two calls: the render path's float atomics make them differ in the last bits)
    assert list(scores) == list(plain) + ['aligned']
    want = eval3d.evaluate_aligned(model, gt, gt_n, fast_cpu=True, n_points=600, generator=torch.Generator(device=DEV).manual_seed(4))
    assert scores['aligned'] == dict(want) and list(want) == ['chamfer-L1', 'normal-cos', 'chamfer-L1-ICP', 'normal-cos-ICP']
    head, vals, end = (tmp_path / 'run' / 'aligned_scores.tsv').read_text().split('\n')
    assert head.split('\t') == list(want) and vals.split('\t') == ['{:.5f}'.format(v) for v in want.values()] and end == ''
    assert (tmp_path / 'run' / 'final_scores.tsv').read_text().split('\n')[0] == (tmp_path / 'plain' / 'final_scores.tsv').read_text().split('\n')[0]
