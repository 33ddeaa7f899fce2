"""GPU tests of the 3D evaluation (run with `-m gpu`): the HIP nearest-neighbour search bit-equal to the torch brute force, the Chamfer
distance, the DTU lattice / downsample / full protocol against the REAL reference's fixtures (tests/golden/chamfer.npz, dtu_tiny.npz),
the model's blocks mesh against the oracle, evaluate_dtu end to end, and the mesh sampler."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle as O                                              # noqa: E402  (checker only)
import dbw_amd                                                  # noqa: E402
from dbw_amd import eval3d                                      # noqa: E402
from test_eval3d_host import run_chamfer_case, sequential_downsample     # noqa: E402

DEV = 'cuda:0'


def _same(a, b):
    return torch.equal(a.cpu(), b.cpu())


def check_nn(x, y, xl=None, yl=None, splits=0):
    d, i = eval3d.nn_points(x.to(DEV), y.to(DEV), None if xl is None else xl.to(DEV), None if yl is None else yl.to(DEV), splits=splits)
    rd, ri = eval3d.nn_points(x.cpu(), y.cpu(), xl, yl)
    assert _same(i, ri), int((i.cpu() != ri).sum())
    assert torch.equal(d.cpu().view(torch.int32), rd.view(torch.int32))
    return d, i


def test_nn_points_bit_equal_to_the_cpu_path():
    g = torch.Generator().manual_seed(0)
    # duplicated points and whole duplicated clouds: the lowest index wins every tie
    y = torch.rand(1, 3001, 3, generator=g)
    y = torch.cat([y, y[:, :1000], torch.round(y * 8) / 8], 1)
    x = torch.cat([torch.rand(1, 2049, 3, generator=g), y[:, 2500:3500], torch.round(torch.rand(1, 777, 3, generator=g) * 8) / 8], 1)
    d, i = check_nn(x, y)
    assert int((i[0, 2049:2549] == torch.arange(2500, 3000, device=DEV)).sum()) == 500      # (exact copies, first occurrence)
    check_nn(x, y, splits=7)
    # N > 1, heterogeneous lengths, an empty y cloud, P not a multiple of any tile
    x = torch.randn(4, 2500, 3, generator=g)
    y = torch.randn(4, 1337, 3, generator=g)
    xl, yl = torch.tensor([2500, 17, 0, 1999]), torch.tensor([1337, 600, 5, 0])
    d, i = check_nn(x, y, xl, yl)
    assert bool((i[1, 17:] == -1).all()) and bool((d[1, 17:] == 0).all()) and bool((i[2] == -1).all())
    assert bool((i[3, :1999] == -1).all()) and bool(torch.isinf(d[3, :1999]).all())
    check_nn(x, y, xl, yl, splits=3)


def test_nn_points_split_merge_and_run_to_run_identity():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 64, 3, generator=g)
    y = torch.randn(1, 300_000, 3, generator=g)
    y[0, 123_456] = x[0, 5]                     # an exact hit far into the range
    y[0, 200_001] = x[0, 5]                     # ... and its duplicate later: the first one wins
    d, i = check_nn(x, y)                        # small P1, large P2: the y range is split across workgroups
    assert int(i[0, 5]) == 123_456 and float(d[0, 5]) == 0.0
    d1, i1 = check_nn(x, y, splits=1)
    d2, i2 = eval3d.nn_points(x.to(DEV), y.to(DEV))
    assert _same(i1, i2) and torch.equal(d1.view(torch.int32), d2.view(torch.int32))


def test_nn_points_large_against_chunked_torch_on_the_device():
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.rand(1, 200_000, 3, generator=g, device=DEV) * 100
    y = torch.rand(1, 300_000, 3, generator=g, device=DEV) * 100
    d, i = eval3d.nn_points(x, y)
    rd, ri = eval3d.nn_points_torch(x, y, chunk_elems=1 << 27)
    assert torch.equal(i, ri) and torch.equal(d.view(torch.int32), rd.view(torch.int32))
    d2, i2 = eval3d.nn_points(x, y)
    assert torch.equal(i, i2) and torch.equal(d.view(torch.int32), d2.view(torch.int32))


@pytest.mark.parametrize('k', range(7))
def test_chamfer_distance_on_the_device_matches_the_reference(golden_dir, k):
    run_chamfer_case(np.load(os.path.join(golden_dir, 'chamfer.npz')), k, DEV)


def _fixture_cloud(g):
    pts, counts = eval3d.dense_lattice(torch.from_numpy(g['verts']).to(DEV), torch.from_numpy(g['faces']).to(DEV))
    return pts, counts


def test_lattice_kernels_match_the_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, 'dtu_tiny.npz'))
    pts, counts = _fixture_cloud(g)
    assert np.array_equal(counts.cpu().numpy(), g['counts'])
    assert pts.shape[0] == int(g['n_points'])
    sub = pts[torch.from_numpy(g['lattice_idx']).to(DEV)].cpu().numpy()
    assert np.array_equal(sub.view(np.uint64), g['lattice_points'].view(np.uint64))


def test_downsample_kernel_matches_the_reference_and_the_sequential_loop(golden_dir, record_property):
    g = np.load(os.path.join(golden_dir, 'dtu_tiny.npz'))
    pts, _ = _fixture_cloud(g)
    keep, rounds = eval3d.radius_downsample(pts[torch.from_numpy(g['perm']).to(DEV)].contiguous(), 0.2)
    assert np.array_equal(keep.cpu().numpy(), g['keep'])
    record_property('rounds_fixture', rounds)
    gen = np.random.default_rng(3)
    p = gen.uniform(0, 10, (50_000, 3))
    for r in (0.1, 0.2, 0.45):
        keep, rounds = eval3d.radius_downsample(torch.from_numpy(p).to(DEV), r)
        assert np.array_equal(keep.cpu().numpy(), sequential_downsample(p, r)), r
        record_property(f'rounds_50k_r{r}', rounds)
        print(f'downsample 50k random points, radius {r}: {rounds} rounds')


def test_dtu_scores_with_the_reference_permutation(golden_dir):
    g = np.load(os.path.join(golden_dir, 'dtu_tiny.npz'))
    s = eval3d.dtu_scores(g['verts'], g['faces'], g['obs_mask'], g['bb'], g['res'], g['plane'], g['stl'], order=g['perm'], device=DEV)
    for k in ('n_points', 'n_down', 'n_in_obs', 'n_stl_above', 'n_d2s', 'n_s2d', 'n_vertices'):
        assert s[k] == int(g[k]), (k, s[k], int(g[k]))
    assert s['n_lattice'] == int(g['counts'].sum())
    for k in ('acc', 'comp', 'avg'):
        assert abs(s[k] - float(g[k])) <= 1e-6 * abs(float(g[k])), (k, s[k], float(g[k]))


def _model(sync_free):
    cfg = {'model': {'name': 'dbw', 'mesh': {'n_blocks': 4, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': 256},
                     'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                     'rend_optim': {'coarse_learning': 1500, 'decimate_txt': 750, 'decimate_factor': 8, 'kill_blocks': True,
                                    'decouple_rendering': True, 'opacity_noise': True},
                     'loss': {'rgb_weight': 1, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}}}
    torch.manual_seed(227391)
    model = dbw_amd.create_model(cfg, (75, 100))
    orc = O.OracleDBW((75, 100), n_blocks=4, txt_size=256, faces_per_pixel=4, seed=227391)
    with torch.no_grad():
        gen = torch.Generator().manual_seed(1)
        for name, scale in (('sq_eps', 1.5), ('T', 0.3), ('R_6d', 0.3), ('S', 0.3)):
            d = torch.randn(orc.p[name].shape, generator=gen) * scale
            orc.p[name].add_(d)
            getattr(model, name).add_(d)
        for k, v in ((1, -2.0), (3, -0.5), (0, 1.0), (2, 0.2)):           # two blocks below the 0.5 filter
            orc.p['alpha_logit'][k] = v
            model.alpha_logit[k] = v
    model = model.to(DEV)
    model.sync_free = sync_free
    return model, orc


@pytest.mark.parametrize('sync_free', [False, True])
def test_blocks_mesh_matches_the_oracle(sync_free):
    model, orc = _model(sync_free)
    model.train()
    verts, faces = model.blocks_mesh(filter_transparent=True)
    ref = orc.build_blocks(training=False, coarse=False, decimate=False, filter_transparent=True)
    assert faces.dtype == torch.int64 and verts.dtype == torch.float32
    assert torch.equal(faces.cpu(), ref['faces'].to(torch.int64))
    assert verts.shape == ref['verts'].shape
    assert float((verts.cpu() - ref['verts'].detach()).abs().max()) <= 1e-5
    assert model.sync_free == sync_free


def _write_dtu_dir(root, scan_id, verts_dtu, rng):
    import scipy.io
    os.makedirs(os.path.join(root, 'ObsMask'))
    os.makedirs(os.path.join(root, 'Points', 'stl'))
    lo, hi = verts_dtu.min(0) - 5, verts_dtu.max(0) + 5
    scipy.io.savemat(os.path.join(root, 'ObsMask', f'ObsMask{scan_id}_10.mat'),
                     {'ObsMask': np.ones((32, 32, 32), np.uint8), 'BB': np.stack([lo, hi]).astype(np.float64), 'Res': np.array([[float((hi - lo).max() / 31)]])})
    scipy.io.savemat(os.path.join(root, 'ObsMask', f'Plane{scan_id}.mat'), {'P': np.array([[0.], [0.], [1.], [-float(lo[2]) + 1]])})
    stl = verts_dtu[rng.integers(0, len(verts_dtu), 2000)] + rng.normal(0, 0.5, (2000, 3))
    hdr = f'ply\nformat binary_little_endian 1.0\nelement vertex {len(stl)}\nproperty float x\nproperty float y\nproperty float z\nend_header\n'
    with open(os.path.join(root, 'Points', 'stl', f'stl{scan_id:03}_total.ply'), 'wb') as f:
        f.write(hdr.encode() + stl.astype('<f4').tobytes())


def test_evaluate_dtu_end_to_end(tmp_path):
    model, _ = _model(False)
    model.eval()
    scale = torch.tensor([[40., 0, 0, 1.], [0, 40., 0, -2.], [0, 0, 40., 3.], [0, 0, 0, 1.]])
    verts, faces = model.blocks_mesh()
    v_dtu = (verts @ scale[:3, :3].to(DEV) + scale[:3, 3].to(DEV)).cpu().numpy().astype(np.float64)
    _write_dtu_dir(str(tmp_path / 'DTU'), 24, v_dtu, np.random.default_rng(0))
    s = eval3d.evaluate_dtu(model, scale, 24, str(tmp_path / 'DTU'), str(tmp_path / 'run'), seed=0)
    assert np.isfinite([s['acc'], s['comp'], s['avg']]).all() and s['n_down'] > 0 and s['n_in_obs'] > 0
    head, vals = (tmp_path / 'run' / 'dtu_scores.tsv').read_text().split('\n')
    assert head == 'acc\tcomp\tavg' and [float(v) for v in vals.split('\t')] == [s['acc'], s['comp'], s['avg']]
    # the same seed, the same scores
    s2 = eval3d.evaluate_dtu(model, scale, 24, str(tmp_path / 'DTU'), str(tmp_path / 'run'), suffix='_b', seed=0)
    assert s2 == s


def test_sample_points_from_meshes():
    from scipy.stats import chi2
    g = torch.Generator(device=DEV).manual_seed(4)
    verts = torch.randn(30, 3, device=DEV, generator=g)
    faces = torch.randint(0, 30, (40, 3), device=DEV, generator=g)
    faces = faces[(faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])]
    S = 200_000
    pts, nrm, fidx = eval3d.sample_points_from_meshes(verts, faces, S, return_normals=True, generator=g, return_face_idx=True)
    assert pts.shape == (1, S, 3) and nrm.shape == (1, S, 3)
    v0, v1, v2 = (verts[faces[fidx, k]].double() for k in range(3))
    p = pts[0].double()
    # barycentrics of the point in its face (least squares on the two edges): in range, and the point lies on the face
    e1, e2, q = v1 - v0, v2 - v0, p - v0
    a11, a12, a22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    b1, b2 = (q * e1).sum(1), (q * e2).sum(1)
    det = a11 * a22 - a12 * a12
    w1, w2 = (a22 * b1 - a12 * b2) / det, (a11 * b2 - a12 * b1) / det
    assert float((q - w1[:, None] * e1 - w2[:, None] * e2).norm(dim=1).max()) < 1e-5
    assert float(w1.min()) > -1e-5 and float(w2.min()) > -1e-5 and float((w1 + w2).max()) < 1 + 1e-5
    fn = torch.linalg.cross(v1 - v0, v2 - v1, dim=1)
    fn = fn / fn.norm(dim=1, keepdim=True)
    assert float((nrm[0].double() - fn).abs().max()) < 1e-5 and float((nrm[0].double().norm(dim=1) - 1).abs().max()) < 1e-5
    fv = verts[faces].double()
    area = 0.5 * torch.linalg.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1).norm(dim=1)
    expected = (area / area.sum() * S).cpu().numpy()
    observed = torch.bincount(fidx, minlength=len(faces)).cpu().numpy()
    stat = float(((observed - expected) ** 2 / expected).sum())
    assert stat < chi2.ppf(0.999, len(faces) - 1), stat
