"""CPU tests of the 3D evaluation (dbw_amd/eval3d.py, csrc/nn_math.h, include/dbw_eval.h), no GPU needed:
  * nn_math.h built by g++ (tests/host_nn_math.cpp): the DTU lattice counts and points bit-exact against a numpy restatement of
    dtu_eval.py:21-30,56-78 and against the REAL reference's cloud (tests/golden/dtu_tiny.npz), the distance formula bit-exact against torch;
  * eval3d.chamfer_distance on CPU tensors against the REAL reference's chamfer_distance (tests/golden/chamfer.npz): values and gradients;
  * the sequential greedy downsample (restated) against the reference's keep mask; the PLY / .mat readers; the TSV format;
  * the C ABI of include/dbw_eval.h: validation before any launch (prototypes, revision, symbols: tests/test_abi_families.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from dbw_amd import _lib, eval3d
from host_build import host_lib


def lib():
    return host_lib('nn_math')


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def host_lattice(tri):
    tri = np.ascontiguousarray(tri, dtype=np.float64)
    F = len(tri)
    counts = np.zeros(F, np.int64)
    lib().host_lattice_counts(_p(tri), ctypes.c_longlong(F), _p(counts))
    offsets = np.ascontiguousarray(np.cumsum(counts) - counts)
    pts = np.zeros((int(counts.sum()), 3))
    lib().host_lattice_points(_p(tri), ctypes.c_longlong(F), _p(counts), _p(offsets), _p(pts))
    return counts, pts


def numpy_lattice(tri):
    """dtu_eval.py:56-78 restated face by face (the reference's expressions; the pool map is a loop)"""
    counts, pts = [], []
    for t in tri:
        v1, v2 = t[1:2] - t[0:1], t[2:3] - t[0:1]
        l1, l2 = np.linalg.norm(v1, axis=-1, keepdims=True), np.linalg.norm(v2, axis=-1, keepdims=True)
        area2 = np.linalg.norm(np.cross(v1, v2), axis=-1, keepdims=True)
        if not (area2 > 0)[0, 0]:
            counts.append(0)
            continue
        thr = 0.2 * np.sqrt(l1 * l2 / area2)
        n1, n2 = np.floor(l1 / thr)[0, 0], np.floor(l2 / thr)[0, 0]
        c = np.mgrid[:n1 + 1, :n2 + 1]
        c += 0.5
        c[0] /= max(n1, 1e-7)
        c[1] /= max(n2, 1e-7)
        c = np.transpose(c, (1, 2, 0))
        k = c[c.sum(axis=-1) < 1]
        q = v1 * k[:, :1] + v2 * k[:, 1:] + t[0:1]
        counts.append(len(q))
        pts.append(q)
    return np.array(counts, np.int64), (np.concatenate(pts) if pts else np.zeros((0, 3)))


def test_lattice_bit_exact_against_numpy():
    rng = np.random.default_rng(0)
    tri = [rng.normal(0, 3, (3, 3)) for _ in range(60)]
    # near-equilateral faces (n1 == n2: the anti-diagonal ties), slivers, a degenerate and a tiny face
    for s in (1.0, 2.3, 4.1, 7.7):
        tri.append(np.array([[0, 0, 0], [s, 0, 0], [s / 2, s * np.sqrt(3) / 2, 0]]) + rng.normal(0, 1, 3))
        tri.append(np.array([[0, 0, 0], [s, 0, 0], [0, s, 0]], float))
    tri += [np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2.]]), np.array([[0, 0, 0], [5, 0, 0], [5, 0.01, 0]]), np.full((3, 3), 1.5),
            np.array([[0, 0, 0], [0.05, 0, 0], [0, 0.05, 0]])]
    tri = np.stack(tri).astype(np.float32).astype(np.float64)       # vertices are fp32 values, as the reference's
    counts, pts = host_lattice(tri)
    rc, rp = numpy_lattice(tri)
    assert np.array_equal(counts, rc)
    assert pts.shape == rp.shape and np.array_equal(pts.view(np.uint64), rp.view(np.uint64))
    assert counts[-4] == 0 and counts[-2] == 0


def test_lattice_matches_the_reference_cloud(golden_dir):
    g = np.load(os.path.join(golden_dir, 'dtu_tiny.npz'))
    V, F_ = g['verts'].astype(np.float64), g['faces']
    counts, pts = host_lattice(V[F_])
    assert np.array_equal(counts, g['counts'])
    assert int(g['n_vertices']) + counts.sum() == int(g['n_points'])
    sub = g['lattice_idx'] - int(g['n_vertices'])
    assert np.array_equal(pts[sub].view(np.uint64), g['lattice_points'].view(np.uint64))


def test_distance_formula_bit_exact_against_torch():
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(100000, 3, generator=gen) * torch.tensor([1e3, 1., 1e-3])[torch.randint(0, 3, (100000, 1), generator=gen)]
    y = x + torch.randn(100000, 3, generator=gen) * 0.01
    d = x - y
    ref = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    out = np.zeros(100000, np.float32)
    xs, ys = np.ascontiguousarray(x.numpy()), np.ascontiguousarray(y.numpy())
    lib().host_nn_dist2(_p(xs), _p(ys), ctypes.c_longlong(100000), _p(out))
    assert np.array_equal(out.view(np.uint32), ref.numpy().view(np.uint32))
    # the CPU path of nn_points uses the same expression and keeps the lowest index of a tie
    dist2, idx = eval3d.nn_points(x[None, :300], torch.cat([y[:200], y[:200]])[None])
    assert idx.max() < 200


def _chamfer_case(g, k):
    kw = eval(str(g[f'c{k}_kwargs']))
    t = {n: torch.from_numpy(g[n]) for n in ('x', 'y', 'x_normals', 'y_normals', 'x_lengths', 'y_lengths', 'weights')}
    args = dict(return_L1=kw['return_L1'], batch_reduction=kw.get('batch_reduction', 'mean'), point_reduction=kw.get('point_reduction', 'mean'),
                direction_reduction=kw.get('direction_reduction', 'sum'))
    if kw.get('lengths'):
        args.update(x_lengths=t['x_lengths'], y_lengths=t['y_lengths'])
    if kw.get('weights'):
        args['weights'] = t['weights']
    return kw, t, args


def run_chamfer_case(g, k, device):
    kw, t, args = _chamfer_case(g, k)
    x, y = t['x'].to(device).requires_grad_(True), t['y'].to(device).requires_grad_(True)
    xn, yn = t['x_normals'].to(device).requires_grad_(True), t['y_normals'].to(device).requires_grad_(True)
    args = {a: (v.to(device) if torch.is_tensor(v) else v) for a, v in args.items()}
    if kw.get('normals'):
        args.update(x_normals=xn, y_normals=yn)
    dist, nrm = eval3d.chamfer_distance(x, y, **args)
    vals = list(dist) if isinstance(dist, tuple) else [dist]
    if nrm is not None:
        vals += list(nrm) if isinstance(nrm, tuple) else [nrm]
    assert len(vals) == int(g[f'c{k}_n_out'])
    for j, v in enumerate(vals):
        np.testing.assert_allclose(v.detach().cpu().numpy(), g[f'c{k}_out{j}'], rtol=1e-6, atol=1e-7, err_msg=f'case {k} output {j}')
    sum(v.sum() for v in vals).backward()
    if bool(g[f'c{k}_has_grad']):
        pairs = [(x, 'grad_x'), (y, 'grad_y')] + ([(xn, 'grad_xn'), (yn, 'grad_yn')] if kw.get('normals') else [])
        for tens, name in pairs:
            ref = g[f'c{k}_{name}']
            np.testing.assert_allclose(tens.grad.cpu().numpy(), ref, rtol=1e-6, atol=1e-6 * max(1.0, np.abs(ref).max()),
                                       err_msg=f'case {k} {name}')


@pytest.mark.parametrize('k', range(7))
def test_chamfer_distance_matches_the_reference_on_cpu(golden_dir, k):
    run_chamfer_case(np.load(os.path.join(golden_dir, 'chamfer.npz')), k, 'cpu')


def sequential_downsample(pts, radius):
    """dtu_eval.py:82-96 restated: in order, point i is kept iff no earlier kept point lies within radius"""
    from scipy.spatial import cKDTree
    nbrs = cKDTree(pts).query_ball_point(pts, radius)
    mask = np.ones(len(pts), np.bool_)
    for curr, idxs in enumerate(nbrs):
        if mask[curr]:
            mask[idxs] = 0
            mask[curr] = 1
    return mask


def test_sequential_downsample_matches_the_reference_keep_mask(golden_dir):
    g = np.load(os.path.join(golden_dir, 'dtu_tiny.npz'))
    V, F_ = g['verts'].astype(np.float64), g['faces']
    used = np.zeros(len(V), bool)
    used[F_.reshape(-1)] = True
    _, pts = host_lattice(V[F_])
    cloud = np.concatenate([V[used], pts])[g['perm']]
    keep = sequential_downsample(cloud, 0.2)
    assert np.array_equal(keep, g['keep']) and int(keep.sum()) == int(g['n_down'])


def test_ply_reader_binary_and_ascii(tmp_path):
    rng = np.random.default_rng(2)
    pts = rng.normal(0, 100, (257, 3)).astype(np.float32)
    rgb = rng.integers(0, 255, (257, 3)).astype(np.uint8)
    hdr = ('ply\nformat {}\ncomment x\nelement vertex 257\nproperty float x\nproperty float y\nproperty float z\n'
           'property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n')
    dt = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('r', 'u1'), ('g', 'u1'), ('b', 'u1')])
    rec = np.zeros(257, dt)
    rec['x'], rec['y'], rec['z'], rec['r'], rec['g'], rec['b'] = pts[:, 0], pts[:, 1], pts[:, 2], rgb[:, 0], rgb[:, 1], rgb[:, 2]
    (tmp_path / 'b.ply').write_bytes(hdr.format('binary_little_endian 1.0').encode() + rec.tobytes() + b'\x03\x00\x00\x00\x00\x01\x00\x00\x00\x02\x00\x00\x00')
    lines = ''.join(f'{float(a)!r} {float(b)!r} {float(c)!r} {r} {gg} {bb}\n' for (a, b, c), (r, gg, bb) in zip(pts, rgb))
    (tmp_path / 'a.ply').write_text(hdr.format('ascii 1.0') + lines + '3 0 1 2\n')
    for name in ('a.ply', 'b.ply'):
        out = eval3d.read_ply_points(str(tmp_path / name))
        assert out.dtype == np.float64 and np.array_equal(out, pts.astype(np.float64)), name


def test_mat_files_and_tsv_format(tmp_path):
    import scipy.io
    os.makedirs(tmp_path / 'ObsMask')
    os.makedirs(tmp_path / 'Points' / 'stl')
    obs = (np.random.default_rng(0).random((4, 5, 6)) > 0.5).astype(np.uint8)
    scipy.io.savemat(str(tmp_path / 'ObsMask' / 'ObsMask24_10.mat'), {'ObsMask': obs, 'BB': np.array([[0., 1, 2], [3, 4, 5]]), 'Res': np.array([[0.5]])})
    scipy.io.savemat(str(tmp_path / 'ObsMask' / 'Plane24.mat'), {'P': np.array([[0.], [0], [1], [2]])})
    (tmp_path / 'Points' / 'stl' / 'stl024_total.ply').write_text('ply\nformat ascii 1.0\nelement vertex 2\nproperty double x\nproperty double y\n'
                                                                 'property double z\nend_header\n1 2 3\n4 5 6\n')
    o, bb, res, plane, stl = eval3d.load_dtu_scan(24, str(tmp_path))
    assert np.array_equal(o, obs) and bb.shape == (2, 3) and float(res[0, 0]) == 0.5 and plane.reshape(4).tolist() == [0, 0, 1, 2]
    assert stl.tolist() == [[1, 2, 3], [4, 5, 6]]
    # dtu_eval.py:162-164, byte for byte (np.float64 formats like a Python float; no newline at the end)
    a, c = np.float64(0.2424651911647909), np.float64(0.6273855587274263)
    eval3d.write_scores_tsv(str(tmp_path / 's.tsv'), a, c, (a + c) / 2)
    assert (tmp_path / 's.tsv').read_text() == f'acc\tcomp\tavg\n{a}\t{c}\t{(a + c) / 2}'


def test_tsv_matches_the_reference_bytes(golden_dir, tmp_path):
    g = np.load(os.path.join(golden_dir, 'dtu_tiny.npz'))
    eval3d.write_scores_tsv(str(tmp_path / 's.tsv'), float(g['acc']), float(g['comp']), float(g['avg']))
    assert (tmp_path / 's.tsv').read_text() == str(g['tsv'])


def test_eval_entry_points_validate_before_any_launch():
    lib = _lib.load()
    assert lib.dbw_nn_points(None, None, None, None, 1, 4, 4, 0, None, None, None, None) == -1
    assert b'null pointer' in lib.dbw_last_error()
    assert lib.dbw_dtu_lattice_counts(None, 3, None, None) == -1
    assert lib.dbw_radius_downsample_round(ctypes.c_void_p(8), ctypes.c_void_p(8), ctypes.c_void_p(8), 4, 3, 3, 0.2, ctypes.c_void_p(8),
                                           ctypes.c_void_p(8), None) == -1
    assert b'must differ' in lib.dbw_last_error()
    with pytest.raises(RuntimeError, match='bad size'):
        _lib.call('dbw_nn_points', ctypes.c_void_p(8), ctypes.c_void_p(8), None, None, 1, 0, 4, 0, ctypes.c_void_p(8), ctypes.c_void_p(8),
                  ctypes.c_void_p(8), None)
