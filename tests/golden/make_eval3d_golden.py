"""
Generates tests/golden/chamfer.npz and tests/golden/dtu_tiny.npz by running the REAL reference functions from /root/reference/src
(read-only; bytecode writing is disabled):
  utils/chamfer.py:7-160     chamfer_distance                (values and gradients, 7 cases)
  utils/dtu_eval.py:47-164   evaluate_mesh                   (the official DTU protocol on a tiny synthetic mm-scale scene)

Like make_golden.py it runs only where the reference checkout exists:   python tests/golden/make_eval3d_golden.py
The real numpy / scipy / sklearn / tqdm are used; pytorch3d and open3d (absent here) are replaced by minimal fakes that return arrays:
knn_points / knn_gather by a brute force, Meshes by a (verts, faces) holder, open3d's TriangleMesh by arrays with
remove_unreferenced_vertices (order kept), read_point_cloud by the synthetic stl cloud.  np.random.default_rng is patched so that the
shuffle of the dense cloud records its permutation; sklearn's NearestNeighbors is wrapped to record what the protocol fits and queries.
The fixtures are data only (inputs + expected outputs); no reference source travels.
"""
import collections
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
import numpy as np
import scipy.io
import sklearn.neighbors as skln
import torch

REF = '/root/reference/src'
HERE = os.path.dirname(os.path.abspath(__file__))
RADIUS, MAX_DIST = 0.2, 20.0


# ------------------------------------------------------------------------------------------------ fakes of pytorch3d / open3d
def _knn_points(p1, p2, lengths1=None, lengths2=None, K=1):
    assert K == 1
    N, P1, _ = p1.shape
    P2 = p2.shape[1]
    l2 = lengths2 if lengths2 is not None else torch.full((N,), P2, dtype=torch.int64)
    l1 = lengths1 if lengths1 is not None else torch.full((N,), P1, dtype=torch.int64)
    with torch.no_grad():
        d = p1[:, :, None, :].double() - p2[:, None, :, :].double()
        d2 = (d * d).sum(-1)
        d2[torch.arange(P2)[None, None, :].expand(N, P1, P2) >= l2[:, None, None]] = float('inf')
        idx = d2.argmin(-1)
    g = p2.gather(1, idx[..., None].expand(-1, -1, 3))
    dd = p1 - g
    dists = (dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]
    dists = torch.where(torch.arange(P1)[None] >= l1[:, None], torch.zeros_like(dists), dists)
    return collections.namedtuple('KNN', 'dists idx knn')(dists[..., None], idx[..., None], None)


def _knn_gather(x, idx, lengths=None):
    N, M, K = idx.shape
    return x[:, :, None].expand(-1, -1, K, -1).gather(1, idx[:, :, :, None].expand(-1, -1, -1, x.shape[2]))


def _validate(batch_reduction, point_reduction):
    assert batch_reduction in (None, 'mean', 'sum') and point_reduction in ('mean', 'sum')


def _handle(points, lengths, normals):
    if lengths is None:
        lengths = torch.full((points.shape[0],), points.shape[1], dtype=torch.int64)
    return points, lengths, normals


class _P3DMeshes:
    def __init__(self, verts, faces):
        self.v, self.f = verts, faces

    def get_mesh_verts_faces(self, i):
        return self.v[i], self.f[i]


class _TriangleMesh:
    def __init__(self, verts, faces):
        self.vertices, self.triangles = np.asarray(verts, np.float64), np.asarray(faces, np.int32)

    def remove_unreferenced_vertices(self):
        used = np.zeros(len(self.vertices), bool)
        used[self.triangles.reshape(-1)] = True
        new_id = np.cumsum(used) - 1
        self.vertices, self.triangles = self.vertices[used], new_id[self.triangles].astype(np.int32)


STL = {}


def install_fakes():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    mod('pytorch3d'); mod('pytorch3d.ops'); mod('pytorch3d.loss')
    mod('pytorch3d.ops.knn', knn_points=_knn_points, knn_gather=_knn_gather)
    mod('pytorch3d.loss.chamfer', _validate_chamfer_reduction_inputs=_validate, _handle_pointcloud_input=_handle)
    mod('pytorch3d.structures', Meshes=_P3DMeshes)
    pc = types.SimpleNamespace
    mod('open3d', geometry=pc(TriangleMesh=_TriangleMesh), utility=pc(Vector3dVector=lambda a: np.asarray(a, np.float64),
                                                                      Vector3iVector=lambda a: np.asarray(a, np.int32)),
        io=pc(read_point_cloud=lambda path: pc(points=STL['points'])))
    mod('trimesh')
    sys.path.insert(0, REF)


# ------------------------------------------------------------------------------------------------ chamfer.npz
def make_chamfer(chamfer_distance):
    g = torch.Generator().manual_seed(3)
    N, P1, P2 = 3, 37, 52
    x = torch.rand(N, P1, 3, generator=g)
    y = torch.rand(N, P2, 3, generator=g) * 1.2 - 0.1
    xn = torch.nn.functional.normalize(torch.randn(N, P1, 3, generator=g), dim=-1)
    yn = torch.nn.functional.normalize(torch.randn(N, P2, 3, generator=g), dim=-1)
    xl, yl = torch.tensor([37, 20, 31]), torch.tensor([52, 45, 9])
    w = torch.tensor([0.5, 2.0, 1.0])
    cases = [dict(return_L1=False),
             dict(return_L1=True, direction_reduction='none'),
             dict(return_L1=False, direction_reduction='mean', normals=True),
             dict(return_L1=False, lengths=True, normals=True, weights=True, direction_reduction='sum'),
             dict(return_L1=True, lengths=True, direction_reduction='none'),
             dict(return_L1=True, weights=True, batch_reduction=None, point_reduction='sum', direction_reduction='mean'),
             dict(return_L1=False, lengths=True, normals=True, batch_reduction='sum', direction_reduction='none')]
    out = dict(x=x.numpy(), y=y.numpy(), x_normals=xn.numpy(), y_normals=yn.numpy(), x_lengths=xl.numpy(), y_lengths=yl.numpy(),
               weights=w.numpy(), n_cases=len(cases))
    for k, c in enumerate(cases):
        xs, ys = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        xns, yns = xn.clone().requires_grad_(True), yn.clone().requires_grad_(True)
        kw = dict(return_L1=c['return_L1'], batch_reduction=c.get('batch_reduction', 'mean'), point_reduction=c.get('point_reduction', 'mean'),
                  direction_reduction=c.get('direction_reduction', 'sum'))
        if c.get('lengths'):
            kw.update(x_lengths=xl, y_lengths=yl)
        if c.get('normals'):
            kw.update(x_normals=xns, y_normals=yns)
        if c.get('weights'):
            kw.update(weights=w)
        dist, nrm = chamfer_distance(xs, ys, **kw)
        vals = list(dist) if isinstance(dist, tuple) else [dist]
        if nrm is not None:
            vals += list(nrm) if isinstance(nrm, tuple) else [nrm]
        total = sum(v.sum() for v in vals)
        for j, v in enumerate(vals):
            out[f'c{k}_out{j}'] = v.detach().numpy()
        try:          # the reference assigns into the output of sqrt in place (return_L1 with masks / weights): not differentiable there
            total.backward()
            out[f'c{k}_grad_x'], out[f'c{k}_grad_y'] = xs.grad.numpy(), ys.grad.numpy()
            if c.get('normals'):
                out[f'c{k}_grad_xn'], out[f'c{k}_grad_yn'] = xns.grad.numpy(), yns.grad.numpy()
            has_grad = True
        except RuntimeError:
            has_grad = False
        out[f'c{k}_kwargs'] = np.array(repr(dict(c)))
        out[f'c{k}_n_out'] = len(vals)
        out[f'c{k}_has_grad'] = has_grad
    np.savez_compressed(os.path.join(HERE, 'chamfer.npz'), **out)
    print('chamfer.npz:', len(cases), 'cases, grads in', sum(bool(out[f'c{k}_has_grad']) for k in range(len(cases))))


# ------------------------------------------------------------------------------------------------ dtu_tiny.npz
def _rot(rng):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    a, b, c, d = q
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


BOX_F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]])


def make_scene(rng):
    verts, faces = [], []
    # (centre, size): inside the grid (two of them where ObsMask is false), past the grid but inside BB + 2 PATCH (+x), before the grid
    # but inside BB - PATCH (-x), and cubes (n1 == n2: the anti-diagonal ties of the lattice)
    boxes = [((0, 0, 0), (4.1, 4.1, 4.1)), ((8, -6, 3), (3.3, 5.3, 2.7)), ((-12, 10, -4), (4.3, 4.3, 4.3)), ((14, 14, -10), (2.9, 6.1, 3.7)),
             ((-20, -18, 12), (3.1, 3.1, 3.1)), ((45, 0, 0), (3.3, 2.9, 4.7)), ((-42, 5, 2), (2.7, 4.1, 3.3))]
    for c, s in boxes:
        corners = np.array([[i, j, k] for i in (-.5, .5) for j in (-.5, .5) for k in (-.5, .5)]) * np.array(s)
        v = corners @ _rot(rng).T + np.array(c) + rng.uniform(-0.3, 0.3, 3)
        faces.append(BOX_F + len(np.concatenate(verts)) if verts else BOX_F.copy())
        verts.append(v)
    nv = sum(len(v) for v in verts)
    verts.append(np.array([[500., 500., 500.], [503.1, 500., 500.], [500., 502.7, 500.3]]))       # far away: out of BB +- PATCH
    faces.append(np.array([[nv, nv + 1, nv + 2]]))
    verts.append(np.array([[1., 2., 3.], [7., 7., 7.]]))                                            # unreferenced vertices
    faces.append(np.array([[0, 0, 1]]))                                                             # a face of zero area (dropped)
    V = np.concatenate(verts).astype(np.float32)
    F_ = np.concatenate(faces).astype(np.int64)
    # ground truth: points near the boxes' surfaces, a few far ones, some below the plane
    k = rng.integers(0, len(BOX_F) * 7, 6000)
    fv = V[F_[k]].astype(np.float64)
    u, w = rng.random(6000), rng.random(6000)
    su = np.sqrt(u)
    stl = (1 - su)[:, None] * fv[:, 0] + (su * (1 - w))[:, None] * fv[:, 1] + (su * w)[:, None] * fv[:, 2] + rng.normal(0, 0.3, (6000, 3))
    stl = np.concatenate([stl, rng.uniform(-30, 30, (300, 3)), rng.uniform(-30, 30, (200, 3)) * [1, 1, 0.1] + [0, 0, -28]])
    return V, F_, stl


def make_dtu(dtu_eval):
    rng = np.random.default_rng(11)
    V, F_, stl = make_scene(rng)
    BB = np.array([[-30., -30., -30.], [30., 30., 30.]])
    Res = np.array([[4.0]])
    shape = tuple((np.ceil((BB[1] - BB[0]) / Res[0, 0]) + 1).astype(int))
    obs = np.ones(shape, np.uint8)
    obs[9:, :7, :] = 0                                     # the box at (8, -6, 3) and (14, 14, -10) partly outside the observed volume
    obs[:, 10:, :6] = 0
    plane = np.array([[0.], [0.], [1.], [25.]])            # z > -25 is above
    STL['points'] = stl
    rec = {}
    real_rng = np.random.default_rng

    class RecRng:
        def __init__(self, *a, **k):
            self.rng = real_rng(2024)

        def shuffle(self, x, axis=0):
            rec['pcd'] = x.copy()
            perm = self.rng.permutation(x.shape[0])
            x[:] = x[perm]
            rec['perm'] = perm

    real_nn = skln.NearestNeighbors

    class RecNN(real_nn):
        def fit(self, X, y=None):
            rec.setdefault('fit', []).append(np.array(X))
            return super().fit(X)

        def radius_neighbors(self, X=None, radius=None, return_distance=True, sort_results=False):
            r = super().radius_neighbors(X, radius=radius, return_distance=return_distance, sort_results=sort_results)
            rec['rnn'] = r
            return r

        def kneighbors(self, X=None, n_neighbors=None, return_distance=True):
            r = super().kneighbors(X, n_neighbors=n_neighbors, return_distance=return_distance)
            rec.setdefault('kq', []).append((np.array(X), r[0][:, 0]))
            return r

    RecNN.__init__ = real_nn.__init__
    np.random.default_rng = RecRng
    dtu_eval.skln.NearestNeighbors = RecNN
    try:
        with tempfile.TemporaryDirectory() as d:
            os.makedirs(f'{d}/ObsMask')
            scipy.io.savemat(f'{d}/ObsMask/ObsMask24_10.mat', {'ObsMask': obs, 'BB': BB, 'Res': Res})
            scipy.io.savemat(f'{d}/ObsMask/Plane24.mat', {'P': plane})
            mesh = _P3DMeshes(torch.from_numpy(V)[None], torch.from_numpy(F_)[None])
            dtu_eval.evaluate_mesh(mesh, 24, d, d, save_viz=False)
            tsv = open(f'{d}/dtu_scores.tsv').read()
    finally:
        np.random.default_rng = real_rng
        dtu_eval.skln.NearestNeighbors = real_nn
    pcd, perm = rec['pcd'], rec['perm']
    shuffled = pcd[perm]
    # the keep mask of the reference's loop (dtu_eval.py:88-92), on the neighbour lists it computed
    mask = np.ones(len(shuffled), np.bool_)
    for curr, idxs in enumerate(rec['rnn']):
        if mask[curr]:
            mask[idxs] = 0
            mask[curr] = 1
    assert np.array_equal(rec['fit'][0], shuffled) and np.array_equal(rec['fit'][1], stl)
    data_in = rec['fit'][2]
    (q_d2s, dist_d2s), (q_s2d, dist_s2d) = rec['kq']
    # margins: no pair within 1e-6 relative of the radius, no NN distance within 1e-6 of MAX_DIST
    dists, _ = real_nn(radius=RADIUS * 1.00001).fit(shuffled).radius_neighbors(shuffled, radius=RADIUS * 1.00001, return_distance=True)
    near = min((np.abs(dd - RADIUS).min() for dd in dists if len(dd)), default=1.0)
    assert near > 1e-6 * RADIUS, f'a pair at {near} from the radius'
    assert np.abs(np.concatenate([dist_d2s, dist_s2d]) - MAX_DIST).min() > 1e-6 * MAX_DIST
    # per-triangle lattice counts from the cloud the reference built (the vertices first, then the faces in order)
    used = np.zeros(len(V), bool)
    used[F_.reshape(-1)] = True
    nvert = int(used.sum())
    counts = _lattice_counts(V.astype(np.float64)[F_])
    assert nvert + counts.sum() == len(pcd)
    acc, comp, avg = (float(s) for s in tsv.split('\n')[1].split('\t'))
    BBf = BB.astype(np.float32)
    data_down = shuffled[mask]
    inbound = ((data_down >= BBf[:1] - 60) & (data_down < BBf[1:] + 120)).sum(axis=-1) == 3
    assert np.array_equal(data_down[inbound], data_in)
    grid = np.around((data_in - BBf[:1]) / Res).astype(np.int32)
    gin = ((grid >= 0) & (grid < np.expand_dims(obs.shape, 0))).sum(axis=-1) == 3
    branches = dict(out_of_box=int((~inbound).sum()), out_of_grid=int((~gin).sum()),
                    obs_false=int((obs[grid[gin][:, 0], grid[gin][:, 1], grid[gin][:, 2]] == 0).sum()),
                    stl_below=int(len(stl) - len(q_s2d)))
    assert all(v > 0 for v in branches.values()), branches
    sub = np.random.default_rng(5).choice(len(pcd) - nvert, 400, replace=False) + nvert
    np.savez_compressed(os.path.join(HERE, 'dtu_tiny.npz'), verts=V, faces=F_, obs_mask=obs, bb=BB, res=Res, plane=plane, stl=stl,
                        perm=perm, counts=counts, n_vertices=nvert, n_points=len(pcd), lattice_idx=sub, lattice_points=pcd[sub],
                        keep=mask, n_down=int(mask.sum()), n_in_obs=len(q_d2s), n_stl_above=len(q_s2d),
                        n_d2s=int((dist_d2s < MAX_DIST).sum()), n_s2d=int((dist_s2d < MAX_DIST).sum()), acc=acc, comp=comp, avg=avg,
                        tsv=np.array(tsv), **{f'branch_{k}': v for k, v in branches.items()})
    print('dtu_tiny.npz: points', len(pcd), 'kept', int(mask.sum()), 'in obs', len(q_d2s), 'stl above', len(q_s2d), branches,
          'acc/comp/avg', acc, comp, avg)


def _lattice_counts(tri):
    """per-face lattice counts, the reference's own expressions (dtu_eval.py:56-70, 21-30) face by face"""
    out = np.zeros(len(tri), np.int64)
    for f, t in enumerate(tri):
        v1, v2 = t[1:2] - t[0:1], t[2:3] - t[0:1]
        l1, l2 = np.linalg.norm(v1, axis=-1, keepdims=True), np.linalg.norm(v2, axis=-1, keepdims=True)
        area2 = np.linalg.norm(np.cross(v1, v2), axis=-1, keepdims=True)
        if not (area2 > 0)[0, 0]:
            continue
        thr = 0.2 * np.sqrt(l1 * l2 / area2)
        n1, n2 = np.floor(l1 / thr)[0, 0], np.floor(l2 / thr)[0, 0]
        c = np.mgrid[:n1 + 1, :n2 + 1]
        c += 0.5
        c[0] /= max(n1, 1e-7)
        c[1] /= max(n2, 1e-7)
        out[f] = int((np.transpose(c, (1, 2, 0)).sum(axis=-1) < 1).sum())
    return out


if __name__ == '__main__':
    install_fakes()
    import importlib
    make_chamfer(importlib.import_module('utils.chamfer').chamfer_distance)
    make_dtu(importlib.import_module('utils.dtu_eval'))
