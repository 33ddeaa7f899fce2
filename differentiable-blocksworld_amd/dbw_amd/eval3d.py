"""3D evaluation of a reconstruction: Chamfer distance and the official DTU protocol, on the GPU (include/dbw_eval.h).

The reference computes these at the end of a DTU run through PyTorch3D's CUDA `knn_points` / `sample_points_from_meshes`
(utils/chamfer.py) and through open3d plus an sklearn KD-tree (utils/dtu_eval.py); neither has a ROCm build.  Here the hot path -- exact
nearest neighbours, the DTU dense lattice and its radius downsample -- is HIP (csrc/nn_search.hip) and torch / numpy do the plumbing.

    nn_points(x, y)                       exact 1-nearest neighbour (knn_points with K = 1)            -> (dist2, idx)
    chamfer_distance(x, y, ...)           utils/chamfer.py:7-160 (L1 / L2, direction reductions)      -> (cham_dist, cham_normals)
    sample_points_from_meshes(v, f, n)    PyTorch3D 0.7.1 ops/sample_points_from_meshes.py             -> (1, n, 3) points [, normals]
    chamfer_l1_scores(v, f, gt, scale)    the custom Chamfer-L1 of mbf_eval.py:54-60 / ems_eval.py:55-61 -> (acc, comp)
    dtu_scores(v, f, obs_mask, ...)       dtu_eval.py:47-160 on arrays                                 -> dict(acc, comp, avg, counts)
    evaluate_mesh(v, f, scan_id, ...)     dtu_eval.py:47-164 on a DTU directory, writes dtu_scores{suffix}.tsv
    evaluate_dtu(model, scale_mat, ...)   trainer.py:255-264: the live blocks of a model, scaled by scale_mat, evaluated
    gradient_icp(pc_pred, pc_gt, ...)     utils/icp.py:11-78, the whole loop in one call (include/dbw_icp.h) -> (upd_pc_pred, [R, T, s])
    gradient_icp_torch(...)               the same loop in torch, any device and dtype: the CPU path and the yardstick of the GPU tests
    normalize_mesh(verts, faces, ...)     utils/mesh.py:25-44 for one mesh                             -> (verts, faces)
    evaluate_aligned(model, points, ...)  the ICP-aligned scores (metrics.MeshEvaluator) of a model's live blocks, aligned_scores.tsv
    plane_ransac(points, ...)             robust plane fit: N points x H hypotheses in one call (dbw_eval_plane_fit) -> PlaneResult
    plane_ransac_torch(...)               the same fit in torch, any device; dtype=torch.float64: the oracle of the tests
    filter_ground(points, ...)            utils/ransac.py as dtu_3d_process.py:36-41 uses it           -> (points off the ground, (p0, p1, p2))
    cluster_points(points, k, ...)        k-means with a PCA of every cluster in one call (dbw_eval_cluster_fit)  -> ClusterResult
    cluster_points_torch(...)             the same fit in torch, any device: the CPU path and the readable restatement
"""
import collections
import ctypes
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib

MAX_DIST = 20                  # dtu_eval.py:16-18
PATCH = 60
DOWNSAMPLE_DENSITY = 0.2
CHAMFER_FACTOR = 10            # mbf_eval.py / ems_eval.py: the custom Chamfer-L1 is reported x10


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _call(name, *args):
    _lib.family('eval')
    _lib.call(name, *args)


# ------------------------------------------------------------------------------------------------ nearest neighbours
def _lengths(lengths, N, P, dev):
    if lengths is None:
        return torch.full((N,), P, dtype=torch.int64, device=dev)
    return torch.as_tensor(lengths, device=dev).to(torch.int64).clamp(0, P).contiguous()


def nn_points_torch(x, y, x_lengths=None, y_lengths=None, chunk_elems=1 << 22):
    """nn_points by chunked brute force in torch, on any device: same distance expression ((dx*dx + dy*dy) + dz*dz, one rounding per
    elementwise op), same tie rule (lowest index).  The CPU path of nn_points and the yardstick of the GPU tests."""
    N, P1, _ = x.shape
    P2 = y.shape[1]
    xl = _lengths(x_lengths, N, P1, 'cpu').tolist()
    yl = _lengths(y_lengths, N, P2, 'cpu').tolist()
    dist2 = torch.zeros(N, P1, dtype=torch.float32, device=x.device)
    idx = torch.full((N, P1), -1, dtype=torch.int64, device=x.device)
    for n in range(N):
        lx, ly = xl[n], yl[n]
        if ly == 0:
            dist2[n, :lx] = math.inf
            continue
        yn = y[n, :ly].float()
        ar = torch.arange(ly, device=x.device)
        step = max(1, chunk_elems // ly)
        for a in range(0, lx, step):
            b = min(lx, a + step)
            d = x[n, a:b, None, :].float() - yn[None]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            m = d2.min(1).values
            dist2[n, a:b] = m
            idx[n, a:b] = torch.where(d2 == m[:, None], ar, ly).min(1).values
    return dist2, idx


def nn_points(x, y, x_lengths=None, y_lengths=None, splits=0):
    """Exact 1-nearest neighbour of every x[n, i] among y[n, :y_lengths[n]] -> (dist2 (N,P1) fp32, idx (N,P1) int64).

    dist2 = ((dx*dx + dy*dy) + dz*dz), d = x - y in fp32; ties go to the lowest index; a query at or past x_lengths gets (0, -1), a batch
    with y_lengths == 0 gets (+inf, -1).  Device tensors use the HIP kernel (dbw_nn_points; `splits` forces the number of y ranges merged
    by the 64-bit atomic min, 0 = from the sizes: the result does not depend on it), CPU tensors the chunked torch brute force.  No
    gradient (chamfer_distance recomputes the distances of the chosen pairs in torch)."""
    if x.dim() != 3 or y.dim() != 3 or x.shape[2] != 3 or y.shape[2] != 3 or x.shape[0] != y.shape[0]:
        raise ValueError(f'nn_points: x (N,P1,3) and y (N,P2,3) expected, got {tuple(x.shape)} and {tuple(y.shape)}')
    if x.device.type == 'cpu' and y.device.type == 'cpu':
        return nn_points_torch(x.detach(), y.detach(), x_lengths, y_lengths)
    if x.device != y.device or x.device.type != 'cuda':
        raise ValueError('nn_points: x and y must be on the same device')
    N, P1, _ = x.shape
    P2 = y.shape[1]
    dev = x.device
    xs = x.detach().to(torch.float32).contiguous()
    ys = y.detach().to(torch.float32).contiguous()
    dist2 = torch.empty(N, P1, dtype=torch.float32, device=dev)
    idx = torch.empty(N, P1, dtype=torch.int64, device=dev)
    if P1 == 0:
        return dist2, idx
    if P2 == 0:
        return dist2.fill_(math.inf), idx.fill_(-1)
    xl = None if x_lengths is None else _lengths(x_lengths, N, P1, dev)
    yl = None if y_lengths is None else _lengths(y_lengths, N, P2, dev)
    keys = torch.empty(N * P1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _call('dbw_nn_points', _p(xs), _p(ys), _p(xl), _p(yl), N, P1, P2, int(splits), _p(keys), _p(dist2), _p(idx), _stream(dev))
    return dist2, idx


# ------------------------------------------------------------------------------------------------ Chamfer distance
def _validate_chamfer_reduction_inputs(batch_reduction, point_reduction):      # pytorch3d/loss/chamfer.py
    if batch_reduction is not None and batch_reduction not in ['mean', 'sum']:
        raise ValueError('batch_reduction must be one of ["mean", "sum"] or None')
    if point_reduction not in ['mean', 'sum']:
        raise ValueError('point_reduction must be one of ["mean", "sum"]')


def _handle_pointcloud_input(points, lengths, normals):                          # pytorch3d/loss/chamfer.py (tensors only)
    if points.ndim != 3:
        raise ValueError('Expected points to be of shape (N, P, D)')
    X = points
    if lengths is not None and (lengths.ndim != 1 or lengths.shape[0] != X.shape[0]):
        raise ValueError('Expected lengths to be of shape (N,)')
    if lengths is None:
        lengths = torch.full((X.shape[0],), X.shape[1], dtype=torch.int64, device=points.device)
    if normals is not None and normals.ndim != 3:
        raise ValueError('Expected normals to be of shape (N, P, 3')
    return X, lengths, normals


def _nn_dist2(x, y, idx, mask):
    """differentiable squared distance of x to its neighbour y[idx] (the kernel's expression); masked queries see distance 1"""
    g = y.gather(1, idx.clamp(min=0)[..., None].expand(-1, -1, 3))
    d = x - g
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return d2 if mask is None else torch.where(mask, torch.ones_like(d2), d2)


def chamfer_distance(x, y, x_lengths=None, y_lengths=None, x_normals=None, y_normals=None, weights=None, batch_reduction='mean',
                     point_reduction='mean', direction_reduction='sum', return_L1=False):
    """utils/chamfer.py:7-160 (PyTorch3D's chamfer_distance with the Chamfer-L1 and the direction reductions of the reference):
    same arguments, defaults and return values -> (cham_dist, cham_normals); direction_reduction 'none' / None returns the pairs
    (cham_x, cham_y) and (cham_norm_x, cham_norm_y).

    The neighbours come from nn_points (the HIP kernel for device tensors); the distances of the chosen pairs are recomputed in torch from
    x and y[idx], so autograd gives what PyTorch3D's knn backward gives, in x, y and the normals.  Masking, weighting and the return_L1
    square root are written out of place (the reference's in-place `cham_x[x_mask] = 0.0` after the square root cannot be
    differentiated); the values are the same, and the square root keeps torch's behaviour at a zero distance."""
    _validate_chamfer_reduction_inputs(batch_reduction, point_reduction)
    x, x_lengths, x_normals = _handle_pointcloud_input(x, x_lengths, x_normals)
    y, y_lengths, y_normals = _handle_pointcloud_input(y, y_lengths, y_normals)
    return_normals = x_normals is not None and y_normals is not None
    N, P1, D = x.shape
    P2 = y.shape[1]
    if y.shape[0] != N or y.shape[2] != D:
        raise ValueError('y does not have the correct shape.')
    is_x_heterogeneous = bool((x_lengths != P1).any())
    is_y_heterogeneous = bool((y_lengths != P2).any())
    x_mask = torch.arange(P1, device=x.device)[None] >= x_lengths[:, None]
    y_mask = torch.arange(P2, device=y.device)[None] >= y_lengths[:, None]
    if weights is not None:
        if weights.size(0) != N:
            raise ValueError('weights must be of shape (N,).')
        if not (weights >= 0).all():
            raise ValueError('weights cannot be negative.')
        if weights.sum() == 0.0:
            weights = weights.view(N, 1)
            if batch_reduction in ['mean', 'sum']:
                return (x.sum((1, 2)) * weights).sum() * 0.0, (x.sum((1, 2)) * weights).sum() * 0.0
            return (x.sum((1, 2)) * weights) * 0.0, (x.sum((1, 2)) * weights) * 0.0

    cham_norm_x = x.new_zeros(())
    cham_norm_y = x.new_zeros(())
    _, x_idx = nn_points(x, y, x_lengths, y_lengths)
    _, y_idx = nn_points(y, x, y_lengths, x_lengths)
    xm = x_mask if is_x_heterogeneous else None
    ym = y_mask if is_y_heterogeneous else None
    cham_x = _nn_dist2(x, y, x_idx, xm)
    cham_y = _nn_dist2(y, x, y_idx, ym)
    if return_L1:
        cham_x, cham_y = cham_x.sqrt(), cham_y.sqrt()
    if is_x_heterogeneous:
        cham_x = torch.where(x_mask, torch.zeros_like(cham_x), cham_x)
    if is_y_heterogeneous:
        cham_y = torch.where(y_mask, torch.zeros_like(cham_y), cham_y)
    if weights is not None:
        cham_x = cham_x * weights.view(N, 1)
        cham_y = cham_y * weights.view(N, 1)

    if return_normals:
        x_normals_near = y_normals.gather(1, x_idx.clamp(min=0)[..., None].expand(-1, -1, y_normals.shape[2]))
        y_normals_near = x_normals.gather(1, y_idx.clamp(min=0)[..., None].expand(-1, -1, x_normals.shape[2]))
        cham_norm_x = 1 - torch.abs(F.cosine_similarity(x_normals, x_normals_near, dim=2, eps=1e-6))
        cham_norm_y = 1 - torch.abs(F.cosine_similarity(y_normals, y_normals_near, dim=2, eps=1e-6))
        if is_x_heterogeneous:
            cham_norm_x = torch.where(x_mask, torch.zeros_like(cham_norm_x), cham_norm_x)
        if is_y_heterogeneous:
            cham_norm_y = torch.where(y_mask, torch.zeros_like(cham_norm_y), cham_norm_y)
        if weights is not None:
            cham_norm_x = cham_norm_x * weights.view(N, 1)
            cham_norm_y = cham_norm_y * weights.view(N, 1)

    cham_x = cham_x.sum(1)
    cham_y = cham_y.sum(1)
    if return_normals:
        cham_norm_x = cham_norm_x.sum(1)
        cham_norm_y = cham_norm_y.sum(1)
    if point_reduction == 'mean':
        cham_x = cham_x / x_lengths
        cham_y = cham_y / y_lengths
        if return_normals:
            cham_norm_x = cham_norm_x / x_lengths
            cham_norm_y = cham_norm_y / y_lengths
    if batch_reduction is not None:
        cham_x = cham_x.sum()
        cham_y = cham_y.sum()
        if return_normals:
            cham_norm_x = cham_norm_x.sum()
            cham_norm_y = cham_norm_y.sum()
        if batch_reduction == 'mean':
            div = weights.sum() if weights is not None else N
            cham_x = cham_x / div
            cham_y = cham_y / div
            if return_normals:
                cham_norm_x = cham_norm_x / div
                cham_norm_y = cham_norm_y / div

    if direction_reduction is None or direction_reduction == 'none':
        cham_dist = (cham_x, cham_y)
        cham_normals = (cham_norm_x, cham_norm_y) if return_normals else None
    else:
        cham_dist = cham_x + cham_y
        cham_normals = cham_norm_x + cham_norm_y if return_normals else None
        if direction_reduction == 'mean':
            cham_dist, cham_normals = 0.5 * cham_dist, 0.5 * cham_normals if return_normals else None
    return cham_dist, cham_normals


# ------------------------------------------------------------------------------------------------ mesh sampling
def sample_points_from_meshes(verts, faces, num_samples, return_normals=False, generator=None, return_face_idx=False):
    """PyTorch3D 0.7.1 `sample_points_from_meshes` for ONE mesh (verts (V,3), faces (F,3)) -> points (1, num_samples, 3)
    [, normals (1, num_samples, 3)] [, face index (num_samples,)].

    Restated from memory of PyTorch3D 0.7.1 (the package is not available here), like SURVEY.md Appendix A: faces are drawn with
    replacement by `multinomial` over the face areas 0.5 * |(v1 - v0) x (v2 - v0)|, then `torch.rand(2, 1, num_samples)` gives u, v and
    w = (1 - sqrt(u), sqrt(u) * (1 - v), sqrt(u) * v); point = (w0 * v0 + w1 * v1) + w2 * v2 of the sampled face.  Normals are the
    normalised (v1 - v0) x (v2 - v1) of the sampled face (norm clamped at the fp64 epsilon).  Differentiable in verts."""
    faces = faces.to(device=verts.device, dtype=torch.int64)
    fv = verts[faces]
    v0, v1, v2 = fv[:, 0], fv[:, 1], fv[:, 2]
    with torch.no_grad():
        areas = 0.5 * torch.linalg.cross(v1 - v0, v2 - v0, dim=1).norm(dim=1)
        fidx = areas[None].multinomial(num_samples, replacement=True, generator=generator)[0]
    uv = torch.rand(2, 1, num_samples, dtype=verts.dtype, device=verts.device, generator=generator)
    u_sqrt = uv[0].sqrt()
    w0, w1, w2 = 1.0 - u_sqrt, u_sqrt * (1.0 - uv[1]), u_sqrt * uv[1]
    pts = w0[:, :, None] * v0[fidx][None] + w1[:, :, None] * v1[fidx][None] + w2[:, :, None] * v2[fidx][None]
    out = [pts]
    if return_normals:
        n = torch.linalg.cross(v1 - v0, v2 - v1, dim=1)
        n = n / n.norm(dim=1, p=2, keepdim=True).clamp(min=np.finfo(np.float64).eps)
        out.append(n[fidx][None])
    if return_face_idx:
        out.append(fidx)
    return out[0] if len(out) == 1 else tuple(out)


def chamfer_l1_scores(verts, faces, gt_points, scale_mat, n_points=500_000, generator=None):
    """The custom Chamfer-L1 of the reference's baseline scripts (mbf_eval.py:54-60, ems_eval.py:55-61): n_points samples of the mesh
    (sample_points_from_meshes), brought into the normalised frame with the inverse of the VolSDF `scale_mat` (points @ inv[:3,:3] +
    inv[:3,3]), Chamfer-L1 against gt_points (P,3) with direction_reduction='none', times 10 -> (acc, comp) floats."""
    dev = verts.device
    pts = sample_points_from_meshes(verts, faces, n_points, generator=generator)
    scale_inv = torch.as_tensor(scale_mat).to(dev).inverse()
    pts = pts @ scale_inv[:3, :3] + scale_inv[:3, 3]
    gt = torch.as_tensor(gt_points).to(device=dev, dtype=pts.dtype)[None]
    acc, comp = chamfer_distance(pts, gt, return_L1=True, direction_reduction='none')[0]
    return CHAMFER_FACTOR * acc.item(), CHAMFER_FACTOR * comp.item()


# ------------------------------------------------------------------------------------------------ DTU protocol
def _device(dev):
    dev = torch.device('cuda' if dev is None else dev)
    if dev.type != 'cuda':
        raise ValueError('the DTU evaluation runs its lattice, downsample and search kernels on the GPU: pass a cuda device')
    return dev


def compact_mesh(verts, faces):
    """open3d's remove_unreferenced_vertices: the referenced vertices in their order, faces renumbered"""
    used = torch.zeros(verts.shape[0], dtype=torch.bool, device=verts.device)
    used[faces.reshape(-1)] = True
    new_id = torch.cumsum(used.to(torch.int64), 0) - 1
    return verts[used], new_id[faces]


def dense_lattice(verts, faces):
    """The dense point cloud of dtu_eval.py:56-78 (HIP kernels, fp64): the vertices (all referenced ones, in order) followed by the lattice
    of every face of non-zero area in face order, each in np.mgrid row-major order -> (points (n,3) fp64, per-face counts (F,) int64).
    verts (V,3) fp32 or fp64 and faces (F,3) on a cuda device; unreferenced vertices are dropped first."""
    dev = verts.device
    v64, faces = compact_mesh(verts.to(torch.float64), faces.to(device=dev, dtype=torch.int64))
    F_ = faces.shape[0]
    counts = torch.zeros(F_, dtype=torch.int64, device=dev)
    if F_ == 0:
        return v64.contiguous(), counts
    tri = v64[faces].contiguous()                                            # (F,3,3)
    with torch.cuda.device(dev):
        _call('dbw_dtu_lattice_counts', _p(tri), F_, _p(counts), _stream(dev))
        offsets = torch.cumsum(counts, 0) - counts
        total = int(counts.sum())
        pts = torch.empty(v64.shape[0] + total, 3, dtype=torch.float64, device=dev)
        pts[:v64.shape[0]] = v64
        if total:
            _call('dbw_dtu_lattice_points', _p(tri), F_, _p(counts), _p(offsets), total, _p(pts[v64.shape[0]:]), _stream(dev))
    return pts, counts


def radius_downsample(points, radius=DOWNSAMPLE_DENSITY):
    """The greedy downsample of dtu_eval.py:82-96 in the given order: point i is kept iff no earlier KEPT point lies within `radius`
    (distance <= radius, fp64).  Computed exactly as a parallel maximal independent set over a uniform grid (cell size >= radius, torch
    sorts the points by cell): each round (dbw_radius_downsample_round) keeps the undecided points without an earlier undecided or kept
    neighbour and removes those with an earlier kept one.  O(log n) rounds for a random order (Blelloch, Fineman and Shun, SPAA 2012).
    points (n,3) fp64 on a cuda device -> (keep mask (n,) bool, number of rounds)."""
    dev = points.device
    n = points.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.bool, device=dev), 0
    p = points.to(torch.float64)
    lo = p.min(0).values
    cell = torch.floor((p - lo) / (radius * (1 + 1e-6))).to(torch.int64) + 1      # a border of empty cells: no neighbour key aliases
    dims = (cell.max(0).values + 2).tolist()
    if dims[0] * dims[1] * dims[2] >= 1 << 62:
        raise ValueError('radius_downsample: the grid is too large for 64-bit cell keys')
    keys = (cell[:, 0] * dims[1] + cell[:, 1]) * dims[2] + cell[:, 2]
    keys_s, rank = torch.sort(keys, stable=True)                # within a cell: the processing order
    pts_s = p[rank].contiguous()
    st = [torch.zeros(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)]
    rounds, open_ = 0, n
    with torch.cuda.device(dev):
        while open_:
            _call('dbw_radius_downsample_round', _p(pts_s), _p(keys_s), _p(rank), n, dims[1], dims[2], float(radius), _p(st[0]), _p(st[1]),
                  _stream(dev))
            st.reverse()
            rounds += 1
            left = int((st[0] == 0).sum())
            if left >= open_:                                   # (the earliest undecided point is always decided: cannot happen)
                raise RuntimeError('radius_downsample: a round decided nothing')
            open_ = left
    keep = torch.empty(n, dtype=torch.bool, device=dev)
    keep[rank] = st[0] == 1
    return keep, rounds


def _nn_fp64(q, ref, center):
    """nearest neighbour of every q among ref: searched in fp32 on coordinates centred on `center`, the chosen pair's distance recomputed in
    fp64 -> distances (len(q),) float64 numpy"""
    if len(q) == 0:
        return np.zeros(0)
    if len(ref) == 0:
        return np.full(len(q), np.inf)
    dev = q.device
    c = torch.as_tensor(center, dtype=torch.float64, device=dev)
    _, idx = nn_points((q - c).float()[None], (ref - c).float()[None])
    d = q - ref[idx[0]]
    return torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).cpu().numpy()


def dtu_scores(verts, faces, obs_mask, bb, res, plane, stl, order=None, seed=None, device=None):
    """The official DTU protocol (dtu_eval.py:47-160) on arrays -> dict(acc, comp, avg, n_vertices, n_lattice, n_points, n_down,
    n_in_obs, n_stl_above, n_d2s, n_s2d, rounds).

    verts (V,3) / faces (F,3) in the DTU frame (mm), obs_mask / bb / res: the ObsMask, BB, Res of ObsMask{id}_10.mat, plane: P of
    Plane{id}.mat, stl (M,3): the ground-truth points.  The dense cloud (dense_lattice) is shuffled with `order` (a permutation of its
    n_points rows: shuffled[k] = cloud[order[k]]) or, when order is None, with np.random.default_rng(seed).permutation.  The reference
    shuffles with an UNSEEDED default_rng(), so its scores are not reproducible from run to run; a fixed seed here is.  Then the greedy
    radius downsample (radius_downsample), the masks of the reference with its exact semantics (BB - PATCH <= p < BB + 2 PATCH, np.around
    half to even, ObsMask lookup, plane test), and the two searches: data in ObsMask -> stl (acc) and stl above the plane -> data inside
    the box (comp, fitted on data_in, not on the ObsMask-filtered set).  Means over the distances < MAX_DIST (20 mm), in fp64.
    n_d2s / n_s2d count the distances below MAX_DIST."""
    dev = _device(device)
    v = torch.as_tensor(verts).to(dev)
    if v.dtype != torch.float64:
        v = v.to(torch.float32)
    f = torch.as_tensor(faces).to(device=dev, dtype=torch.int64)
    pcd, counts = dense_lattice(v, f)
    n = pcd.shape[0]
    if order is None:
        order = np.random.default_rng(seed).permutation(n)
    order = torch.as_tensor(np.asarray(order), dtype=torch.int64, device=dev)
    if order.shape != (n,):
        raise ValueError(f'dtu_scores: order must be a permutation of the {n} points of the dense cloud')
    pcd = pcd[order].contiguous()
    keep, rounds = radius_downsample(pcd, DOWNSAMPLE_DENSITY)
    data_down = pcd[keep].cpu().numpy()

    BB = np.asarray(bb).astype(np.float32)
    res = np.asarray(res)
    obs_mask = np.asarray(obs_mask)
    inbound = ((data_down >= BB[:1] - PATCH) & (data_down < BB[1:] + PATCH * 2)).sum(axis=-1) == 3
    data_in = data_down[inbound]
    data_grid = np.around((data_in - BB[:1]) / res).astype(np.int32)
    grid_inbound = ((data_grid >= 0) & (data_grid < np.expand_dims(obs_mask.shape, 0))).sum(axis=-1) == 3
    data_grid_in = data_grid[grid_inbound]
    in_obs = obs_mask[data_grid_in[:, 0], data_grid_in[:, 1], data_grid_in[:, 2]].astype(np.bool_)
    data_in_obs = data_in[grid_inbound][in_obs]

    stl = np.asarray(stl, dtype=np.float64)
    stl_hom = np.concatenate([stl, np.ones_like(stl[:, :1])], -1)
    above = (np.asarray(plane).reshape((1, 4)) * stl_hom).sum(-1) > 0
    stl_above = stl[above]

    center = (BB[0].astype(np.float64) + BB[1].astype(np.float64)) / 2
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)         # noqa: E731
    d_in = t(data_in)
    dist_d2s = _nn_fp64(t(data_in_obs), t(stl), center)
    dist_s2d = _nn_fp64(t(stl_above), d_in, center)
    d2s, s2d = dist_d2s[dist_d2s < MAX_DIST], dist_s2d[dist_s2d < MAX_DIST]
    mean_d2s = float(d2s.mean()) if len(d2s) else float('nan')
    mean_s2d = float(s2d.mean()) if len(s2d) else float('nan')
    return dict(acc=mean_d2s, comp=mean_s2d, avg=(mean_d2s + mean_s2d) / 2, n_vertices=n - int(counts.sum()), n_lattice=int(counts.sum()),
                n_points=n, n_down=int(len(data_down)), n_in_obs=int(len(data_in_obs)), n_stl_above=int(len(stl_above)), n_d2s=int(len(d2s)),
                n_s2d=int(len(s2d)), rounds=rounds)


# ------------------------------------------------------------------------------------------------ files
_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


def read_ply_points(path):
    """x, y, z of the `vertex` element of a PLY file (ascii or binary_little_endian) -> (n,3) float64.  Elements before `vertex` must have
    fixed-size properties; what follows it is not read."""
    with open(path, 'rb') as fh:
        if fh.readline().strip() != b'ply':
            raise ValueError(f'{path}: not a PLY file')
        fmt, elements = None, []
        while True:
            line = fh.readline()
            if not line:
                raise ValueError(f'{path}: no end_header')
            tok = line.decode('ascii', 'replace').split()
            if not tok or tok[0] in ('comment', 'obj_info'):
                continue
            if tok[0] == 'end_header':
                break
            if tok[0] == 'format':
                fmt = tok[1]
            elif tok[0] == 'element':
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == 'property':
                if tok[1] == 'list':
                    elements[-1][2].append((tok[4], None))
                else:
                    elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
        if fmt not in ('ascii', 'binary_little_endian'):
            raise ValueError(f'{path}: PLY format {fmt} is not supported (ascii, binary_little_endian)')
        for name, count, props in elements:
            if name == 'vertex':
                if any(t is None for _, t in props):
                    raise ValueError(f'{path}: list property in the vertex element')
                names = [p for p, _ in props]
                if fmt == 'ascii':
                    rows = [fh.readline().split() for _ in range(count)]
                    arr = np.array(rows, dtype=np.float64).reshape(count, len(props))
                    return np.stack([arr[:, names.index(c)] for c in 'xyz'], 1)
                dt = np.dtype([(p, '<' + t) for p, t in props])
                arr = np.frombuffer(fh.read(dt.itemsize * count), dtype=dt, count=count)
                return np.stack([arr[c].astype(np.float64) for c in 'xyz'], 1)
            if any(t is None for _, t in props):
                raise ValueError(f'{path}: variable-size element {name} before the vertices')
            if fmt == 'ascii':
                for _ in range(count):
                    fh.readline()
            else:
                fh.read(np.dtype([(p, '<' + t) for p, t in props]).itemsize * count)
    raise ValueError(f'{path}: no vertex element')


def write_scores_tsv(path, acc, comp, avg):
    """dtu_scores{suffix}.tsv exactly as dtu_eval.py:162-164 writes it (no newline after the values)"""
    with open(path, 'w') as f:
        f.write('acc\tcomp\tavg\n')
        f.write(f'{float(acc)}\t{float(comp)}\t{float(avg)}')


def load_dtu_scan(scan_id, dataset_dir):
    """(obs_mask, bb, res, plane, stl) of a DTU scan: ObsMask/ObsMask{id}_10.mat, ObsMask/Plane{id}.mat, Points/stl/stl{id:03}_total.ply"""
    from scipy.io import loadmat
    m = loadmat(f'{dataset_dir}/ObsMask/ObsMask{scan_id}_10.mat')
    plane = loadmat(f'{dataset_dir}/ObsMask/Plane{scan_id}.mat')['P']
    stl = read_ply_points(f'{dataset_dir}/Points/stl/stl{scan_id:03}_total.ply')
    return m['ObsMask'], m['BB'], m['Res'], plane, stl


def evaluate_mesh(verts, faces, scan_id, dataset_dir, eval_dir, suffix='', seed=None, order=None, device=None):
    """dtu_eval.py:47-164 on a mesh (verts (V,3) in the DTU frame, faces (F,3)) and a DTU directory laid out like the reference's: the
    scores of dtu_scores, written to {eval_dir}/dtu_scores{suffix}.tsv in the reference's format -> the dtu_scores dict.  The
    reference's `save_viz` point clouds are not produced."""
    obs_mask, bb, res, plane, stl = load_dtu_scan(scan_id, dataset_dir)
    dev = device if device is not None else (verts.device if torch.is_tensor(verts) and verts.is_cuda else None)
    s = dtu_scores(verts, faces, obs_mask, bb, res, plane, stl, order=order, seed=seed, device=dev)
    os.makedirs(eval_dir, exist_ok=True)
    write_scores_tsv(os.path.join(str(eval_dir), f'dtu_scores{suffix}.tsv'), s['acc'], s['comp'], s['avg'])
    return s


def evaluate_dtu(model, scale_mat, scan_id, dataset_dir, eval_dir, suffix='', seed=None):
    """trainer.py:255-264: the blocks of a trained model (filter_transparent=True, world coordinates: model.blocks_mesh) brought to the DTU
    frame with `verts @ scale_mat[:3, :3] + scale_mat[:3, 3]` (the scale_mat of cameras.load_idr_cameras) and evaluated with
    evaluate_mesh -> the dtu_scores dict (dtu_scores{suffix}.tsv in eval_dir)."""
    verts, faces = model.blocks_mesh(filter_transparent=True)
    scale = torch.as_tensor(scale_mat).to(device=verts.device, dtype=verts.dtype)
    verts = verts @ scale[:3, :3] + scale[:3, 3]
    return evaluate_mesh(verts, faces, scan_id, dataset_dir, eval_dir, suffix=suffix, seed=seed, device=verts.device)


# ------------------------------------------------------------------------------------------------ ICP-aligned evaluation
def normalize_mesh(verts, faces, center=True, scale_mode='unit_cube', use_center_mass=False):
    """utils/mesh.py:25-44 for one mesh (verts (V,3), faces (F,3)) -> (verts, faces): centred on the middle of its bounding box, then scaled
    to fit [-0.5, 0.5]^3 ('unit_cube'), the sphere of diameter 1 ('unit_sphere') or not at all ('none' / None).  `use_center_mass` (the mean
    of 100 000 random surface samples in the reference) is refused: it makes the frame depend on the random draw."""
    if use_center_mass:
        raise NotImplementedError('normalize_mesh: use_center_mass draws random samples to centre the mesh; only the bounding-box centre is built')
    if center:
        verts = verts - 0.5 * (verts.max(0).values + verts.min(0).values)
    if scale_mode == 'none' or scale_mode is None:
        return verts, faces
    if scale_mode == 'unit_cube':
        scale = verts.abs().max() * 2
    elif scale_mode == 'unit_sphere':
        scale = verts.norm(dim=1).max() * 2
    else:
        raise NotImplementedError(f'normalize_mesh: scale_mode {scale_mode!r}')
    return verts * (1 / scale), faces


def keep_best_history(losses, N=1):
    """The keep-best rule of icp.py:27-28,65-74 on a loss history (csrc/icp_math.h states it for the device) -> (best_loss, best_iter,
    checks): checks = [(iteration, meter average, kept)] for every iteration with it % 10 == 0; best_iter -1 and best_loss 1e6 if no check
    ever beat 1e6."""
    loss_min, best, acc, cnt, checks = 1e6, -1, 0.0, 0, []
    for it, loss in enumerate(losses):
        acc += float(loss) * N
        cnt += N
        if it % 10 == 0:
            avg = acc / cnt
            if avg < loss_min:
                loss_min, best = avg, it
            checks.append((it, avg, best == it))
            acc, cnt = 0.0, 0
    return loss_min, best, checks


def _print_checks(trace, N):
    for _, avg, kept in keep_best_history(trace['loss'].tolist(), N)[2]:      # what icp.py prints with verbose=True
        print(avg, 'save checkpoint') if kept else print(avg)


def gradient_icp_torch(pc_pred, pc_gt, estimate_scale=True, anisotropic_scale=False, lr=0.01, n_iter=300, verbose=False,
                       return_trace=False):
    """The per-instance loop of utils/icp.py:59-78 in torch, on any device and in the dtype of pc_pred: chamfer_distance (its searches run
    on the HIP kernel for device tensors), mesh.rotation_6d_to_matrix, torch.optim.Adam, a host read of the loss per iteration.
    -> (upd_pc_pred, [Rf (N,3,3), Tf (N,3), sf (N,3) or (N,1)]) [, trace].  The kept parameters are COPIES taken at the check (the
    reference keeps `T.detach()` / `s.detach()`, views that Adam goes on updating in place, so it returns the kept R with the LAST T and s
    whenever n_iter - 1 is not a kept check; that is not restated)."""
    from .mesh import rotation_6d_to_matrix
    if pc_pred.dim() != 3 or pc_gt.dim() != 3 or len(pc_pred) != len(pc_gt):
        raise ValueError('expected points to be of shape (N, P, D), with the same N')
    dev, dt, N = pc_pred.device, pc_pred.dtype, len(pc_pred)
    pc_pred, pc_gt = pc_pred.detach(), pc_gt.detach().to(dt)
    with torch.enable_grad():
        R6 = torch.nn.Parameter(torch.tensor([[1., 0., 0., 0., 1., 0.]], dtype=dt, device=dev).repeat(N, 1))
        T = torch.nn.Parameter(torch.zeros(N, 3, dtype=dt, device=dev))
        if estimate_scale:
            s = torch.nn.Parameter(torch.ones(N, 3 if anisotropic_scale else 1, dtype=dt, device=dev))
            params = [R6, T, s]
        else:
            s = torch.ones(N, 3, dtype=dt, device=dev)
            params = [R6, T]
        snap = lambda: [rotation_6d_to_matrix(R6).detach().clone(), T.detach().clone(), s.detach().clone()]      # noqa: E731
        argmin, losses, hist = snap(), [], []
        loss_min, best, acc, cnt = 1e6, -1, 0.0, 0
        opt = torch.optim.Adam(params, lr=lr)
        for it in range(n_iter):
            opt.zero_grad()
            loss = chamfer_distance(s[:, None] * pc_pred @ rotation_6d_to_matrix(R6) + T[:, None], pc_gt)[0]
            loss.backward()
            opt.step()
            losses.append(loss.item())
            acc += losses[-1] * N
            cnt += N
            if return_trace:
                hist.append(snap())
            if it % 10 == 0:
                if acc / cnt < loss_min:
                    loss_min, best, argmin = acc / cnt, it, snap()
                acc, cnt = 0.0, 0
    Rf, Tf, sf = argmin
    upd = sf[:, None] * pc_pred @ Rf + Tf[:, None]
    trace = dict(loss=torch.tensor(losses, dtype=torch.float64), best_loss=loss_min, best_iter=best)
    if return_trace:
        for k, name in enumerate('RTs'):
            trace[name] = torch.stack([h[k] for h in hist]) if hist else torch.zeros((0,) + argmin[k].shape, dtype=dt, device=dev)
    if verbose:
        _print_checks(trace, N)
    return (upd, [Rf, Tf, sf], trace) if return_trace else (upd, [Rf, Tf, sf])


def _icp_call(name, *args):
    lib = _lib.family('icp')
    if name == 'dbw_icp_workspace_bytes':
        return lib.dbw_icp_workspace_bytes(*args)
    _lib.call(name, *args)


def icp_run(pc_pred, pc_gt, estimate_scale=True, anisotropic_scale=False, lr=0.01, n_iter=300, splits=0, with_trace=False):
    """dbw_icp_run on device tensors pc_pred (N,P1,3), pc_gt (N,P2,3): the whole alignment enqueued by one call, nothing read by the host
    -> dict(cloud (N,P1,3), R (N,3,3), T (N,3), s (N,3), best (2,) fp64 = [kept loss average, kept iteration], trace (n_iter, 1 + 15 N)
    fp64 or None), all on the device, fp32 unless said.  `splits`: as in nn_points; the result does not depend on it."""
    if pc_pred.dim() != 3 or pc_gt.dim() != 3 or pc_pred.shape[2] != 3 or pc_gt.shape[2] != 3 or len(pc_pred) != len(pc_gt):
        raise ValueError(f'icp_run: pc_pred (N,P1,3) and pc_gt (N,P2,3) expected, got {tuple(pc_pred.shape)} and {tuple(pc_gt.shape)}')
    if pc_pred.device.type != 'cuda' or pc_gt.device != pc_pred.device:
        raise ValueError('icp_run: both clouds must be on the same cuda device (CPU tensors: gradient_icp_torch)')
    N, P1, _ = pc_pred.shape
    P2 = pc_gt.shape[1]
    dev = pc_pred.device
    p = pc_pred.detach().to(torch.float32).contiguous()
    g = pc_gt.detach().to(torch.float32).contiguous()
    n_iter = int(n_iter)
    nbytes = _icp_call('dbw_icp_workspace_bytes', N, P1, P2, n_iter)
    if nbytes == 0:
        raise ValueError(f'icp_run: sizes N={N}, P1={P1}, P2={P2}, n_iter={n_iter} are refused (empty clouds, or too large)')
    ws = torch.empty((nbytes + 15) // 16 * 2, dtype=torch.float64, device=dev)
    out = dict(cloud=torch.empty_like(p), R=torch.empty(N, 3, 3, dtype=torch.float32, device=dev),
               T=torch.empty(N, 3, dtype=torch.float32, device=dev), s=torch.empty(N, 3, dtype=torch.float32, device=dev),
               best=torch.empty(2, dtype=torch.float64, device=dev),
               trace=torch.empty(n_iter, 1 + _lib.ICP_TRACE_PER_INSTANCE * N, dtype=torch.float64, device=dev) if with_trace else None)
    with torch.cuda.device(dev):
        _icp_call('dbw_icp_run', _p(p), _p(g), N, P1, P2, int(bool(estimate_scale)), int(bool(anisotropic_scale)), float(lr), n_iter, int(splits),
                  _p(ws), _p(out['cloud']), _p(out['R']), _p(out['T']), _p(out['s']), _p(out['best']),
                  _p(out['trace']) if with_trace and n_iter else ctypes.c_void_p(0), _stream(dev))
    return out


def gradient_icp(pc_pred, pc_gt, estimate_scale=True, anisotropic_scale=False, lr=0.01, n_iter=300, batch_size=None, shared_params=False,
                 verbose=False, return_trace=False):
    """utils/icp.py:11-78: aligns pc_pred (N,P1,3) to pc_gt (N,P2,3) by minimising the Chamfer distance over a rotation, a translation and
    a scale per instance with Adam, keeping the best check of every 10th iteration -> (upd_pc_pred, [Rf (N,3,3), Tf (N,3), sf]) with
    upd_pc_pred = sf[:, None] * pc_pred @ Rf + Tf[:, None]; sf is (N,1) for an isotropic scale, (N,3) otherwise.  return_trace=True appends a
    dict: loss (n_iter,) fp64, R / T / s after every iteration's step, best_loss, best_iter.

    Device tensors run the loop behind one call (icp_run), CPU tensors gradient_icp_torch.  The mini-batch variant (`batch_size`) and
    `shared_params=True` (one transform for all instances, which the mini-batches need) are not built: the evaluator uses neither."""
    if batch_size is not None or shared_params:
        raise NotImplementedError('gradient_icp: batch_size / shared_params=True (the mini-batch ICP with one transform shared by all instances, '
                                  'icp.py:30-57) is not built: MeshEvaluator aligns every instance on its own with full clouds')
    if pc_pred.dim() != 3 or pc_gt.dim() != 3 or len(pc_pred) != len(pc_gt):
        raise ValueError('expected points to be of shape (N, P, D), with the same N')
    if pc_pred.device.type == 'cpu' and pc_gt.device.type == 'cpu':
        return gradient_icp_torch(pc_pred, pc_gt, estimate_scale, anisotropic_scale, lr, n_iter, verbose, return_trace)
    N, dt = len(pc_pred), pc_pred.dtype
    o = icp_run(pc_pred, pc_gt, estimate_scale, anisotropic_scale, lr, n_iter, with_trace=return_trace or verbose)
    iso = estimate_scale and not anisotropic_scale
    res = [o['R'].to(dt), o['T'].to(dt), (o['s'][:, :1] if iso else o['s']).to(dt)]
    if not (return_trace or verbose):
        return o['cloud'].to(dt), res
    tr, best = o['trace'].cpu(), o['best'].tolist()
    rts = tr[:, 1:].reshape(len(tr), N, _lib.ICP_TRACE_PER_INSTANCE)
    trace = dict(loss=tr[:, 0].clone(), best_loss=best[0], best_iter=int(best[1]), R=rts[..., :9].reshape(len(tr), N, 3, 3).to(dt),
                 T=rts[..., 9:12].to(dt), s=(rts[..., 12:13] if iso else rts[..., 12:15]).to(dt))
    if verbose:
        _print_checks(trace, N)
    return (o['cloud'].to(dt), res, trace) if return_trace else (o['cloud'].to(dt), res)


def unit_cube_frame(points):
    """(offset (3,), scale) that bring a cloud (.., 3) to the unit cube by its own bounding box: (points - offset) / scale has its box
    centred on 0 and its largest absolute coordinate at 0.5."""
    flat = points.reshape(-1, 3)
    offset = 0.5 * (flat.max(0).values + flat.min(0).values)
    return offset, (flat - offset).abs().max() * 2


def evaluate_aligned(model, points, normals=None, eval_dir=None, generator=None, samples=None, **evaluator_kwargs):
    """The ICP-aligned 3D scores of a trained model against a ground-truth cloud that shares neither frame nor scale with it (a
    BlendedMVS or custom scene: there is no DTU protocol for it).  The live blocks (model.blocks_mesh(filter_transparent=True)) and
    `points` (P,3) [, `normals` (P,3)] are brought to the unit cube by the ground truth's own bounding box, then scored by
    metrics.MeshEvaluator (keywords in evaluator_kwargs; `generator` / `samples`: MeshEvaluator.evaluate) -> OrderedDict of scores;
    with eval_dir, {eval_dir}/aligned_scores.tsv: a line of names, a line of '{:.5f}' values, like final_scores.tsv."""
    from .metrics import MeshEvaluator
    verts, faces = model.blocks_mesh(filter_transparent=True)
    verts = verts.detach()
    gt = torch.as_tensor(points).to(device=verts.device, dtype=verts.dtype).reshape(-1, 3)
    offset, scale = unit_cube_frame(gt)
    gt, verts = (gt - offset) / scale, (verts - offset) / scale
    if normals is not None:
        normals = torch.as_tensor(normals).to(device=verts.device, dtype=verts.dtype).reshape(1, -1, 3)
    names = evaluator_kwargs.pop('names', [n for n in MeshEvaluator.default_names
                                            if not n.startswith('3D-IoU') and (normals is not None or not n.startswith('normal'))])
    scores = MeshEvaluator(names=names, **evaluator_kwargs).evaluate((verts, faces), gt[None], normals, generator=generator, samples=samples)
    if eval_dir is not None:
        os.makedirs(str(eval_dir), exist_ok=True)
        with open(os.path.join(str(eval_dir), 'aligned_scores.tsv'), mode='w') as f:
            f.write('\t'.join(scores.keys()) + '\n')
            f.write('\t'.join('{:.5f}'.format(float(v)) for v in scores.values()) + '\n')
    return scores


# ------------------------------------------------------------------------------------------------ plane RANSAC
PlaneResult = collections.namedtuple('PlaneResult', 'normal offset n_inliers best counts mask triples rounds')
PlaneResult.__doc__ = """A plane fit, every field a tensor on the device of the points: normal (3,) and offset () fp64 (normal . p = offset on the
plane; zeros when no hypothesis was admissible), n_inliers () int32 of the final plane, best () int32 (the winning hypothesis, -1: none),
counts (H,) int32 or None (-1: degenerate or inadmissible), mask (N,) bool or None, triples (H,3) int32, rounds () int32 (refinement rounds
done)."""
PLANE_MODES = {'orthogonal': _lib.EVAL_PLANE_ORTHOGONAL, 'vertical': _lib.EVAL_PLANE_VERTICAL}
PLANE_STREAM = 0x504C414E                # csrc/plane_math.h: PLANE_STREAM
VERTICAL_THRESH = 0.001                  # ransac.py:32


def plane_draw(seed, n_hyp, N):
    """csrc/plane_math.h plane_draw for j = 0 .. n_hyp - 1 -> (n_hyp,3) int32 numpy: Philox4x32-10 with the counter (j, 0, 0, 'PLAN') and the
    key (seed low, seed high), word k scaled to [0, N) by (word * N) >> 32."""
    M32 = np.uint64(0xffffffff)
    c = [np.arange(n_hyp, dtype=np.uint64), np.zeros(n_hyp, np.uint64), np.zeros(n_hyp, np.uint64), np.full(n_hyp, PLANE_STREAM, np.uint64)]
    k0, k1 = np.uint64(int(seed) & 0xffffffff), np.uint64((int(seed) >> 32) & 0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack([(w * np.uint64(N)) >> np.uint64(32) for w in c[:3]], 1).astype(np.int32)


def _plane_args(points, n_hyp, thresh, residual, up, max_tilt, cams, min_side, refine, triples):
    if residual not in PLANE_MODES:
        raise ValueError(f"plane_ransac: residual must be 'orthogonal' or 'vertical', got {residual!r}")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f'plane_ransac: points (N,3) expected, got {tuple(points.shape)}')
    N = points.shape[0]
    if triples is not None:
        triples = torch.as_tensor(triples).to(device=points.device, dtype=torch.int32).reshape(-1, 3).contiguous()
        n_hyp = triples.shape[0]
    n_hyp, refine = int(n_hyp), int(refine)
    if not (1 <= n_hyp <= 4096 and 3 <= N < 2 ** 31 and 0 <= refine <= 8):
        raise ValueError(f'plane_ransac: 1 <= n_hyp <= 4096, 3 <= N < 2^31 and 0 <= refine <= 8 expected, got n_hyp={n_hyp}, N={N}, refine={refine}')
    mode = PLANE_MODES[residual]
    if thresh is None:
        if mode == _lib.EVAL_PLANE_VERTICAL:
            thresh = VERTICAL_THRESH
        else:                                # (one host read: give thresh to avoid it) 1 % of the bounding box's diagonal
            thresh = 0.01 * float((points.max(0).values.double() - points.min(0).values.double()).norm())
    thresh = float(np.float32(thresh))
    if not (thresh > 0 and math.isfinite(thresh)):
        raise ValueError(f'plane_ransac: thresh must be positive and finite, got {thresh}')
    tau = thresh if mode == _lib.EVAL_PLANE_ORTHOGONAL else 0.0
    thresh2 = float(np.float32(thresh) * np.float32(thresh)) if mode == _lib.EVAL_PLANE_ORTHOGONAL else thresh
    if not thresh2 > 0:
        raise ValueError(f'plane_ransac: thresh {thresh} squares to 0 in fp32')
    cos_tilt, min_cams = 0.0, 0
    if mode == _lib.EVAL_PLANE_VERTICAL:
        up, cams, refine = None, None, 0
    if up is not None:
        up = torch.as_tensor(up).detach().to(device=points.device, dtype=torch.float32).reshape(3).contiguous()
        cos_tilt = float(np.float32(math.cos(math.radians(float(max_tilt)))))
    if cams is not None:
        cams = torch.as_tensor(cams).detach().to(device=points.device, dtype=torch.float32).reshape(-1, 3).contiguous()
        if not 1 <= cams.shape[0] <= 65536:
            raise ValueError(f'plane_ransac: 1 to 65536 camera centres expected, got {cams.shape[0]}')
        min_cams = min(cams.shape[0], max(0, math.ceil(float(min_side) * cams.shape[0] - 1e-9)))
    return n_hyp, mode, thresh2, tau, up, cos_tilt, cams, min_cams, refine, triples


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _plane_hypotheses(tri_pts, mode, up, cos_tilt, cams, tau, min_cams, dt):
    """csrc/plane_math.h plane_from_triple and plane_admissible on (H,3,3) points in dtype dt, expression by expression -> (planes (H,4),
    valid (H,) bool).  Computed on the CPU, where every torch op is one IEEE rounding: the fp32 planes are those of the kernel, bit for bit."""
    a, b, c = tri_pts[:, 0], tri_pts[:, 1], tri_pts[:, 2]
    e1, e2 = b - a, c - a
    m = torch.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    L2 = _dot3(m, m)
    valid = (L2 < math.inf) & ~(L2 <= torch.tensor(1e-8, dtype=dt) * (_dot3(e1, e1) * _dot3(e2, e2)))
    if mode == _lib.EVAL_PLANE_VERTICAL:
        valid = valid & (m[:, 2] != 0)
        n = m / m[:, 2:3]
    else:
        n = m / L2.sqrt()[:, None]
        if up is not None:
            n = torch.where((_dot3(n, up[None]) < 0)[:, None], -n, n)
    d = _dot3(n, a)
    if mode == _lib.EVAL_PLANE_ORTHOGONAL:
        if up is not None:
            valid = valid & (_dot3(n, up[None]) >= cos_tilt)
        if cams is not None:
            r = ((n[:, None, 0] * cams[None, :, 0] + n[:, None, 1] * cams[None, :, 1]) + n[:, None, 2] * cams[None, :, 2]) - d[:, None]
            valid = valid & ((r > tau).sum(1) >= min_cams)
    planes = torch.cat([n, d[:, None]], 1)
    return torch.where(valid[:, None], planes, torch.zeros_like(planes)), valid


def _plane_inliers(pl, x, y, z, thresh2):
    r = ((pl[0] * x + pl[1] * y) + pl[2] * z) - pl[3]
    return r * r < thresh2


def plane_ransac_torch(points, n_hyp=512, thresh=None, residual='orthogonal', up=None, max_tilt=60.0, cams=None, min_side=0.9, refine=2, seed=0,
                       triples=None, return_counts=False, return_mask=False, dtype=torch.float32, chunk_elems=1 << 24):
    """plane_ransac in torch, on any device: the triples of csrc/plane_math.h's plane_draw, the hypotheses and their priors expression by
    expression (on the CPU: H x a few numbers), the scoring in chunks of hypotheses that materialise a (chunk, N) residual matrix as the
    reference's batches do, the refinement in fp64 with torch.linalg.eigh.  dtype=torch.float32 states the kernel's arithmetic: the same
    counts and the same best hypothesis on the CPU (on a device torch's own kernels have been seen a point off at the threshold); dtype=torch.float64 does everything in fp64 and is the oracle of the tests.  Reads the best index to
    the host."""
    n_hyp, mode, thresh2, tau, up, cos_tilt, cams, min_cams, refine, triples = _plane_args(points, n_hyp, thresh, residual, up, max_tilt, cams,
                                                                                          min_side, refine, triples)
    dev, N = points.device, points.shape[0]
    pts = points.detach().to(torch.float32)
    if triples is None:
        triples = torch.from_numpy(plane_draw(seed, n_hyp, N)).to(dev)
    t64 = triples.to(torch.int64)
    in_range = ((t64 >= 0) & (t64 < N)).all(1)
    tri_pts = pts[t64.clamp(0, N - 1).reshape(-1)].reshape(n_hyp, 3, 3).cpu().to(dtype)
    cpu = lambda t: None if t is None else t.cpu().to(dtype)                    # noqa: E731
    th2 = torch.tensor(thresh2, dtype=dtype)
    planes, valid = _plane_hypotheses(tri_pts, mode, cpu(up), torch.tensor(cos_tilt, dtype=dtype), cpu(cams), torch.tensor(tau, dtype=dtype),
                                      min_cams, dtype)
    planes, valid, th2 = planes.to(dev), valid.to(dev) & in_range, th2.to(dev)
    x, y, z = (pts[:, k].to(dtype) for k in range(3))
    counts = torch.empty(n_hyp, dtype=torch.int32, device=dev)
    step = max(1, chunk_elems // N)
    for a in range(0, n_hyp, step):
        pl = planes[a:a + step]
        r = ((pl[:, 0:1] * x[None] + pl[:, 1:2] * y[None]) + pl[:, 2:3] * z[None]) - pl[:, 3:4]
        counts[a:a + step] = (r * r < th2).sum(1)
    counts = torch.where(valid, counts, torch.full_like(counts, -1))
    top = counts.max()
    best = int(torch.where(counts == top, torch.arange(n_hyp, device=dev), n_hyp).min()) if int(top) >= 0 else -1
    plane = torch.zeros(4, dtype=torch.float64, device=dev)
    rounds = 0
    if best >= 0:
        plane = planes[best].to(torch.float64)
        a0 = pts[t64[best, 0]].to(torch.float64)
        for _ in range(refine):
            inl = _plane_inliers(plane.to(dtype), x, y, z, th2)
            q = pts[inl].to(torch.float64) - a0
            if q.shape[0] < 3:
                break
            mean = q.sum(0) / q.shape[0]
            cov = (q.T @ q) / q.shape[0] - mean[:, None] * mean[None]
            v = torch.linalg.eigh(cov).eigenvectors[:, 0]
            v = torch.where((v * plane[:3]).sum() < 0, -v, v)
            plane = torch.cat([v, (v * (a0 + mean)).sum()[None]])
            rounds += 1
        mask = _plane_inliers(plane.to(dtype), x, y, z, th2)
    else:
        mask = torch.zeros(N, dtype=torch.bool, device=dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)              # noqa: E731
    return PlaneResult(plane[:3], plane[3], mask.sum().to(torch.int32), i32(best), counts if return_counts else None,
                       mask if return_mask else None, triples, i32(rounds))


def plane_fit(points, n_hyp, mode, thresh2, seed=0, triples=None, up=None, cos_tilt=0.0, cams=None, tau=0.0, min_cams=0, refine=0,
              with_counts=True, with_mask=True):
    """dbw_eval_plane_fit on device tensors, arguments as in include/dbw_eval.h (points (N,3) fp32 contiguous; triples int32; up, cams fp32)
    -> dict(plane (4,) fp64, info (4,) int32, counts (H,) int32 or None, triples (H,3) int32, mask (N,) uint8 or None).  Everything is
    enqueued on the current stream; nothing is read by the host."""
    dev, N = points.device, points.shape[0]
    lib = _lib.family('eval')
    nbytes = lib.dbw_eval_plane_workspace_bytes(N, int(n_hyp))
    if nbytes == 0:
        raise ValueError(f'plane_fit: sizes N={N}, H={n_hyp} are refused (1 <= H <= 4096, 3 <= N < 2^31)')
    ws = torch.empty((nbytes + 15) // 16 * 2, dtype=torch.float64, device=dev)
    out = dict(plane=torch.empty(4, dtype=torch.float64, device=dev), info=torch.empty(4, dtype=torch.int32, device=dev),
               counts=torch.empty(n_hyp, dtype=torch.int32, device=dev) if with_counts else None,
               triples=torch.empty(n_hyp, 3, dtype=torch.int32, device=dev),
               mask=torch.empty(N, dtype=torch.uint8, device=dev) if with_mask else None)
    seed = int(seed) & 0xffffffffffffffff
    seed = seed - (1 << 64) if seed >= 1 << 63 else seed                        # the 64 bits, as the int64_t of the prototype
    with torch.cuda.device(dev):
        _call('dbw_eval_plane_fit', _p(points), N, int(n_hyp), int(mode), float(thresh2), seed, _p(triples), _p(up), float(cos_tilt), _p(cams),
              0 if cams is None else cams.shape[0], float(tau), int(min_cams), int(refine), _p(ws), _p(out['plane']), _p(out['info']),
              _p(out['counts']), _p(out['triples']), _p(out['mask']), _stream(dev))
    return out


def plane_ransac(points, n_hyp=512, thresh=None, residual='orthogonal', up=None, max_tilt=60.0, cams=None, min_side=0.9, refine=2, seed=0,
                 triples=None, return_counts=False, return_mask=False):
    """Robust plane fit of a cloud (N,3): n_hyp planes through random triples of points (or through the rows of `triples` (H,3)), each scored
    by its number of inliers among all N points, the best one (lowest index on ties) refined -> PlaneResult.

    residual 'orthogonal': unit normal, a point is an inlier iff its distance is below `thresh` (None: 1 % of the bounding box's diagonal,
    which costs one host read); `refine` rounds refit the plane to its inliers (smallest eigenvector of their covariance, fp64).  Priors:
    with `up` (3,), the normal points to the side of up and its tilt against it is at most `max_tilt` degrees; with `cams` (M,3), at least
    ceil(min_side * M) camera centres lie more than `thresh` above the plane.  residual 'vertical': the reference's regression
    z = p0 + p1 x + p2 y through the triple (ransac.py), inlier iff the SQUARED residual is below `thresh` (None: 0.001); no priors, no
    refinement; normal = (-p1, -p2, 1), offset = p0.

    Device tensors run csrc/plane_fit.hip in one call with no host read (the result's fields are device tensors), CPU tensors
    plane_ransac_torch.  The draw of the triples is a function of (seed, hypothesis index, N) alone, the same on both paths."""
    if points.device.type == 'cpu':
        return plane_ransac_torch(points, n_hyp, thresh, residual, up, max_tilt, cams, min_side, refine, seed, triples, return_counts, return_mask)
    n_hyp, mode, thresh2, tau, up, cos_tilt, cams, min_cams, refine, triples = _plane_args(points, n_hyp, thresh, residual, up, max_tilt, cams,
                                                                                          min_side, refine, triples)
    pts = points.detach().to(torch.float32).contiguous()
    o = plane_fit(pts, n_hyp, mode, thresh2, seed, triples, up, cos_tilt, cams, tau, min_cams, refine, with_counts=return_counts,
                  with_mask=return_mask)
    return PlaneResult(o['plane'][:3], o['plane'][3], o['info'][2], o['info'][0], o['counts'], None if o['mask'] is None else o['mask'].bool(),
                       o['triples'], o['info'][3])


def filter_ground(points, thresh=VERTICAL_THRESH, n_iter=100, seed=0, batch_size=10, triples=None):
    """The ground filter of dtu_3d_process.py:36-41: Ransac() of utils/ransac.py fits z = p0 + p1 x + p2 y to the cloud (n_iter // batch_size
    * batch_size hypotheses, each the plane through three points; the first hypothesis with the most inliers wins), and the points whose
    squared residual is below `thresh` are dropped -> (points[~inlier], (p0, p1, p2) as a (3,) fp64 tensor).  The triples are this
    package's counter-based draw, not torch.randint's, unless `triples` (H,3) gives them."""
    n_hyp = int(n_iter) // int(batch_size) * int(batch_size)
    res = plane_ransac(points, n_hyp=n_hyp, thresh=thresh, residual='vertical', refine=0, seed=seed, triples=triples, return_mask=True)
    params = torch.stack([res.offset, -res.normal[0], -res.normal[1]])
    return points[~res.mask], params


# ------------------------------------------------------------------------------------------------ k-means with per-cluster PCA
ClusterResult = collections.namedtuple('ClusterResult', 'centres labels counts mean cov evals axes rounds changed n_nonempty')
ClusterResult.__doc__ = """A k-means fit, every field a tensor on the device of the points: centres (K,3) fp32, the centres the labels belong to;
labels (N,) int32 (-1: a point with a non-finite coordinate); counts (K,) int32; mean (K,3), cov (K,6: xx xy xz yy yz zz), evals (K,3,
descending) and axes (K,3,3: row i the unit eigenvector of evals[i], a proper rotation) fp64; rounds, changed (labels that changed in the last
pass), n_nonempty () int32."""
CLUSTER_MAX_K, CLUSTER_MAX_ITER = 256, 64        # csrc/cluster_math.h
_COV_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def _cluster_args(points, k, n_iter, init):
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f'cluster_points: points (N,3) expected, got {tuple(points.shape)}')
    if init is not None:
        init = torch.as_tensor(init).detach().to(device=points.device, dtype=torch.float32).reshape(-1, 3).contiguous()
        if init.shape[0] != int(k):
            raise ValueError(f'cluster_points: init (k,3) = ({int(k)},3) expected, got {tuple(init.shape)}')
    k, n_iter, N = int(k), int(n_iter), points.shape[0]
    if not (1 <= k <= CLUSTER_MAX_K and k <= N < 2 ** 31 and 0 <= n_iter <= CLUSTER_MAX_ITER):
        raise ValueError(f'cluster_points: 1 <= k <= {CLUSTER_MAX_K}, k <= N < 2^31 and 0 <= n_iter <= {CLUSTER_MAX_ITER} expected, got k={k}, '
                         f'N={N}, n_iter={n_iter}')
    return k, n_iter, init


def _cluster_dist2(p, c):
    d = p[:, None, :] - c[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _cluster_assign(p, finite, c, chunk):
    """labels (N,) int64 of the fp32 points p against the centres c: the first smallest dist2, -1 for a non-finite point"""
    out = torch.empty(p.shape[0], dtype=torch.int64, device=p.device)
    for a in range(0, p.shape[0], chunk):
        d2 = _cluster_dist2(p[a:a + chunk], c)
        d2 = torch.where(d2 != d2, torch.full_like(d2, math.inf), d2)               # (a NaN distance is never the smallest)
        m = d2.min(1, keepdim=True).values
        ks = torch.arange(c.shape[0], device=p.device)[None].expand_as(d2)
        out[a:a + chunk] = torch.where(d2 == m, ks, c.shape[0]).min(1).values
    return torch.where(finite, out, torch.full_like(out, -1))


def _cluster_moments(p, labels, c):
    """(K,10) fp64: count, sum d, sum d d^T of every cluster about its centre"""
    K = c.shape[0]
    keep = labels >= 0
    lab = labels[keep]
    d = p[keep].to(torch.float64) - c.to(torch.float64)[lab]
    terms = torch.cat([torch.ones_like(d[:, :1]), d] + [(d[:, a] * d[:, b])[:, None] for a, b in _COV_PAIRS], 1)
    return torch.zeros(K, 10, dtype=torch.float64, device=p.device).index_add_(0, lab, terms)


def _cluster_finish(sums, c):
    n = sums[:, :1]
    safe = n.clamp(min=1)
    m = sums[:, 1:4] / safe
    mean = torch.where(n > 0, c.to(torch.float64) + m, c.to(torch.float64))
    cov = sums[:, 4:] / safe - torch.stack([m[:, a] * m[:, b] for a, b in _COV_PAIRS], 1)
    return mean.to(torch.float32), mean, torch.where(n >= 2, cov, torch.zeros_like(cov)), n[:, 0].to(torch.int32)


def _cluster_seed(p, finite, K):
    """farthest-point seeding (include/dbw_eval.h) -> centres (K,3) fp32"""
    q = p[finite]
    if q.shape[0] == 0:
        return torch.zeros(K, 3, dtype=torch.float32, device=p.device)
    first = lambda hit: torch.where(hit, torch.arange(q.shape[0], device=p.device), q.shape[0]).min()       # noqa: E731
    c = (q.to(torch.float64).sum(0) / q.shape[0]).to(torch.float32)
    d = _cluster_dist2(q, c[None])[:, 0]
    order = [first(d == d.min())]
    mind = None
    for _ in range(1, K):
        d = _cluster_dist2(q, q[order[-1]][None])[:, 0]
        mind = d if mind is None else torch.minimum(mind, d)
        order.append(first(mind == mind.max()))
    return q[torch.stack(order)]


def _cluster_axes(cov, counts):
    """eigenvalues (descending) and axes (rows, signed as csrc/cluster_math.h's sym3_eigen signs them) of (K,6) covariances, through eigh"""
    C = torch.stack([cov[:, 0], cov[:, 1], cov[:, 2], cov[:, 1], cov[:, 3], cov[:, 4], cov[:, 2], cov[:, 4], cov[:, 5]], 1).reshape(-1, 3, 3)
    w, V = torch.linalg.eigh(C.cpu())                                               # (K small matrices: the host's LAPACK)
    w, V = w.to(cov.device).flip(1), V.to(cov.device).flip(2).transpose(1, 2)      # descending, vectors as rows
    big = V[:, :2].abs().argmax(2, keepdim=True)
    sign = torch.where(V[:, :2].gather(2, big) < 0, -1.0, 1.0)
    r01 = V[:, :2] * sign
    axes = torch.cat([r01, torch.linalg.cross(r01[:, 0], r01[:, 1])[:, None]], 1)
    few = (counts < 2)[:, None]
    eye = torch.eye(3, dtype=cov.dtype, device=cov.device)[None].expand_as(axes)
    return torch.where(few, torch.zeros_like(w), w), torch.where(few[:, :, None], eye, axes)


def cluster_points_torch(points, k, n_iter=20, init=None, chunk=1 << 16):
    """cluster_points in torch, on any device: the readable restatement of csrc/cluster_fit.hip and the path of CPU tensors.  fp32 distances
    in the stated order of operations, fp64 sums (index_add_: torch's order, not the kernel's -- the sums agree within the rounding of a
    reordered fp64 sum, the labels exactly unless a centre differs in its last bit), eigh for the axes."""
    k, n_iter, init = _cluster_args(points, k, n_iter, init)
    p = points.detach().to(torch.float32)
    finite = torch.isfinite(p).all(1)
    c = _cluster_seed(p, finite, k) if init is None else init.clone()
    prev = None
    for r in range(n_iter + 1):
        labels = _cluster_assign(p, finite, c, chunk)
        changed = (labels != prev).sum() if prev is not None else torch.tensor(p.shape[0], device=p.device)
        sums = _cluster_moments(p, labels, c)
        new, mean, cov, counts = _cluster_finish(sums, c)
        if r < n_iter:
            c, prev = new, labels
    evals, axes = _cluster_axes(cov, counts)
    i32 = lambda v: torch.as_tensor(v, device=p.device).to(torch.int32)            # noqa: E731
    return ClusterResult(c, labels.to(torch.int32), counts, mean, cov, evals, axes, i32(n_iter), i32(changed), i32((counts > 0).sum()))


def cluster_fit(points, k, n_iter=20, init=None, with_labels=True):
    """dbw_eval_cluster_fit on device tensors, arguments as in include/dbw_eval.h (points (N,3) fp32 contiguous, init (k,3) fp32 or None) ->
    dict(centres, labels or None, counts, mean, cov, evals, axes, info (4,) int32).  Everything is enqueued on the current stream; nothing is
    read by the host."""
    dev, N = points.device, points.shape[0]
    lib = _lib.family('eval')
    nbytes = lib.dbw_eval_cluster_workspace_bytes(N, int(k))
    if nbytes == 0:
        raise ValueError(f'cluster_fit: sizes N={N}, K={k} are refused (1 <= K <= {CLUSTER_MAX_K}, K <= N < 2^31)')
    ws = torch.empty((nbytes + 15) // 16 * 2, dtype=torch.float64, device=dev)
    f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)      # noqa: E731
    out = dict(centres=torch.empty(k, 3, dtype=torch.float32, device=dev), labels=torch.empty(N, dtype=torch.int32, device=dev) if with_labels else None,
               counts=torch.empty(k, dtype=torch.int32, device=dev), mean=f64(k, 3), cov=f64(k, 6), evals=f64(k, 3), axes=f64(k, 3, 3),
               info=torch.empty(4, dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        _call('dbw_eval_cluster_fit', _p(points), N, int(k), _p(init), int(n_iter), _p(ws), _p(out['centres']), _p(out['labels']), _p(out['counts']),
              _p(out['mean']), _p(out['cov']), _p(out['evals']), _p(out['axes']), _p(out['info']), _stream(dev))
    return out


def cluster_points(points, k, n_iter=20, init=None):
    """k-means of a cloud (N,3) with a PCA of every cluster -> ClusterResult.  k centres: the rows of `init` (k,3), or deterministic
    farthest-point seeding (centre 0 the point nearest the mean, centre j the point farthest from the centres before it, the lowest index on
    ties); n_iter Lloyd rounds with no early stop, then one more pass against the final centres that gives every field.  A point with a
    non-finite coordinate gets the label -1 and enters no sum; an empty cluster keeps its centre.

    Device tensors run csrc/cluster_fit.hip in one call with no host read (the result's fields are device tensors) and give the same bytes on
    every call; CPU tensors run cluster_points_torch."""
    if points.device.type == 'cpu':
        return cluster_points_torch(points, k, n_iter, init)
    k, n_iter, init = _cluster_args(points, k, n_iter, init)
    o = cluster_fit(points.detach().to(torch.float32).contiguous(), k, n_iter, init)
    return ClusterResult(o['centres'], o['labels'], o['counts'], o['mean'], o['cov'], o['evals'], o['axes'], o['info'][0], o['info'][1], o['info'][2])


# ---------------------------------------------------------------------------------------------------------------- the surface term
def _closest_on_faces(p, tri):
    """p (n,3), tri (F,3,3) -> (d2 (n,F), bary (n,F,3)): per face the projection onto its plane where that lies inside, else the nearest of
    the clamped projections onto its sides (a face without area: its sides) -- the definition csrc/surface_math.h implements, in p's dtype."""
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    e1, e2, q = b - a, c - a, p[:, None, :] - a
    n = torch.linalg.cross(e1, e2)
    nn = (n * n).sum(-1)
    ok = nn > 0
    den = torch.where(ok, nn, torch.ones_like(nn))
    u = (torch.linalg.cross(q, e2.expand_as(q)) * n).sum(-1) / den
    v = (torch.linalg.cross(e1.expand_as(q), q) * n).sum(-1) / den
    inside = ok & (u >= 0) & (v >= 0) & (u + v <= 1)

    def at(u_, v_):
        r = q - (u_[..., None] * e1 + v_[..., None] * e2)
        return (r * r).sum(-1)

    def seg(q0, d):
        dd = (d * d).sum(-1)
        t = (q0 * d).sum(-1) / torch.where(dd > 0, dd, torch.ones_like(dd))
        return torch.where(dd > 0, t, torch.zeros_like(t)).clamp(0, 1)

    s1, s2, s3 = seg(q, e1), seg(q - e1, e2 - e1), seg(q - e2, -e2)
    zero = torch.zeros_like(s1)
    cands = [(s1, zero), (1 - s2, s2), (zero, 1 - s3)]
    d_side = torch.stack([at(*c_) for c_ in cands], 0)
    j = d_side.argmin(0)
    us = torch.stack([c_[0] for c_ in cands], 0).gather(0, j[None])[0]
    vs = torch.stack([c_[1] for c_ in cands], 0).gather(0, j[None])[0]
    u, v = torch.where(inside, u, us), torch.where(inside, v, vs)
    return at(u, v), torch.stack([1 - u - v, u, v], -1)


def surface_draw(seed, step, n_points, n_cloud):
    """The cloud indices a step draws (csrc/surface_math.h: surface_draw_index), on the host: word 0 of Philox4x32-10 with counter
    (i, 2, step) and key seed, mod the cloud's size -> (n_points,) int64."""
    i = np.arange(int(n_points), dtype=np.uint64)
    c = [i, np.full_like(i, 2), np.full_like(i, int(step) & 0xffffffff), np.full_like(i, int(step) >> 32)]
    k = [np.uint64(int(seed) & 0xffffffff), np.uint64((int(seed) >> 32) & 0xffffffff)]
    m32 = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k[0]) & m32, p1 & m32, ((p0 >> np.uint64(32)) ^ c[3] ^ k[1]) & m32, p0 & m32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & m32, (k[1] + np.uint64(0xBB67AE85)) & m32]
    return torch.from_numpy((c[0] % np.uint64(int(n_cloud))).astype(np.int64))


def surface_term_torch(points, verts, faces, face_group, group_keep, vert_alpha, vert_group, *, n_points, tau, back, seed, step, weight,
                       back_count=None, chunk=1024):
    """ops.surface_term in torch, in the dtype of verts, on any device: the readable statement of DESIGN.md 6u, the timing baseline of
    tools/surface_bench.py and, in float64, the gradient reference of the tests.  Autograd gives the envelope gradient by itself: the
    closest point is differentiated through the barycentrics of the winning face, and their derivative is orthogonal to p - c or clamped.
    To keep exactly the stated gradient (-2 b_m (p - c), 2 a_k (x_v - nn)) the barycentrics and the nearest neighbours are detached."""
    dt, dev = verts.dtype, verts.device
    P = points.to(device=dev, dtype=dt)
    N, V = P.shape[0], verts.shape[0]
    idx = surface_draw(seed, step, n_points, N).to(dev) if n_points else torch.arange(N, device=dev)
    fk = torch.ones(faces.shape[0], dtype=torch.bool, device=dev)
    if group_keep is not None:
        G = face_group.numel() - 1
        counts = (face_group[1:] - face_group[:-1]).to(torch.int64)
        fk = torch.repeat_interleave(group_keep.to(torch.bool), counts, output_size=faces.shape[0]) if G else fk
    fid = fk.nonzero().flatten()
    fc = faces.to(torch.int64)[fid]
    t2 = float(tau) ** 2
    total = verts.new_zeros(())
    p_all = P[idx]
    for s in range(0, p_all.shape[0], chunk):
        p = p_all[s:s + chunk]
        with torch.no_grad():
            d2, bary = _closest_on_faces(p, verts.detach()[fc])
            j = d2.argmin(1)
            b = bary[torch.arange(len(j), device=dev), j]
        c = (b[..., None] * verts[fc[j]]).sum(1)
        d2 = ((p - c) ** 2).sum(-1)
        total = total + torch.where(d2 < t2, d2, torch.full_like(d2, t2)).sum()
    value = total / p_all.shape[0]
    if back > 0:
        sel = (vert_group >= 0).nonzero().flatten()
        x = verts[sel]
        with torch.no_grad():
            nn_i = torch.cat([((x[s:s + chunk, None, :].detach() - P[None]) ** 2).sum(-1).argmin(1) for s in range(0, x.shape[0], chunk)])
        d2 = ((x - P[nn_i]) ** 2).sum(-1)
        rho = torch.where(d2 < t2, d2, torch.full_like(d2, t2))
        bc = float(back_count) if back_count is not None else float(sel.numel())        # (n_blocks * BNV: the block vertices)
        value = value + float(back) * (vert_alpha.to(dt)[vert_group[sel].to(torch.int64)] * rho).sum() / bc
    return float(weight) * value
