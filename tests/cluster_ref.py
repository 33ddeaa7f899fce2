"""Checker side of the k-means / PCA fit: the host build of csrc/cluster_math.h (tests/host_cluster_math.cpp through host_build.host_lib)
behind numpy arguments, an independent numpy restatement of the same algorithm (np_*), the seeded clouds the tests share, and the bounds."""
import ctypes

import numpy as np

import host_build

NSUM = 10
EPS64 = 2.0 ** -52
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))          # xx xy xz yy yz zz


def lib():
    return host_build.host_lib('cluster_math')


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _f32(a, shape=(-1, 3)):
    return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float32)).reshape(shape)


# ------------------------------------------------------------------------------------------------ the host build
def host_fit(points, K, n_iter=0, init=None):
    """host_cluster_fit -> dict(rc, centres, labels, counts, mean, cov, evals, axes, info, sums (K,10))"""
    pts, init = _f32(points), _f32(init)
    N = len(pts)
    o = dict(centres=np.zeros((K, 3), np.float32), labels=np.zeros(N, np.int32), counts=np.zeros(K, np.int32), mean=np.zeros((K, 3)),
             cov=np.zeros((K, 6)), evals=np.zeros((K, 3)), axes=np.zeros((K, 3, 3)), info=np.zeros(4, np.int32), sums=np.zeros((K, NSUM)))
    o['rc'] = lib().host_cluster_fit(_ptr(pts), ctypes.c_int64(N), int(K), _ptr(init), int(n_iter), _ptr(o['centres']), _ptr(o['labels']),
                                     _ptr(o['counts']), _ptr(o['mean']), _ptr(o['cov']), _ptr(o['evals']), _ptr(o['axes']), _ptr(o['info']),
                                     _ptr(o['sums']))
    return o


def host_seed(points, K):
    pts = _f32(points)
    centres, order = np.zeros((K, 3), np.float32), np.zeros(K, np.int64)
    lib().host_cluster_seed(_ptr(pts), ctypes.c_int64(len(pts)), int(K), _ptr(centres), _ptr(order))
    return centres, order


def host_assign(points, centres):
    pts, cen = _f32(points), _f32(centres)
    labels, d2 = np.zeros(len(pts), np.int32), np.zeros(len(pts), np.float32)
    lib().host_cluster_assign(_ptr(pts), ctypes.c_int64(len(pts)), _ptr(cen), len(cen), _ptr(labels), _ptr(d2))
    return labels, d2


def host_moments(points, centres, labels):
    pts, cen, lab = _f32(points), _f32(centres), np.ascontiguousarray(labels, dtype=np.int32)
    sums = np.zeros((len(cen), NSUM))
    lib().host_cluster_moments(_ptr(pts), ctypes.c_int64(len(pts)), _ptr(cen), len(cen), _ptr(lab), _ptr(sums))
    return sums


def host_eigen(C):
    C = np.ascontiguousarray(np.asarray(C, dtype=np.float64).reshape(-1, 6))
    evals, axes = np.zeros((len(C), 3)), np.zeros((len(C), 3, 3))
    lib().host_sym3_eigen(_ptr(C), ctypes.c_int64(len(C)), _ptr(evals), _ptr(axes))
    return evals, axes


def host_keys(d):
    d = np.ascontiguousarray(d, dtype=np.float32)
    far, near = np.zeros(len(d), np.uint64), np.zeros(len(d), np.uint64)
    lib().host_cluster_keys(_ptr(d), ctypes.c_int64(len(d)), _ptr(far), _ptr(near))
    return far, near


# ------------------------------------------------------------------------------------------------ numpy, on its own
def np_finite(p):
    return np.isfinite(p).all(1)


def np_dist2(p, c):
    """(N,K) fp32: ((dx*dx + dy*dy) + dz*dz), every numpy operation on fp32 arrays one rounding"""
    with np.errstate(all='ignore'):
        d = p[:, None, :].astype(np.float32) - c[None, :, :].astype(np.float32)
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def np_assign(p, c):
    d2 = np_dist2(p, c)
    d2 = np.where(np.isnan(d2), np.float32(np.inf), d2)          # (a NaN distance is never the smallest)
    return np.where(np_finite(p), d2.argmin(1), -1).astype(np.int32)       # argmin: the first of equal ones


def np_terms(p, c, labels, k):
    """(n,10) fp64: the terms of cluster k's ten sums"""
    d = p[labels == k].astype(np.float64) - c[k].astype(np.float64)
    return np.concatenate([np.ones((len(d), 1)), d] + [(d[:, a] * d[:, b])[:, None] for a, b in PAIRS], 1)


def np_moments(p, c, labels):
    """-> (sums (K,10) fp64, bound (K,10): 8 eps64 sum|term|, what a sum of the same exact terms in another order may differ by).  Every sum is
    numpy's pairwise sum over a contiguous column -- not an axis-0 reduction, which adds row by row: one running sum over these terms drifts
    downwards by about n / 8 ulp (tests/host_cluster_math.cpp, host_cluster_moments says why), which is the reference's own error and, from a
    hundred points on, more than the bound."""
    terms = [np_terms(p, c, labels, k) for k in range(len(c))]
    return (np.stack([np.array([np.ascontiguousarray(t[:, j]).sum() for j in range(NSUM)]) for t in terms]),
            np.stack([8 * EPS64 * np.abs(t).sum(0) for t in terms]))


def np_finish(sums, c):
    """-> (new centres (K,3) fp32, mean (K,3), cov (K,6), counts (K,))"""
    n = sums[:, 0]
    safe = np.maximum(n, 1)[:, None]
    m = sums[:, 1:4] / safe
    mean = np.where(n[:, None] > 0, c.astype(np.float64) + m, c.astype(np.float64))
    cov = sums[:, 4:] / safe - np.stack([m[:, a] * m[:, b] for a, b in PAIRS], 1)
    cov = np.where(n[:, None] >= 2, cov, 0.0)
    return mean.astype(np.float32), mean, cov, n.astype(np.int32)


def np_seed(p, K):
    """-> (centres (K,3) fp32, order (K,)): farthest-point seeding, argmin / argmax take the first of equal ones"""
    fin = np_finite(p)
    idx = np.flatnonzero(fin)
    if len(idx) == 0:
        return np.zeros((K, 3), np.float32), np.full(K, -1)
    q = p[idx].astype(np.float32)
    c = (q.astype(np.float64).sum(0) / len(q)).astype(np.float32)
    order = [int(np_dist2(q, c[None])[:, 0].argmin())]
    mind = None
    for _ in range(1, K):
        d = np_dist2(q, q[order[-1]][None])[:, 0]
        mind = d if mind is None else np.minimum(mind, d)
        order.append(int(mind.argmax()))
    return q[order], idx[order]


def np_fit(p, K, n_iter=0, init=None):
    p = _f32(p)
    c = np_seed(p, K)[0] if init is None else _f32(init).copy()
    rounds = []
    for r in range(n_iter + 1):
        labels = np_assign(p, c)
        sums, bound = np_moments(p, c, labels)
        new, mean, cov, counts = np_finish(sums, c)
        rounds.append(dict(centres=c.copy(), labels=labels, sums=sums, bound=bound, mean=mean, cov=cov, counts=counts))
        if r < n_iter:
            c = new
    return rounds


# ------------------------------------------------------------------------------------------------ clouds
def lattice_cloud(seed=0, n=400, side=5, K=9):
    """points with small integer coordinates, many of them repeated, and centres that are lattice points too (two of them equal): ties
    occur, and every distance is an exact fp32 integer.  -> (points (n,3) fp32, centres (K,3) fp32)"""
    rng = np.random.RandomState(seed)
    p = rng.randint(-side, side + 1, size=(n, 3)).astype(np.float32)
    p[n // 2:n // 2 + 20] = p[:20]                                # exact duplicates
    c = rng.randint(-side, side + 1, size=(K, 3)).astype(np.float32)
    c[K - 1] = c[1]                                               # a duplicated centre: it stays empty
    return p, c


def random_cloud(N, seed, n_blobs=5):
    rng = np.random.RandomState(seed)
    centres = rng.uniform(-2, 2, size=(n_blobs, 3))
    which = rng.randint(0, n_blobs, size=N)
    return (centres[which] + rng.randn(N, 3) * rng.uniform(0.05, 0.4, size=(n_blobs, 1))[which]).astype(np.float32)


def ulp_diff(a, b):
    """the distance of two fp32 arrays in units in the last place (of finite numbers of the same sign, or zero)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def check_eigen(C, evals, axes, tag=''):
    """what a decomposition (evals (3,), axes (3,3) rows) of the symmetric C (6,) must satisfy"""
    A = np.array([[C[0], C[1], C[2]], [C[1], C[3], C[4]], [C[2], C[4], C[5]]])
    nrm = np.linalg.norm(A)
    tol = 64 * EPS64
    for i in range(3):
        assert np.linalg.norm(A @ axes[i] - evals[i] * axes[i]) <= tol * nrm, (tag, i)
    assert np.abs(axes @ axes.T - np.eye(3)).max() <= tol, tag
    assert abs(np.linalg.det(axes) - 1) <= tol, tag
    assert evals[0] >= evals[1] >= evals[2], tag
    assert np.abs(evals - np.linalg.eigvalsh(A)[::-1]).max() <= tol * nrm, tag
    for i in range(2):
        m = int(np.abs(axes[i]).argmax())                         # argmax: the lowest index of equal ones
        assert axes[i][m] > 0, (tag, i)
    assert np.abs(axes[2] - np.cross(axes[0], axes[1])).max() <= tol, tag


# ------------------------------------------------------------------------------------------------ three boxes
BOX_M = (8, 7, 6)                                                 # grid points per edge: 512, 343 and 216 points, so the order by count is known
BOX_CENTRES = np.array([[-0.9, -0.2, 0.3], [0.8, 0.1, -0.6], [0.1, 0.5, 0.9]])
BOX_HALF = np.array([[0.21, 0.13, 0.08], [0.18, 0.11, 0.075], [0.16, 0.10, 0.07]])       # (all above the smallest block size, 0.075)
BOX_WORLD = dict(S_world=0.7, R_world=(-100.0, 25.0, 10.0), T_world=(0.3, -0.2, 1.1))      # (elev, azim, roll) of mesh.world_rotation
OUTLIERS = np.array([[1.9, 2.9, 1.9], [-1.9, 2.9, -1.9], [1.9, 2.8, -1.9]])              # inside the bound of blocks_from_points, far from every box


def _proper(rng):
    Q, _ = np.linalg.qr(rng.randn(3, 3))
    if np.linalg.det(Q) < 0:
        Q[:, 0] *= -1
    return Q


def three_boxes(n_outliers=0, seed=0):
    """Three solid boxes in the scene frame of a model (T_range (1,1,1): the ground is y = -0.9), each a regular m x m x m grid of points with
    centre BOX_CENTRES[b], axes the rows of rot[b] and half-extents BOX_HALF[b]; shuffled; n_outliers stray points appended.  The variance of a
    regular grid of m points over [-a, a] is a^2 / 3 * (m + 1) / (m - 1).  The boxes are further apart than a box diagonal.
    -> dict(points (N,3) fp32 in the frame of the cameras, scene (N,3) fp64 in the scene frame, box (N,) the box of each point (-1: stray),
    rot (3,3,3), lam (3,3) the analytic eigenvalues, matrix (3,3) R_world)"""
    from dbw_amd import mesh
    rng = np.random.RandomState(seed)
    rot = np.stack([_proper(rng) for _ in range(3)])
    pts, box = [], []
    for b, m in enumerate(BOX_M):
        g = np.linspace(-1, 1, m)
        grid = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3) * BOX_HALF[b]
        pts.append(grid @ rot[b] + BOX_CENTRES[b])
        box.append(np.full(len(grid), b))
    scene, box = np.concatenate(pts), np.concatenate(box)
    perm = rng.permutation(len(scene))
    scene, box = scene[perm], box[perm]
    if n_outliers:
        scene, box = np.concatenate([scene, OUTLIERS[:n_outliers]]), np.concatenate([box, np.full(n_outliers, -1)])
    Rw = mesh.world_rotation(*BOX_WORLD['R_world']).double().numpy()
    world = (scene * BOX_WORLD['S_world']) @ Rw + np.array(BOX_WORLD['T_world'])
    lam = np.stack([BOX_HALF[b] ** 2 / 3 * (m + 1) / (m - 1) for b, m in enumerate(BOX_M)])
    diag = 2 * np.linalg.norm(BOX_HALF, axis=1).max()
    gaps = [np.linalg.norm(BOX_CENTRES[a] - BOX_CENTRES[b]) for a in range(3) for b in range(a)]
    assert min(gaps) - diag > diag                                # the nearest points of two boxes are more than a box diagonal apart
    return dict(points=world.astype(np.float32), scene=scene, box=box, rot=rot, lam=lam, matrix=Rw)


def scene_rounding(points):
    """What a coordinate of the scene frame may differ by when it is computed in fp32 from the fp32 points: the points are rounded once, and
    (p - T_world) @ R_world^T / S_world is a dozen fp32 operations on numbers no larger than |p| + |T_world| -> 16 eps32 of that, over S_world"""
    return 16 * 2.0 ** -24 * (np.abs(points).max() + np.abs(BOX_WORLD['T_world']).max()) / BOX_WORLD['S_world']
