"""Checker side of the surface term: a numpy float64 reference written from the definition, independent of
csrc/surface_math.h -- the closest point on a triangle by the region classification of Ericson (Real-Time Collision Detection, 5.1.5: the
Voronoi regions of the three vertices, the three edges and the interior), where the header projects onto the plane and falls back to the
sides -- the draw restated on Python integers, the scenes of the tests, and the ctypes side of tests/host_surface.cpp.

Unit of error: the element-wise bar of tests/render_ref64.py,  bars(a, b) = max_i |a_i - b_i| / (1e-4 |b_i| + 1e-6 max|b|),  b the float64
result; a result passes at <= 1 bar."""
import ctypes

import numpy as np

BNV, BNF = 42, 80                       # vertices / faces of a block (icosphere level 1)
MARGIN = 1e-5                           # relative d2 margin below which a point is left out of a gradient comparison


def bars(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    if b.size == 0:
        return 0.0
    tol = 1e-4 * np.abs(b) + 1e-6 * np.abs(b).max()
    tol = np.where(tol > 0, tol, 1e-300)
    return float((np.abs(a - b) / tol).max())


# ---------------------------------------------------------------------------------------------------------------- closest point, fp64
def _dot(a, b):
    return (a * b).sum(-1)


def _segment(p, s0, s1):
    d = s1 - s0
    dd = _dot(d, d)
    t = np.where(dd > 0, _dot(p - s0, d) / np.where(dd > 0, dd, 1.0), 0.0).clip(0.0, 1.0)
    return t


def closest_on_triangles(p, a, b, c):
    """p, a, b, c (..., 3) float64, broadcast against each other -> (d2 (...), bary (..., 3)) of the closest point of every triangle."""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(x, np.float64) for x in (p, a, b, c)))
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = p - b
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = p - c
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    one, zero = np.ones_like(d1), np.zeros_like(d1)

    def safe(n, d):
        return n / np.where(d != 0, d, 1.0)

    v_ab, w_ac, w_bc = safe(d1, d1 - d3), safe(d2, d2 - d6), safe(d4 - d3, (d4 - d3) + (d5 - d6))
    den = va + vb + vc
    v_in, w_in = safe(vb, den), safe(vc, den)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
    bary_v = np.select(conds, [zero, one, v_ab, zero, zero, 1.0 - w_bc], v_in)
    bary_w = np.select(conds, [zero, zero, zero, one, w_ac, w_bc], w_in)
    # a face without area has no interior: the nearest of its three sides (Ericson's interior formula would divide by zero)
    n = np.cross(ab, ac)
    flat = _dot(n, n) <= 1e-24 * np.maximum(_dot(ab, ab), _dot(ac, ac)) ** 2
    if flat.any():
        cand = []
        for (s0, s1, bw) in ((a, b, lambda t: (t, 0 * t)), (b, c, lambda t: (1 - t, t)), (c, a, lambda t: (0 * t, 1 - t))):
            t = _segment(p, s0, s1)
            q = s0 + t[..., None] * (s1 - s0)
            cand.append((_dot(p - q, p - q),) + bw(t))
        best = np.argmin(np.stack([x[0] for x in cand]), 0)
        fv = np.choose(best, [x[1] for x in cand])
        fw = np.choose(best, [x[2] for x in cand])
        bary_v, bary_w = np.where(flat, fv, bary_v), np.where(flat, fw, bary_w)
    bary = np.stack([1.0 - bary_v - bary_w, bary_v, bary_w], -1)
    q = bary[..., 0:1] * a + bary[..., 1:2] * b + bary[..., 2:3] * c
    return _dot(p - q, p - q), bary


def nearest_on_surface(points, verts, faces, face_keep=None, chunk=256):
    """-> dict: d2 (n), face (n), bary (n,3), c (n,3) of the closest point of the kept faces, and d2_second (n): the smallest d2 among the faces
    whose closest point is a DIFFERENT point (inf without one)."""
    P, Vt = np.asarray(points, np.float64), np.asarray(verts, np.float64)
    Fc = np.asarray(faces, np.int64)
    ids = np.arange(len(Fc)) if face_keep is None else np.nonzero(np.asarray(face_keep))[0]
    tri = Vt[Fc[ids]]
    scale = max(1.0, float(np.abs(Vt).max()))
    out = {k: [] for k in ('d2', 'face', 'bary', 'c', 'd2_second')}
    for s in range(0, len(P), chunk):
        p = P[s:s + chunk, None, :]
        d2, bary = closest_on_triangles(p, tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
        c = (bary[..., None] * tri[None]).sum(-2)
        j = d2.argmin(1)
        r = np.arange(len(j))
        cb = c[r, j]
        other = np.abs(c - cb[:, None]).max(-1) > 1e-9 * scale
        out['d2'].append(d2[r, j]); out['face'].append(ids[j]); out['bary'].append(bary[r, j]); out['c'].append(cb)
        out['d2_second'].append(np.where(other, d2, np.inf).min(1))
    return {k: np.concatenate(v) for k, v in out.items()}


def kept_for_gradients(near, tau):
    """The points whose gradient the fp32 kernels and the fp64 reference must agree on: best and second-best distinct closest points apart
    by MARGIN in d2, relatively, and d2 not within MARGIN of tau^2."""
    d2, t2 = near['d2'], tau * tau
    tie = (near['d2_second'] - d2) < MARGIN * np.maximum(near['d2_second'], 1e-300)
    return ~tie & ~(np.abs(d2 - t2) < MARGIN * t2)


def term_value(points, verts, faces, face_keep, tau, cloud=None, vert_alpha=None, vert_group=None, back=0.0, back_count=1.0):
    """(forward mean, back mean) of the definition, float64."""
    near = nearest_on_surface(points, verts, faces, face_keep)
    fwd = np.minimum(near['d2'], tau * tau).mean()
    bk = 0.0
    if back > 0:
        C, Vt = np.asarray(cloud, np.float64), np.asarray(verts, np.float64)
        g = np.asarray(vert_group)
        sel = np.nonzero(g >= 0)[0]
        d2 = ((Vt[sel, None, :] - C[None]) ** 2).sum(-1).min(1)
        bk = float((np.asarray(vert_alpha, np.float64)[g[sel]] * np.minimum(d2, tau * tau)).sum() / back_count)
    return float(fwd), bk


# ---------------------------------------------------------------------------------------------------------------- the draw, on Python integers
def _philox(ctr, key):
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k[0]) & 0xffffffff, p1 & 0xffffffff, ((p0 >> 32) ^ c[3] ^ k[1]) & 0xffffffff, p0 & 0xffffffff]
        k = [(k[0] + 0x9E3779B9) & 0xffffffff, (k[1] + 0xBB67AE85) & 0xffffffff]
    return c


def draw_index(seed, step, i, n_cloud):
    """Draw i of a step: word 0 of Philox4x32-10 with counter (i, 2, step lo, step hi) and key (seed lo, seed hi), mod the cloud's size."""
    return _philox([i, 2, step & 0xffffffff, step >> 32], [seed & 0xffffffff, seed >> 32])[0] % n_cloud


def draw_indices(seed, step, m, n_cloud):
    return np.array([draw_index(seed, step, i, n_cloud) for i in range(m)], np.int64)


# ---------------------------------------------------------------------------------------------------------------- scenes
def _icosphere1():
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
                  [-t, 0, -1], [-t, 0, 1]], np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts, cache, out = [x for x in v], {}, []

    def mid(i, j):
        key = (min(i, j), max(i, j))
        if key not in cache:
            m = verts[i] + verts[j]
            verts.append(m / np.linalg.norm(m))
            cache[key] = len(verts) - 1
        return cache[key]

    for (a, b, c) in f:
        ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
        out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    return np.array(verts), np.array(out, np.int64)


def scene(n_blocks=3, ground=True, seed=0, drop=None, degenerate=False):
    """Convex, well-separated blocks (ellipsoids on an icosphere of 42 vertices, 80 faces) over a ground of 8 faces: ->
    dict of verts (V,3) f32, faces (F,3) i32, face_group (G+1) i32, group_keep (G) i32 or None, vert_group (V) i32 (block index, -1 ground),
    n_blocks.  drop: a block that group_keep leaves out.  degenerate: face 1 of block 0 gets a repeated vertex (a zero-area face)."""
    rng = np.random.default_rng(seed)
    sv, sf = _icosphere1()
    assert sv.shape == (BNV, 3) and sf.shape == (BNF, 3)
    verts, faces, fg, vg = [], [], [0], []
    if ground:
        g = np.array([[x, -0.6, z] for z in (-2.0, 0.0, 2.0) for x in (-2.0, 0.0, 2.0)], np.float64)
        gf = []
        for r in range(2):
            for q in range(2):
                i = r * 3 + q
                gf += [(i, i + 3, i + 1), (i + 1, i + 3, i + 4)]
        verts.append(g); faces.append(np.array(gf, np.int64)); fg.append(len(gf)); vg += [-1] * len(g)
    off = sum(len(v) for v in verts)
    for k in range(n_blocks):
        radii = rng.uniform(0.15, 0.3, 3)
        centre = np.array([-0.8 + 0.8 * k, 0.05 * k, 0.1 * (k % 2)])
        verts.append(sv * radii + centre)
        f = sf + off
        if degenerate and k == 0:
            f = f.copy()
            f[1, 2] = f[1, 1]
        faces.append(f); fg.append(fg[-1] + BNF); vg += [k] * BNV
        off += BNV
    keep = None
    if drop is not None:
        keep = np.ones(len(fg) - 1, np.int32)
        keep[drop + (1 if ground else 0)] = 0
    return dict(verts=np.concatenate(verts).astype(np.float32), faces=np.concatenate(faces).astype(np.int32), face_group=np.array(fg, np.int32),
                group_keep=keep, vert_group=np.array(vg, np.int32), n_blocks=n_blocks)


def face_keep_of(sc):
    fg, keep = sc['face_group'], sc['group_keep']
    m = np.ones(len(sc['faces']), bool)
    if keep is not None:
        for g in range(len(keep)):
            if not keep[g]:
                m[fg[g]:fg[g + 1]] = False
    return m


def cloud_near(sc, n, seed=1, noise=0.02):
    """n points near the kept blocks' surfaces (vertices blown up a little and jittered), a few on the ground, one far beyond any tau and
    one exactly on the surface (a vertex)."""
    rng = np.random.default_rng(seed)
    v, g = sc['verts'].astype(np.float64), sc['vert_group']
    blk = np.nonzero(g >= 0)[0]
    if len(blk) == 0:
        blk = np.arange(len(v))
    pick = blk[rng.integers(0, len(blk), n)]
    w = rng.dirichlet(np.ones(3), n)
    tri = v[sc['faces'][rng.integers(0, len(sc['faces']), n)].astype(np.int64)]
    p = np.where(rng.random(n)[:, None] < 0.5, v[pick] + rng.normal(0, noise, (n, 3)), (w[:, :, None] * tri).sum(1) + rng.normal(0, noise, (n, 3)))
    p = p.astype(np.float32)
    if n >= 3:
        p[1] = (50.0, 40.0, -30.0)
        p[2] = sc['verts'][int(blk[0])]
    return p


# ---------------------------------------------------------------------------------------------------------------- the host build
def host():
    from host_build import host_lib
    L = host_lib('surface')
    L.host_surface_draw_index.restype = ctypes.c_uint32
    L.host_surface_draw_index.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32]
    L.host_surface_key.restype = ctypes.c_uint64
    L.host_surface_key.argtypes = [ctypes.c_float, ctypes.c_uint32]
    L.host_surface_rho.restype = ctypes.c_float
    L.host_surface_rho.argtypes = [ctypes.c_float, ctypes.c_float]
    return L


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_closest(tri, p):
    tri, p = np.ascontiguousarray(tri, np.float32).reshape(-1, 9), np.ascontiguousarray(p, np.float32).reshape(-1, 3)
    out = np.empty((len(p), 3), np.float32)
    host().host_surface_closest(_ptr(tri), _ptr(p), ctypes.c_int64(len(p)), _ptr(out))
    return out


def host_box_bound(lo, hi, p):
    lo, hi, p = (np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in (lo, hi, p))
    out = np.empty(len(p), np.float32)
    host().host_surface_box_bound(_ptr(lo), _ptr(hi), _ptr(p), ctypes.c_int64(len(p)), _ptr(out))
    return out


def host_records(points, sc, n_points, seed, step, tau, cull):
    """-> (records (M,4) uint32: d2 bits, face, u bits, v bits; rho (M) f32)"""
    P = np.ascontiguousarray(points, np.float32)
    M = n_points or len(P)
    rec, rho = np.empty((M, 4), np.uint32), np.empty(M, np.float32)
    keep = sc['group_keep']
    host().host_surface_records(_ptr(P), ctypes.c_int64(len(P)), ctypes.c_int64(n_points), ctypes.c_uint64(seed), ctypes.c_uint64(step),
                                _ptr(sc['verts']), ctypes.c_int(len(sc['verts'])), _ptr(sc['faces']), ctypes.c_int(len(sc['faces'])),
                                _ptr(sc['face_group']), _ptr(keep) if keep is not None else None, ctypes.c_int(len(sc['face_group']) - 1),
                                ctypes.c_float(tau), ctypes.c_int(cull), _ptr(rec), _ptr(rho))
    return rec, rho
