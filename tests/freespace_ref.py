"""Checker side of the free-space term: a numpy float64 restatement of the definition, independent of csrc/freespace_math.h
-- the intersection as the plane's t = n . (a - o) / (n . e) with the barycentrics of the hit point solved from the Gram matrix of
(e1, e2), where the header runs Moeller-Trumbore on scalar triple products --, the rays set aside from a gradient comparison, the scenes
and rays of the tests, and the ctypes side of tests/host_freespace.cpp.

Unit of error: the project's element-wise bar (surface_ref.bars), |a - b| / (1e-4 |b| + 1e-6 max|b|), b the float64 result; <= 1 passes.

Rays set aside.  A first hit next to a shared edge, a grazing face or a threshold can pick another face in fp32 than in fp64, and the
gradient then differs.  flagged() marks a ray, from the float64 numbers alone, when
  * a face has min(u, v, 1 - u - v) within EDGE of 0 at a t in (-EDGE, 1 + EDGE), or
  * a face that the ray's line meets inside the triangle widened by EDGE (u, v >= -EDGE, u + v <= 1 + EDGE) at such a t has det^2 within a
    factor 2 of the graze threshold -- the threshold only decides anything for a face that the ray would otherwise hit; a face that is
    missed by a wide margin is no candidate on either side of it --, or
  * g is within G_EDGE of 0 or of tau.
Flagged rays leave the gradient comparison, never the byte comparison with the host build."""
import ctypes

import numpy as np

import surface_ref as SR
from surface_ref import BNF, BNV, bars, face_keep_of  # noqa: F401  (the tests' one import)

GRAZE = 2.0 ** -16
EDGE, G_EDGE, FLAG_CAP = 1e-3, 1e-4, 0.02


def _dot(a, b):
    return (a * b).sum(-1)


# ---------------------------------------------------------------------------------------------------------------- intersection, fp64
def intersect(o, e, a, b, c):
    """o, e, a, b, c (..., 3) float64, broadcast against each other -> dict of t, u, v, det2, thr (the graze threshold of det2) and cand,
    the definition's candidate test.  A face whose plane the ray is parallel to has t = u = v = nan and is no candidate."""
    o, e, a, b, c = np.broadcast_arrays(*(np.asarray(x, np.float64) for x in (o, e, a, b, c)))
    e1, e2 = b - a, c - a
    n = np.cross(e1, e2)
    ne = _dot(n, e)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(ne != 0, _dot(n, a - o) / np.where(ne != 0, ne, 1.0), np.nan)
        x = o + t[..., None] * e - a                            # the hit point, relative to a
        g11, g12, g22 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2)
        den = g11 * g22 - g12 * g12
        r1, r2 = _dot(x, e1), _dot(x, e2)
        den = np.where(den > 0, den, np.nan)
        u, v = (g22 * r1 - g12 * r2) / den, (g11 * r2 - g12 * r1) / den
    det2, thr = ne * ne, GRAZE * _dot(n, n) * _dot(e, e)
    with np.errstate(invalid='ignore'):
        cand = (det2 > thr) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < 1)
    return dict(t=t, u=u, v=v, det2=det2, thr=thr, cand=cand)


def rays_of(ends, frame, origins):
    """-> (o (n,3), e (n,3)) float64; a ray with a frame outside the table gets e = 0 (no hit)."""
    P, fr, O = np.asarray(ends, np.float64), np.asarray(frame), np.asarray(origins, np.float64)
    ok = (fr >= 0) & (fr < len(O))
    o = np.where(ok[:, None], O[np.where(ok, fr, 0)], P)
    return o, P - o


def first_hits(ends, frame, origins, verts, faces, face_keep=None, tau=0.1, margin=0.02, chunk=256):
    """-> dict: t (n; nan without a hit), face (n; -1), u, v, g, psi, and flagged (n) bool, all from float64."""
    o_all, e_all = rays_of(ends, frame, origins)
    Vt, Fc = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    ids = np.arange(len(Fc)) if face_keep is None else np.nonzero(np.asarray(face_keep))[0]
    tri = Vt[Fc[ids]]
    out = {k: [] for k in ('t', 'face', 'u', 'v', 'flagged')}
    for s in range(0, len(o_all), chunk):
        o, e = o_all[s:s + chunk, None, :], e_all[s:s + chunk, None, :]
        r = intersect(o, e, tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
        t = np.where(r['cand'], r['t'], np.inf)
        j = t.argmin(1)                                         # (the first of equal t: the lowest face)
        rows = np.arange(len(j))
        hit = r['cand'].any(1)
        with np.errstate(invalid='ignore'):
            near_t = (r['t'] > -EDGE) & (r['t'] < 1 + EDGE)
            w = np.minimum(np.minimum(r['u'], r['v']), 1 - r['u'] - r['v'])
            edge = near_t & (np.abs(w) <= EDGE)
            # The graze flag, read for the faces the ray would otherwise hit (w >= -EDGE).  The issue's wording is "a face's det^2 is
            # within a factor 2 of the graze threshold", any face: taken literally that is sin of the ray-plane angle in (0.0028, 0.0055)
            # for ANY of a mesh's faces, which 24 % to 26 % of the rays meet on the 248 faces of the fixtures, against a cap of 2 %.  The
            # threshold decides nothing for a face the ray misses by a wide margin, so the narrower reading sets aside every ray whose
            # first hit the threshold can change and keeps more rays in the comparison (a stricter test, not a looser one).
            graze = near_t & (w >= -EDGE) & (r['det2'] > 0.5 * r['thr']) & (r['det2'] < 2.0 * r['thr'])
        out['t'].append(np.where(hit, t[rows, j], np.nan)); out['face'].append(np.where(hit, ids[j], -1))
        out['u'].append(np.where(hit, r['u'][rows, j], 0.0)); out['v'].append(np.where(hit, r['v'][rows, j], 0.0))
        out['flagged'].append(edge.any(1) | graze.any(1))
    res = {k: np.concatenate(v) for k, v in out.items()}
    l = np.linalg.norm(e_all, axis=1)
    g = np.where(res['face'] >= 0, (1 - np.nan_to_num(res['t'])) * l - margin, -np.inf)
    res['g'], res['psi'] = g, psi(g, tau)
    res['flagged'] = res['flagged'] | (np.abs(g) <= G_EDGE) | (np.abs(g - tau) <= G_EDGE)
    return res


def psi(g, tau):
    g = np.asarray(g, np.float64)
    with np.errstate(invalid='ignore'):
        return np.where(g <= 0, 0.0, np.where(g <= tau, g * g, tau * (2 * g - tau)))


def face_alpha(sc, vert_alpha):
    """the opacity of every face's group (1 for the ground)"""
    fg, ga = sc['face_group'], sc['group_alpha']
    a = np.ones(len(sc['faces']))
    for g in range(len(ga)):
        if ga[g] >= 0:
            a[fg[g]:fg[g + 1]] = vert_alpha[ga[g]]
    return a


def term_value(ends, frame, origins, sc, vert_alpha, tau, margin):
    """(1/M) sum a psi of the definition over the given rays, float64."""
    h = first_hits(ends, frame, origins, sc['verts'], sc['faces'], face_keep_of(sc), tau, margin)
    a = face_alpha(sc, np.asarray(vert_alpha, np.float64))[np.maximum(h['face'], 0)]
    return float((a * h['psi']).sum() / len(h['psi']))


def closed_form_grads(ends, frame, origins, sc, vert_alpha, tau, margin, weight):
    """The gradient as DESIGN.md 6v states it, float64, from first_hits alone: dL/dvert_m = -(w/M) a psi'(g) l wts_m n / (n . e),
    dL/da_k = (w/M) sum psi -> (grad_verts (V,3), grad_alpha (A))."""
    h = first_hits(ends, frame, origins, sc['verts'], sc['faces'], face_keep_of(sc), tau, margin)
    o, e = rays_of(ends, frame, origins)
    Vt, Fc = sc['verts'].astype(np.float64), sc['faces'].astype(np.int64)
    va = np.asarray(vert_alpha, np.float64)
    fa = face_alpha(sc, va)
    gv, ga = np.zeros_like(Vt), np.zeros(len(va))
    M = len(e)
    fgroup = np.repeat(np.arange(len(sc['group_alpha'])), np.diff(sc['face_group']))
    for i in np.nonzero((h['face'] >= 0) & (h['g'] > 0))[0]:
        f = h['face'][i]
        a, b, c = Vt[Fc[f]]
        n = np.cross(b - a, c - a)
        l = np.linalg.norm(e[i])
        wts = (1 - h['u'][i] - h['v'][i], h['u'][i], h['v'][i])
        for m in range(3):
            gv[Fc[f, m]] += -(weight / M) * fa[f] * 2 * min(h['g'][i], tau) * l * wts[m] * n / np.dot(n, e[i])
        row = sc['group_alpha'][fgroup[f]]
        if row >= 0:
            ga[row] += (weight / M) * h['psi'][i]
    return gv, ga


# ---------------------------------------------------------------------------------------------------------------- the draw, on Python integers
def draw_index(seed, step, i, n_rays):
    """Draw i of a step: word 0 of Philox4x32-10 with counter (i, 3, step lo, step hi) and key (seed lo, seed hi), mod the number of rays."""
    return SR._philox([i, 3, step & 0xffffffff, step >> 32], [seed & 0xffffffff, seed >> 32])[0] % n_rays


def draw_indices(seed, step, m, n_rays):
    return np.array([draw_index(seed, step, i, n_rays) for i in range(m)], np.int64)


# ---------------------------------------------------------------------------------------------------------------- scenes and rays
ORIGINS = np.array([[-1.6, 0.9, 2.1], [1.5, 1.1, 1.9], [0.1, 1.7, -2.2], [-0.3, 0.6, 0.9]], np.float32)


def scene(name):
    """The five shapes of the tests -> (sc, origins): sc as surface_ref.scene's, with group_alpha (G) int32 added.  'one_face': a single
    triangle; 'blocks': three ellipsoids and the ground; 'dropped': block 1 left out by group_keep; 'degenerate': one face of block 0 has a
    repeated vertex; 'inside': as 'blocks', with a fifth origin at the centre of block 2."""
    if name == 'one_face':
        sc = dict(verts=np.array([[-0.4, -0.1, 0.1], [0.5, 0.0, -0.1], [0.0, 0.6, 0.2]], np.float32), faces=np.array([[0, 1, 2]], np.int32),
                  face_group=np.array([0, 1], np.int32), group_keep=None, vert_group=np.zeros(3, np.int32), n_blocks=1,
                  group_alpha=np.array([0], np.int32))
        return sc, ORIGINS
    sc = SR.scene(3, ground=True, seed=4, drop=1 if name == 'dropped' else None, degenerate=name == 'degenerate')
    sc['group_alpha'] = np.array([-1, 0, 1, 2], np.int32)
    origins = ORIGINS
    if name == 'inside':
        centre = sc['verts'][sc['vert_group'] == 2].astype(np.float64).mean(0)
        origins = np.concatenate([ORIGINS, centre[None].astype(np.float32)])
    return sc, origins


def rays_through(sc, origins, n, seed=1):
    """n rays: ends scattered about the ground's height under and around the blocks (so that many rays pass through a block on their way,
    some end above the ground and some a little below it), a few ends inside or short of a block, one ray with a frame outside the table
    and one of zero length."""
    rng = np.random.default_rng(seed)
    nf = len(origins)
    frame = rng.integers(0, nf, n).astype(np.int32)
    if len(sc['verts']) == 3:                                   # the one face: ends behind it, as seen from the origins
        w = rng.dirichlet(np.ones(3), n)
        on = (w[:, :, None] * sc['verts'].astype(np.float64)[None]).sum(1) + rng.normal(0, 0.25, (n, 3))
        behind = np.where(rng.random((n, 1)) < 0.5, rng.uniform(0.0, 0.06, (n, 1)), rng.uniform(0.0, 0.8, (n, 1)))      # half of them within tau or so
        ends = on + behind * (on - origins.astype(np.float64)[frame])
    else:
        ends = np.stack([rng.uniform(-1.6, 1.6, n), -0.6 + rng.normal(0, 0.08, n), rng.uniform(-1.0, 1.2, n)], 1)
        k = n // 8
        blk = sc['verts'].astype(np.float64)[sc['vert_group'] >= 0]
        ends[:k] = blk[rng.integers(0, len(blk), k)] * rng.uniform(0.7, 1.3, (k, 1))
    ends = ends.astype(np.float32)
    if n >= 4:
        frame[1] = nf + 3
        ends[3] = origins[frame[3]]
    return ends, frame


# ---------------------------------------------------------------------------------------------------------------- the host build
def host():
    from host_build import host_lib
    L = host_lib('freespace')
    L.host_freespace_draw_index.restype = ctypes.c_uint32
    L.host_freespace_draw_index.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32]
    L.host_freespace_key.restype = ctypes.c_uint64
    L.host_freespace_key.argtypes = [ctypes.c_float, ctypes.c_uint32]
    L.host_freespace_psi.restype = ctypes.c_float
    L.host_freespace_psi.argtypes = [ctypes.c_float, ctypes.c_float]
    L.host_freespace_g.restype = ctypes.c_float
    L.host_freespace_g.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]
    L.host_freespace_graze.restype = ctypes.c_float
    return L


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_hit(tri, o, e):
    """-> (n,4) float32: hit, t, u, v"""
    tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 9)
    o, e = (np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in (o, e))
    out = np.empty((len(o), 4), np.float32)
    host().host_freespace_hit(_ptr(tri), _ptr(o), _ptr(e), ctypes.c_int64(len(o)), _ptr(out))
    return out


def host_slab(lo, hi, o, e, t_max):
    lo, hi, o, e = (np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in (lo, hi, o, e))
    t_max = np.ascontiguousarray(t_max, np.float32)
    out = np.empty(len(o), np.int32)
    host().host_freespace_slab(_ptr(lo), _ptr(hi), _ptr(o), _ptr(e), _ptr(t_max), ctypes.c_int64(len(o)), _ptr(out))
    return out.astype(bool)


def host_records(ends, frame, origins, sc, n_rays, seed, step, tau, margin, cull):
    """-> (records (M,4) uint32: t bits, face, u bits, v bits; psi (M) f32)"""
    P, fr, O = np.ascontiguousarray(ends, np.float32), np.ascontiguousarray(frame, np.int32), np.ascontiguousarray(origins, np.float32)
    M = n_rays or len(P)
    rec, ps = np.empty((M, 4), np.uint32), np.empty(M, np.float32)
    keep = sc['group_keep']
    host().host_freespace_records(_ptr(P), _ptr(fr), _ptr(O), ctypes.c_int64(len(P)), ctypes.c_int(len(O)), ctypes.c_int64(n_rays),
                                  ctypes.c_uint64(seed), ctypes.c_uint64(step), _ptr(sc['verts']), _ptr(sc['faces']), _ptr(sc['face_group']),
                                  _ptr(keep) if keep is not None else None, ctypes.c_int(len(sc['face_group']) - 1), ctypes.c_float(tau),
                                  ctypes.c_float(margin), ctypes.c_int(cull), _ptr(rec), _ptr(ps))
    return rec, ps


def host_depth_rays(depth, cams, target, poses, d_min=1, d_max=65535, stride=1, permille=0, box=None, G=1):
    """dbw_lens_depth_rays through the host build (tests/host_depth_rays.cpp) -> records (N,Hs,Ws,4) uint32 [px, py, pz bits, frame]; with
    a cube `box` ([lo, lo, lo, inv_step] fp32) of G cells also depth_sample's cell (N,Hs,Ws) int32 of the same pixels."""
    from host_build import host_lib
    depth = np.ascontiguousarray(depth, np.uint16)
    N, H, W = depth.shape
    cams, target = np.ascontiguousarray(cams, np.float32), np.ascontiguousarray(target, np.float32)
    poses = np.ascontiguousarray(poses, np.float32).reshape(N, 12)
    Hs, Ws = -(-H // stride), -(-W // stride)
    rays = np.empty((N, Hs, Ws, 4), np.uint32)
    cell = np.empty((N, Hs, Ws), np.int32) if box is not None else None
    bx = np.ascontiguousarray(box, np.float32) if box is not None else None
    host_lib('depth_rays').host_depth_rays(_ptr(depth), N, H, W, _ptr(cams), _ptr(target), _ptr(poses), int(d_min), int(d_max), int(stride),
                                           int(permille), _ptr(rays), _ptr(bx) if bx is not None else None, int(G),
                                           _ptr(cell) if cell is not None else None)
    return rays if box is None else (rays, cell)
