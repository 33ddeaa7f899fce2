"""Checker side of the plane RANSAC: the host build of csrc/plane_math.h (tests/host_plane_math.cpp through host_build.host_lib) behind
numpy arguments, for tests/test_host_plane_math.py and tests/test_gpu_worldfit.py, and the golden fixture of the reference's own Ransac."""
import ctypes
import os

import numpy as np

import host_build

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ransac_plane.npz')
ORTHOGONAL, VERTICAL = 0, 1
MIN_SHAPE, EDGE = 0.05, 1e-3          # tests/golden/make_golden_plane.py: which hypotheses are compared, what "at the threshold" means


def lib():
    L = host_build.host_lib('plane_math')
    L.host_plane_count.restype = ctypes.c_int64
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _f32(a, shape=None):
    if a is None:
        return None
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    return a if shape is None else a.reshape(shape)


def host_fit(points, H, mode, thresh2, seed=0, triples=None, up=None, cos_tilt=0.0, cams=None, tau=0.0, min_cams=0, refine=0):
    """host_plane_fit: the stages of dbw_eval_plane_fit as plain loops -> dict(rc, plane (4,) fp64, info (4,), counts (H,), triples (H,3), mask (N,))"""
    pts = _f32(points, (-1, 3))
    N = len(pts)
    tri = None if triples is None else np.ascontiguousarray(np.asarray(triples, dtype=np.int32).reshape(-1, 3))
    up, cams = _f32(up), _f32(cams, (-1, 3))
    out = dict(plane=np.zeros(4), info=np.zeros(4, np.int32), counts=np.zeros(H, np.int32), triples=np.zeros((H, 3), np.int32), mask=np.zeros(N, np.uint8))
    out['rc'] = lib().host_plane_fit(_ptr(pts), ctypes.c_int64(N), int(H), int(mode), ctypes.c_float(thresh2), ctypes.c_uint64(seed), _ptr(tri), _ptr(up),
                                     ctypes.c_float(cos_tilt), _ptr(cams), 0 if cams is None else len(cams), ctypes.c_float(tau), int(min_cams), int(refine),
                                     _ptr(out['plane']), _ptr(out['info']), _ptr(out['counts']), _ptr(out['triples']), _ptr(out['mask']))
    return out


def from_triple(a, b, c, mode, up=None):
    out = np.zeros(4, np.float32)
    ok = lib().host_plane_from_triple(_ptr(_f32(a)), _ptr(_f32(b)), _ptr(_f32(c)), int(mode), _ptr(_f32(up)), _ptr(out))
    return bool(ok), out


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden_restated(g):
    """fp64 per hypothesis of the fixture: (number of points within EDGE * thresh of the threshold, triangle shape |m.z| / (|e1||e2|))"""
    p, thresh = g['points'].astype(np.float64), float(g['thresh'])
    edge, shape = [], []
    for t in g['triples']:
        a, b, c = p[t]
        m = np.cross(b - a, c - a)
        shape.append(abs(m[2]) / max(np.linalg.norm(b - a) * np.linalg.norm(c - a), 1e-300))
        if m[2] == 0:
            edge.append(0)
            continue
        n = m / m[2]
        r2 = (p @ n - n @ a) ** 2
        edge.append(int((np.abs(r2 - thresh) < EDGE * thresh).sum()))
    return np.array(edge), np.array(shape)


def check_golden(g, counts, best, best_count):
    """the conditions a VERTICAL fit on the fixture's triples is held to"""
    edge, shape = golden_restated(g)
    ok = shape > MIN_SHAPE
    assert ok.sum() >= 90
    diff = np.abs(counts.astype(np.int64) - g['counts'])
    print('golden: compared', int(ok.sum()), 'differ', int((diff[ok] > 0).sum()), 'max diff', int(diff[ok].max()), 'allowed max', int(edge[ok].max()))
    assert (counts[ok] >= 0).all() and (diff[ok] <= edge[ok]).all()
    assert best == int(g['best']) and best_count == int(g['best_n'])
