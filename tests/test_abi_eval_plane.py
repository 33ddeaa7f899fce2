"""CPU: the plane RANSAC entry points added to include/dbw_eval.h under its revision 1 -- the prototypes against the ctypes binding one
argument at a time, the exported symbols, and _lib.family('eval') on a library that has the family but not these functions."""
import ctypes
import re
import types

import pytest

import abi_header as AH
from dbw_amd import _lib

NEW = {'dbw_eval_plane_fit': 'int', 'dbw_eval_plane_workspace_bytes': 'size_t'}
SCALARS = {'int': ctypes.c_int, 'float': ctypes.c_float, 'int64_t': ctypes.c_int64, 'dbw_stream_t': ctypes.c_void_p}
OTHER_WORDS = ('viz', 'render_lit', 'vertex_normals', 'export', 'frames', 'resample', 'ingest', 'lens', 'undistort', 'monitor', 'meter', 'scores', 'icp')


def _declared(name):
    """[(type as written, argument name)] of the prototype of `name` in include/dbw_eval.h"""
    src = re.sub(r'/\*.*?\*/', '', AH.text('dbw_eval.h'), flags=re.S)
    ret, args = re.search(r'\b(\w+)\s+%s\s*\(([^;]*?)\)\s*;' % name, src, flags=re.S).groups()
    out = []
    for a in ' '.join(args.split()).split(','):
        m = re.fullmatch(r'\s*(.*?)(\w+)\s*', a)
        out.append((m.group(1).strip(), m.group(2)))
    return ret, out


def test_prototypes_match_the_binding_argument_by_argument():
    ret, args = _declared('dbw_eval_plane_fit')
    assert ret == 'int'
    assert [n for _, n in args] == ['points', 'N', 'H', 'mode', 'thresh2', 'seed', 'triples', 'up', 'cos_tilt', 'cams', 'M', 'tau', 'min_cams', 'refine',
                                    'workspace', 'plane', 'info', 'counts', 'triples_out', 'mask', 'stream']
    pointers = {'points': 'const float *', 'triples': 'const int32_t *', 'up': 'const float *', 'cams': 'const float *', 'workspace': 'void *',
                'plane': 'double *', 'info': 'int32_t *', 'counts': 'int32_t *', 'triples_out': 'int32_t *', 'mask': 'uint8_t *'}
    bound = _lib.EVAL_SIGNATURES['dbw_eval_plane_fit']
    assert len(bound) == len(args)
    for (typ, name), c in zip(args, bound):
        if name in pointers:
            assert typ == pointers[name] and c is ctypes.c_void_p, name
        else:
            assert '*' not in typ and SCALARS[typ] is c, name
    ret, args = _declared('dbw_eval_plane_workspace_bytes')
    assert ret == 'size_t' and [t for t, _ in args] == ['int64_t', 'int']
    assert _lib.EVAL_OTHER_SIGNATURES['dbw_eval_plane_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int])
    assert _lib.FAMILIES['eval'].other_signatures is _lib.EVAL_OTHER_SIGNATURES
    d = AH.defines('dbw_eval.h')
    assert d['DBW_EVAL_ABI_VERSION'] == 1
    assert (d['DBW_EVAL_PLANE_ORTHOGONAL'], d['DBW_EVAL_PLANE_VERTICAL']) == (_lib.EVAL_PLANE_ORTHOGONAL, _lib.EVAL_PLANE_VERTICAL) == (0, 1)


def test_names_and_exports():
    for n in NEW:
        assert 'eval' in n and not any(w in n for w in OTHER_WORDS)
        assert n in AH.exported()
    lib = _lib.family('eval')
    assert lib.dbw_eval_plane_fit.restype is ctypes.c_int and lib.dbw_eval_plane_workspace_bytes.restype is ctypes.c_size_t
    # the size query: refused sizes give 0, accepted ones a multiple of 16 that grows with H
    q = lib.dbw_eval_plane_workspace_bytes
    assert q(2, 8) == 0 and q(1 << 31, 8) == 0 and q(100, 0) == 0 and q(100, 4097) == 0
    assert q(100, 1) % 16 == 0 and 0 < q(100, 1) < q(100, 4096) and q((1 << 31) - 1, 4096) < 1 << 20


def test_family_refuses_a_library_without_the_new_functions(monkeypatch):
    f = _lib.FAMILIES['eval']
    old = {n: (lambda *a: 0) for n in f.signatures if n not in NEW}
    stub = types.SimpleNamespace(dbw_eval_abi_version=lambda: 1, **old)
    monkeypatch.setattr(_lib, '_lib', stub)
    with pytest.raises(RuntimeError, match=r'has the eval family of include/dbw_eval\.h at revision 1 but not .*dbw_eval_plane_fit.*rebuild it'):
        _lib.family('eval')
    for n in NEW:
        setattr(stub, n, lambda *a: 0)
    assert _lib.family('eval') is stub
