"""CPU: the surface-term entry points added to include/dbw_eval.h under its revision 1 -- the prototypes against the ctypes binding one
argument at a time, the exported symbols, the size query, every refused argument (validated before any launch: no device is needed), and
_lib.family('eval') on a library that has the family but not these functions."""
import ctypes
import re
import types

import numpy as np
import pytest

import abi_header as AH
from dbw_amd import _lib

NEW = {'dbw_eval_surface_fwd': 'int', 'dbw_eval_surface_bwd': 'int', 'dbw_eval_surface_workspace_bytes': 'size_t'}
SCALARS = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'int64_t': ctypes.c_int64, 'dbw_stream_t': ctypes.c_void_p}
OTHER_WORDS = ('viz', 'render_lit', 'vertex_normals', 'export', 'frames', 'resample', 'ingest', 'lens', 'undistort', 'monitor', 'meter', 'scores', 'icp')
FWD = ['points', 'N', 'n_points', 'seed', 'step', 'verts', 'V', 'faces', 'faces_host', 'F', 'face_group', 'group_keep', 'G', 'vert_alpha',
       'vert_group', 'A', 'back_count', 'tau', 'back', 'cull', 'workspace', 'records', 'value', 'stream']
BWD = ['points', 'N', 'n_points', 'seed', 'step', 'verts', 'V', 'faces', 'F', 'G', 'vert_alpha', 'vert_group', 'A', 'back_count', 'tau', 'back',
       'weight', 'grad_out', 'segment', 'records', 'workspace', 'grad_verts', 'grad_alpha', 'stream']
POINTERS = {'points': 'const float *', 'verts': 'const float *', 'faces': 'const int32_t *', 'faces_host': 'const int32_t *',
            'face_group': 'const int32_t *', 'group_keep': 'const int32_t *', 'vert_alpha': 'const float *', 'vert_group': 'const int32_t *',
            'workspace': 'void *', 'value': 'double *', 'grad_out': 'const float *', 'grad_verts': 'float *', 'grad_alpha': 'float *'}
FLOATS = ('back_count', 'tau', 'back', 'weight')


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
    for fn, names, rec_type in (('dbw_eval_surface_fwd', FWD, 'void *'), ('dbw_eval_surface_bwd', BWD, 'const void *')):
        ret, args = _declared(fn)
        assert ret == 'int' and [n for _, n in args] == names
        bound = _lib.EVAL_SIGNATURES[fn]
        assert len(bound) == len(args)
        for (typ, name), c in zip(args, bound):
            if name == 'records':
                assert typ == rec_type and c is ctypes.c_void_p
            elif name in POINTERS:
                assert typ == POINTERS[name] and c is ctypes.c_void_p, name
            else:
                assert '*' not in typ and SCALARS[typ] is c, name
    ret, args = _declared('dbw_eval_surface_workspace_bytes')
    assert ret == 'size_t' and [t for t, _ in args] == ['int64_t', 'int', 'int', 'int', 'int'] and [n for _, n in args] == ['M', 'F', 'V', 'G', 'segment']
    assert _lib.EVAL_OTHER_SIGNATURES['dbw_eval_surface_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int64] + [ctypes.c_int] * 4)
    assert AH.defines('dbw_eval.h')['DBW_EVAL_ABI_VERSION'] == 1
    assert AH.defines('dbw_eval.h')['DBW_EVAL_SURFACE_SEGMENT'] == _lib.EVAL_SURFACE_SEGMENT == 1024


def test_names_exports_and_the_size_query():
    for n in NEW:
        assert 'eval' in n and not any(w in n for w in OTHER_WORDS)
        assert n in AH.exported()
    lib = _lib.family('eval')
    assert lib.dbw_eval_surface_fwd.restype is ctypes.c_int and lib.dbw_eval_surface_bwd.restype is ctypes.c_int
    assert lib.dbw_eval_surface_workspace_bytes.restype is ctypes.c_size_t
    q = lib.dbw_eval_surface_workspace_bytes
    for bad in ((0, 10, 10, 1, 0), ((1 << 24) + 1, 10, 10, 1, 0), (100, 0, 10, 1, 0), (100, (1 << 20) + 1, 10, 1, 0), (100, 10, 0, 1, 0),
                (100, 10, (1 << 21) + 1, 1, 0), (100, 10, 10, 0, 0), (100, 10, 10, 4097, 0), (100, 10, 10, 1, -1), (1 << 24, 10, 10, 1, 64)):
        assert q(*bad) == 0, bad
    for ok in ((1, 1, 1, 1, 0), (1000, 368, 135, 4, 0), (1000, 368, 135, 4, 64), (16384, 4128, 2181, 51, 0), (262144, 4128, 2181, 51, 0), (1 << 24, 1 << 20, 1 << 21, 4096, 0)):
        assert q(*ok) > 0 and q(*ok) % 16 == 0, ok
    assert q(1000, 368, 135, 4, 64) > q(1000, 368, 135, 4, 0)                       # sixteen segments of partials, not one
    assert q(16384, 4128, 2181, 51, 0) >= 16 * 2181 * 3 * 8 + 4128 * 9 * 4
    assert q(1000, 368, 135, 4, 0) < q(1000, 368, 1350, 4, 0) and q(1000, 368, 135, 4, 0) < q(1000, 3680, 135, 4, 0)


def test_the_workspace_sizes_are_those_of_the_layout_before_the_shared_header():
    """(M, F, V, G, segment) -> bytes, read from the library of the commit before csrc/mesh_walk.h laid the common regions down."""
    q = _lib.family('eval').dbw_eval_surface_workspace_bytes
    for args, nbytes in (((1, 1, 3, 1, 0), 240), ((257, 12, 8, 2, 64), 1728), ((1000, 928, 501, 11, 0), 63008),
                         ((16384, 4128, 2181, 51, 0), 1064064), ((16384, 4128, 2181, 51, 64), 13626624)):
        assert q(*args) == nbytes, args
    assert q(0, 1, 3, 1, 0) == 0 and q(1, 1, 3, 1, -1) == 0


def _caller(lib, fn, names, good):
    ints = {'N', 'n_points', 'seed', 'step', 'V', 'F', 'G', 'A', 'cull', 'segment'}

    def refused(text, **change):
        a = dict(good, **change)
        rc = getattr(lib, fn)(*[a[n] if n in ints else (float(a[n]) if n in FLOATS else ctypes.c_void_p(a[n])) for n in names])
        assert rc < 0, change
        msg = lib.dbw_last_error().decode()
        assert msg.startswith(fn + ': ') and text in msg, (change, msg)
    return refused


def test_refused_arguments_return_their_text_before_any_launch():
    """Nothing here reaches a kernel: the device pointers are made-up addresses that are only looked at, never followed."""
    lib = _lib.family('eval')
    A = 1 << 20                                                     # an aligned, non-null address
    common = dict(points=A, N=1000, n_points=256, seed=1, step=2, verts=A, V=135, faces=A, F=368, G=4, vert_alpha=A, vert_group=A, A=3,
                  back_count=126.0, tau=0.1, back=0.5, workspace=A, records=A, stream=0)
    fwd = _caller(lib, 'dbw_eval_surface_fwd', FWD, dict(common, faces_host=0, face_group=A, group_keep=0, cull=1, value=A))
    bwd = _caller(lib, 'dbw_eval_surface_bwd', BWD, dict(common, weight=1.0, grad_out=0, segment=0, grad_verts=A, grad_alpha=A))
    for name in ('points', 'verts', 'faces', 'face_group', 'workspace', 'records', 'value'):
        fwd('null pointer', **{name: 0})
    for name in ('points', 'verts', 'faces', 'workspace', 'records', 'grad_verts'):
        bwd('null pointer', **{name: 0})
    for ref in (fwd, bwd):
        ref('N must be in [1, 2^31)', N=0)
        ref('N must be in [1, 2^31)', N=1 << 31)
        ref('must be in [1, 2^24]', n_points=-1)
        ref('must be in [1, 2^24]', n_points=(1 << 24) + 1)
        ref('must be in [1, 2^24]', n_points=0, N=(1 << 24) + 1)
        ref('F must be in [1, 2^20]', F=0)
        ref('F must be in [1, 2^20]', F=(1 << 20) + 1)
        ref('V must be in [1, 2^21]', V=0)
        ref('V must be in [1, 2^21]', V=(1 << 21) + 1)
        ref('G must be in [1, 4096]', G=0)
        ref('G must be in [1, 4096]', G=4097)
        ref('tau must be positive and finite', tau=0.0)
        ref('tau must be positive and finite', tau=-1.0)
        ref('tau must be positive and finite', tau=float('nan'))
        ref('back must be non-negative and finite', back=-0.5)
        ref('back must be non-negative and finite', back=float('inf'))
        ref('back > 0 needs vert_alpha and vert_group', vert_alpha=0)
        ref('back > 0 needs vert_alpha and vert_group', vert_group=0)
        ref('A must be in [0, V]', A=-1)
        ref('A must be in [0, V]', A=136)
        ref('back > 0 needs A >= 1 and a positive back_count', A=0)
        ref('back > 0 needs A >= 1 and a positive back_count', back_count=0.0)
        ref('workspace is not 16-byte aligned', workspace=A + 8)
        ref('records are not 16-byte aligned', records=A + 8)
        for name in ('points', 'verts', 'faces', 'vert_alpha', 'vert_group'):
            ref('misaligned pointer', **{name: A + 2})
    fwd('cull must be 0 or 1', cull=2)
    for name in ('face_group', 'group_keep'):
        fwd('misaligned pointer', **{name: A + 2})
    fwd('misaligned pointer', value=A + 4)
    bwd('back > 0 needs grad_alpha', grad_alpha=0)
    bwd('weight must be finite', weight=float('inf'))
    bwd('segment must be 0 or in [64, 2^20]', segment=63)
    bwd('segment must be 0 or in [64, 2^20]', segment=(1 << 20) + 1)
    bwd('too many segments', n_points=1 << 24, segment=64)
    for name in ('grad_out', 'grad_verts', 'grad_alpha'):
        bwd('misaligned pointer', **{name: A + 2})
    # a host copy of the faces is checked against V, the one pointer here that IS followed
    faces = np.zeros((368, 3), np.int32)
    faces[200, 1] = 135
    fwd('a face index is outside [0, V)', faces_host=faces.ctypes.data)
    faces[200, 1] = -1
    fwd('a face index is outside [0, V)', faces_host=faces.ctypes.data)


def test_family_refuses_a_library_without_the_new_functions(monkeypatch):
    f = _lib.FAMILIES['eval']
    old = {n: (lambda *a: 0) for n in list(f.signatures) + list(f.other_signatures) if n not in NEW}
    stub = types.SimpleNamespace(dbw_eval_abi_version=lambda: 1, **old)
    monkeypatch.setattr(_lib, '_lib', stub)
    with pytest.raises(RuntimeError, match=r'has the eval family of include/dbw_eval\.h at revision 1 but not .*dbw_eval_surface_fwd.*rebuild it'):
        _lib.family('eval')
    for n in NEW:
        setattr(stub, n, lambda *a: 0)
    assert _lib.family('eval') is stub
