"""CPU: the k-means entry points added to include/dbw_eval.h under its revision 1 -- the prototypes against the ctypes binding one argument at
a time, the exported symbols, the size query, every refused argument (validated before any launch: no device is needed), and
_lib.family('eval') on a library that has the family but not these functions."""
import ctypes
import re
import types

import pytest

import abi_header as AH
from dbw_amd import _lib

NEW = {'dbw_eval_cluster_fit': 'int', 'dbw_eval_cluster_workspace_bytes': 'size_t'}
SCALARS = {'int': ctypes.c_int, 'float': ctypes.c_float, 'int64_t': ctypes.c_int64, 'dbw_stream_t': ctypes.c_void_p}
OTHER_WORDS = ('viz', 'render_lit', 'vertex_normals', 'export', 'frames', 'resample', 'ingest', 'lens', 'undistort', 'monitor', 'meter', 'scores', 'icp')
ARGS = ['points', 'N', 'K', 'init', 'n_iter', 'workspace', 'centres', 'labels', 'counts', 'mean', 'cov', 'evals', 'axes', 'info', 'stream']


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
    ret, args = _declared('dbw_eval_cluster_fit')
    assert ret == 'int' and [n for _, n in args] == ARGS
    pointers = {'points': 'const float *', 'init': 'const float *', 'workspace': 'void *', 'centres': 'float *', 'labels': 'int32_t *',
                'counts': 'int32_t *', 'mean': 'double *', 'cov': 'double *', 'evals': 'double *', 'axes': 'double *', 'info': 'int32_t *'}
    bound = _lib.EVAL_SIGNATURES['dbw_eval_cluster_fit']
    assert len(bound) == len(args)
    for (typ, name), c in zip(args, bound):
        if name in pointers:
            assert typ == pointers[name] and c is ctypes.c_void_p, name
        else:
            assert '*' not in typ and SCALARS[typ] is c, name
    ret, args = _declared('dbw_eval_cluster_workspace_bytes')
    assert ret == 'size_t' and [t for t, _ in args] == ['int64_t', 'int']
    assert _lib.EVAL_OTHER_SIGNATURES['dbw_eval_cluster_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int])
    assert AH.defines('dbw_eval.h')['DBW_EVAL_ABI_VERSION'] == 1


def test_names_exports_and_the_size_query():
    for n in NEW:
        assert 'eval' in n and not any(w in n for w in OTHER_WORDS)
        assert n in AH.exported()
    lib = _lib.family('eval')
    assert lib.dbw_eval_cluster_fit.restype is ctypes.c_int and lib.dbw_eval_cluster_workspace_bytes.restype is ctypes.c_size_t
    q = lib.dbw_eval_cluster_workspace_bytes
    assert q(100, 0) == 0 and q(100, 257) == 0 and q(3, 4) == 0 and q(1 << 31, 8) == 0 and q(0, 0) == 0 and q(-5, 1) == 0
    for N, K in ((1, 1), (100, 1), (100, 100), (5000, 64), (5000, 256), ((1 << 31) - 1, 256)):
        assert q(N, K) > 0 and q(N, K) % 16 == 0, (N, K)
    assert q(5000, 1) < q(5000, 256) and q(5000, 8) < q(50000, 8)
    assert q((1 << 31) - 1, 256) >= 8 * ((1 << 31) - 1)            # mind and the labels: two 4-byte entries a point


def test_refused_arguments_return_their_text_before_any_launch():
    """Nothing here reaches a kernel: the pointers are made-up addresses that are only looked at, never followed."""
    lib = _lib.family('eval')
    A = 1 << 20                                                     # an aligned, non-null address
    good = dict(points=A, N=100, K=4, init=0, n_iter=3, workspace=A, centres=A, labels=0, counts=A, mean=0, cov=0, evals=0, axes=0, info=A, stream=0)

    def refused(text, **change):
        a = dict(good, **change)
        rc = lib.dbw_eval_cluster_fit(*[ctypes.c_void_p(a[n]) if n not in ('N', 'K', 'n_iter') else a[n] for n in ARGS])
        assert rc < 0, change
        msg = lib.dbw_last_error().decode()
        assert msg.startswith('dbw_eval_cluster_fit: ') and text in msg, (change, msg)

    for name in ('points', 'workspace', 'centres', 'counts', 'info'):
        refused('null pointer', **{name: 0})
    refused('K must be in [1, 256]', K=0)
    refused('K must be in [1, 256]', K=257, N=1000)
    refused('N must be in [K, 2^31)', N=3)
    refused('N must be in [K, 2^31)', N=1 << 31)
    refused('n_iter must be in [0, 64]', n_iter=-1)
    refused('n_iter must be in [0, 64]', n_iter=65)
    refused('workspace is not 16-byte aligned', workspace=A + 8)
    for name in ('points', 'init', 'centres', 'labels', 'counts', 'info'):
        refused('misaligned pointer', **{name: A + 2})
    for name in ('mean', 'cov', 'evals', 'axes'):
        refused('misaligned pointer', **{name: A + 4})


def test_family_refuses_a_library_without_the_new_functions(monkeypatch):
    f = _lib.FAMILIES['eval']
    old = {n: (lambda *a: 0) for n in list(f.signatures) + list(f.other_signatures) if n not in NEW}
    stub = types.SimpleNamespace(dbw_eval_abi_version=lambda: 1, **old)
    monkeypatch.setattr(_lib, '_lib', stub)
    with pytest.raises(RuntimeError, match=r'has the eval family of include/dbw_eval\.h at revision 1 but not .*dbw_eval_cluster_fit.*rebuild it'):
        _lib.family('eval')
    for n in NEW:
        setattr(stub, n, lambda *a: 0)
    assert _lib.family('eval') is stub
