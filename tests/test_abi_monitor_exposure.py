"""CPU: the exposure entry points added to include/dbw_monitor.h under its revision 1 -- the prototypes against the ctypes binding one
argument at a time, the exported symbols, the size query, every refused argument (validated before any launch: no device is needed), and
_lib.family('monitor') on a library that has the family but not these functions."""
import ctypes
import re
import types

import pytest

import abi_header as AH
from dbw_amd import _lib

NEW = {'dbw_monitor_exposure_composite': 'int', 'dbw_monitor_exposure_composite_workspace_bytes': 'size_t'}
SCALARS = {'int': ctypes.c_int, 'double': ctypes.c_double, 'dbw_stream_t': ctypes.c_void_p}
OTHER_WORDS = ('eval', 'nn_points', 'lattice', 'downsample', 'viz', 'render_lit', 'vertex_normals', 'export', 'frames', 'resample', 'ingest', 'lens',
               'undistort', 'icp')
ARGS = ['fg', 'env', 'imgs', 'masks', 'theta', 'ids', 'N', 'H', 'W', 'V', 'scale', 'workspace', 'rec', 'value', 'upstream', 'grad_rec', 'grad_fg',
        'grad_env', 'grad_theta', 'stream']
POINTERS = {'fg': 'const float *', 'env': 'const float *', 'imgs': 'const float *', 'masks': 'const float *', 'theta': 'const float *',
            'ids': 'const int32_t *', 'workspace': 'void *', 'rec': 'float *', 'value': 'double *', 'upstream': 'const float *',
            'grad_rec': 'const float *', 'grad_fg': 'float *', 'grad_env': 'float *', 'grad_theta': 'float *'}


def _declared(name):
    """[(type as written, argument name)] of the prototype of `name` in include/dbw_monitor.h"""
    src = re.sub(r'/\*.*?\*/', '', AH.text('dbw_monitor.h'), flags=re.S)
    ret, args = re.search(r'\b(\w+)\s+%s\s*\(([^;]*?)\)\s*;' % name, src, flags=re.S).groups()
    out = []
    for a in ' '.join(args.split()).split(','):
        m = re.fullmatch(r'\s*(.*?)(\w+)\s*', a)
        out.append((m.group(1).strip(), m.group(2)))
    return ret, out


def test_prototypes_match_the_binding_argument_by_argument():
    ret, args = _declared('dbw_monitor_exposure_composite')
    assert ret == 'int' and [n for _, n in args] == ARGS
    bound = _lib.MONITOR_SIGNATURES['dbw_monitor_exposure_composite']
    assert len(bound) == len(args)
    for (typ, name), c in zip(args, bound):
        if name in POINTERS:
            assert typ == POINTERS[name] and c is ctypes.c_void_p, name
        else:
            assert '*' not in typ and SCALARS[typ] is c, name
    ret, args = _declared('dbw_monitor_exposure_composite_workspace_bytes')
    assert ret == 'size_t' and [t for t, _ in args] == ['int', 'int', 'int']
    assert _lib.MONITOR_OTHER_SIGNATURES['dbw_monitor_exposure_composite_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert AH.defines('dbw_monitor.h')['DBW_MONITOR_ABI_VERSION'] == 1 and AH.defines('dbw_hip.h')['DBW_ABI_VERSION'] == 7


def test_names_exports_and_the_size_query():
    for n in NEW:
        assert 'monitor' in n and not any(w in n for w in OTHER_WORDS)
        assert n in AH.exported()
    lib = _lib.family('monitor')
    assert lib.dbw_monitor_exposure_composite.restype is ctypes.c_int
    assert lib.dbw_monitor_exposure_composite_workspace_bytes.restype is ctypes.c_size_t
    q = lib.dbw_monitor_exposure_composite_workspace_bytes
    assert q(0, 8, 8) == 0 and q(-1, 8, 8) == 0 and q(2, 0, 8) == 0 and q(2, 8, -1) == 0 and q(65536, 8, 8) == 0
    assert q(1, 1 << 16, 1 << 15) == 0                                # H * W = 2^31
    assert q(1, 1, 1) == 48                                           # one workgroup, six fp64
    assert q(3, 40, 100) == 3 * 16 * 48                               # ceil(4000 / 256) workgroups a view in the element form
    assert q(2, 1024, 1024) == 2 * 256 * 48                           # at most 256 workgroups a view
    assert all(q(N, H, W) % 8 == 0 for N in (1, 4, 7) for H in (1, 5, 33) for W in (1, 7, 128))


def test_refused_arguments_return_their_text_before_any_launch():
    """Nothing here reaches a kernel: the device pointers are made-up addresses that are only looked at, never followed."""
    lib = _lib.family('monitor')
    A = 1 << 20                                                     # an aligned, non-null address
    fwd = dict(fg=A, env=A, imgs=A, masks=A, theta=A, ids=A, N=2, H=8, W=12, V=5, scale=0.25, workspace=A, rec=A, value=A, upstream=0, grad_rec=0,
               grad_fg=0, grad_env=0, grad_theta=0, stream=0)
    bwd = dict(fwd, rec=0, value=0, upstream=A, grad_rec=A, grad_fg=A, grad_env=A, grad_theta=A)

    def call(a):
        return lib.dbw_monitor_exposure_composite(*[ctypes.c_void_p(a[n]) if n in POINTERS or n == 'stream' else a[n] for n in ARGS])

    def refused(good, text, **change):
        rc = call(dict(good, **change))
        assert rc < 0, change
        msg = lib.dbw_last_error().decode()
        assert msg.startswith('dbw_monitor_exposure_composite: ') and text in msg, (change, msg)

    for good in (fwd, bwd):
        for name in ('fg', 'env', 'imgs', 'theta', 'ids'):
            refused(good, 'null pointer', **{name: 0})
        for change in (dict(N=-1), dict(N=65536), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15)):
            refused(good, 'bad size', **change)
        refused(good, 'V below 1', V=0)
        for bad in (float('nan'), float('inf')):
            refused(good, 'scale is not finite', scale=bad)
        refused(good, 'workspace: null or not 8-byte aligned', workspace=0)
        refused(good, 'workspace: null or not 8-byte aligned', workspace=A + 4)
        for name in ('fg', 'env', 'imgs', 'masks', 'theta', 'ids'):
            refused(good, 'misaligned pointer', **{name: A + 2})
    for names in (('grad_fg',), ('grad_env',), ('grad_theta',), ('grad_fg', 'grad_env'), ('grad_env', 'grad_theta')):
        refused(bwd, 'all or none', **{n: 0 for n in names})
    refused(fwd, 'forward: rec and an 8-byte aligned value', rec=0)
    refused(fwd, 'forward: rec and an 8-byte aligned value', value=0)
    refused(fwd, 'forward: rec and an 8-byte aligned value', value=A + 4)
    refused(fwd, 'forward: rec and an 8-byte aligned value', grad_rec=A)
    refused(fwd, 'forward: rec and an 8-byte aligned value', upstream=A)
    refused(fwd, 'misaligned pointer', rec=A + 2)
    refused(bwd, 'backward: the upstream scalar', upstream=0)
    refused(bwd, 'backward: the upstream scalar', rec=A)
    refused(bwd, 'backward: the upstream scalar', value=A)
    for name in ('upstream', 'grad_rec', 'grad_fg', 'grad_env', 'grad_theta'):
        refused(bwd, 'misaligned pointer', **{name: A + 2})
    # N = 0 launches nothing and needs no workspace; masks and grad_rec may be NULL (checked with N = 0: nothing is followed)
    assert call(dict(fwd, N=0, workspace=0)) == 0 and call(dict(bwd, N=0, workspace=0)) == 0
    assert call(dict(fwd, N=0, masks=0)) == 0 and call(dict(bwd, N=0, masks=0, grad_rec=0)) == 0


def test_family_refuses_a_library_without_the_new_functions(monkeypatch):
    f = _lib.FAMILIES['monitor']
    old = {n: (lambda *a: 0) for n in list(f.signatures) + list(f.other_signatures) if n not in NEW}
    stub = types.SimpleNamespace(dbw_monitor_abi_version=lambda: 1, **old)
    monkeypatch.setattr(_lib, '_lib', stub)
    with pytest.raises(RuntimeError, match=r'has the monitor family of include/dbw_monitor\.h at revision 1 but not '
                                           r'.*dbw_monitor_exposure_composite.*rebuild it'):
        _lib.family('monitor')
    for n in NEW:
        setattr(stub, n, lambda *a: 0)
    assert _lib.family('monitor') is stub
