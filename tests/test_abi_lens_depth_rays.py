"""CPU: dbw_lens_depth_rays, added to include/dbw_lens.h under its revision 1 -- the prototype against the ctypes binding one argument at a
time (the arguments of dbw_lens_depth_cloud without the grid and the cube), the exported symbol, every refused argument (validated before
any launch: no device is needed), and _lib.family('lens') on a library that has the family but not this function."""
import ctypes
import re
import types

import numpy as np
import pytest

import abi_header as AH
from dbw_amd import _lib

NEW = {'dbw_lens_depth_rays': 'int'}
SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'dbw_stream_t': ctypes.c_void_p}
OTHER_WORDS = ('eval', 'nn_points', 'lattice', 'downsample', 'viz', 'render_lit', 'vertex_normals', 'export', 'frames', 'resample', 'ingest', 'monitor',
               'meter', 'scores', 'icp')
ARGS = ['depth', 'N', 'H', 'W', 'cams', 'target', 'poses', 'd_min', 'd_max', 'stride', 'edge_permille', 'rays', 'stream']
POINTERS = {'depth': 'const uint16_t *', 'cams': 'const float *', 'target': 'const float *', 'poses': 'const float *', 'rays': 'void *'}


def _declared(name):
    """[(type as written, argument name)] of the prototype of `name` in include/dbw_lens.h"""
    src = re.sub(r'/\*.*?\*/', '', AH.text('dbw_lens.h'), flags=re.S)
    ret, args = re.search(r'\b(\w+)\s+%s\s*\(([^;]*?)\)\s*;' % name, src, flags=re.S).groups()
    out = []
    for a in ' '.join(args.split()).split(','):
        m = re.fullmatch(r'\s*(.*?)(\w+)\s*', a)
        out.append((m.group(1).strip(), m.group(2)))
    return ret, out


def test_the_prototype_matches_the_binding_argument_by_argument():
    ret, args = _declared('dbw_lens_depth_rays')
    assert ret == 'int' and [n for _, n in args] == ARGS
    bound = _lib.LENS_SIGNATURES['dbw_lens_depth_rays']
    assert len(bound) == len(args)
    for (typ, name), c in zip(args, bound):
        if name in POINTERS:
            assert typ == POINTERS[name] and c is ctypes.c_void_p, name
        else:
            assert '*' not in typ and SCALARS[typ] is c, name
    # the arguments of the depth cloud without the grid, the cube and what a reduction needs
    cloud = [n for _, n in _declared('dbw_lens_depth_cloud')[1]]
    dropped = ('box', 'G', 'min_count', 'workspace', 'points', 'counts', 'capacity', 'info')
    assert [n for n in cloud if n not in dropped] == [n for n in ARGS if n != 'rays']
    assert AH.defines('dbw_lens.h')['DBW_LENS_ABI_VERSION'] == 1


def test_the_name_and_the_export():
    for n in NEW:
        assert 'lens' in n and not any(w in n for w in OTHER_WORDS)
        assert n in AH.exported()
    assert _lib.family('lens').dbw_lens_depth_rays.restype is ctypes.c_int


def test_refused_arguments_return_their_text_before_any_launch():
    """Nothing here reaches a kernel: the device pointers are made-up addresses that are only looked at, never followed; the three host
    arrays are real, since the call reads them."""
    lib = _lib.family('lens')
    A = 1 << 20                                                     # an aligned, non-null address
    N = 3
    cams = np.zeros((N, 16), np.float32)
    cams[:, 1:5] = (30.0, 30.0, 16.0, 12.0)
    target = np.float32([16.0, 12.0, 1 / 30.0, 1 / 30.0])
    poses = np.tile(np.float32([1e-3, 0, 0, 0, 1e-3, 0, 0, 0, 1e-3, 0, 0, 0]), (N, 1))
    host = {'cams': cams, 'target': target, 'poses': poses}
    good = dict(depth=A, N=N, H=24, W=32, d_min=1, d_max=65535, stride=1, edge_permille=50, rays=A, stream=0)

    def refused(text, **change):
        a = dict(good, **{k: v for k, v in change.items() if k not in host})
        arrays = {k: np.ascontiguousarray(change.get(k, v), dtype=np.float32) if change.get(k, v) is not None else None for k, v in host.items()}
        a.update({k: (0 if v is None else v.ctypes.data) for k, v in arrays.items()})
        rc = lib.dbw_lens_depth_rays(*[ctypes.c_void_p(a[n]) if n in POINTERS or n == 'stream' else a[n] for n in ARGS])
        assert rc < 0, change
        msg = lib.dbw_last_error().decode()
        assert msg.startswith('dbw_lens_depth_rays: ') and text in msg, (change, msg)

    for name in ('depth', 'rays'):
        refused('null pointer', **{name: 0})
    for name in host:
        refused('null pointer', **{name: None})
    refused('rays are not 16-byte aligned', rays=A + 8)
    refused('rays are not 16-byte aligned', rays=A + 4)
    refused('depth: misaligned', depth=A + 1)
    refused('N below 1', N=0)
    refused('H, W below 1', H=0)
    refused('H, W below 1', W=0)
    refused('H * W must be below 2^29', H=1 << 15, W=1 << 14)
    refused('stride below 1', stride=0)
    refused('d_min must be in [1, d_max]', d_min=0)
    refused('d_min must be in [1, d_max]', d_min=301, d_max=300)
    refused('d_max above 65535', d_max=65536)
    refused('edge_permille must be in [0, 1000]', edge_permille=-1)
    refused('edge_permille must be in [0, 1000]', edge_permille=1001)
    refused('must be below 2^31', H=1 << 14, W=1 << 14, N=8, cams=np.tile(cams[:1], (8, 1)), poses=np.tile(poses[:1], (8, 1)))
    for name, a in host.items():
        for bad in (np.nan, np.inf):
            b = a.copy()
            b.reshape(-1)[-1 if name != 'cams' else 7] = bad
            refused(f'{name}: a value that is not finite', **{name: b})
    for v in (0.0, -1.0):
        b = cams.copy()
        b[1, 2] = v
        refused('cams: a focal length that is not positive', cams=b)
        b = target.copy()
        b[2] = v
        refused('target: a reciprocal focal length that is not positive', target=b)
    b = cams.copy()
    b[0, 0] = 2.0
    refused('cams: a model id that is neither 0 nor 1', cams=b)


def test_family_refuses_a_library_without_the_new_function(monkeypatch):
    f = _lib.FAMILIES['lens']
    old = {n: (lambda *a: 0) for n in list(f.signatures) + list(f.other_signatures) if n not in NEW}
    stub = types.SimpleNamespace(dbw_lens_abi_version=lambda: 1, **old)
    monkeypatch.setattr(_lib, '_lib', stub)
    with pytest.raises(RuntimeError, match=r'has the lens family of include/dbw_lens\.h at revision 1 but not .*dbw_lens_depth_rays.*rebuild it'):
        _lib.family('lens')
    for n in NEW:
        setattr(stub, n, lambda *a: 0)
    assert _lib.family('lens') is stub
