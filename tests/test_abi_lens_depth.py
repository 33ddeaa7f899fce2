"""CPU: the depth-cloud entry points added to include/dbw_lens.h under its revision 1 -- the prototypes against the ctypes binding one argument
at a time, the exported symbols, the size query, every refused argument (validated before any launch: no device is needed), and
_lib.family('lens') on a library that has the family but not these functions."""
import ctypes
import re
import types

import numpy as np
import pytest

import abi_header as AH
from dbw_amd import _lib

NEW = {'dbw_lens_depth_cloud': 'int', 'dbw_lens_depth_cloud_workspace_bytes': 'size_t'}
SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'dbw_stream_t': ctypes.c_void_p}
OTHER_WORDS = ('eval', 'nn_points', 'lattice', 'downsample', 'viz', 'render_lit', 'vertex_normals', 'export', 'frames', 'resample', 'ingest', 'monitor',
               'meter', 'scores', 'icp')
ARGS = ['depth', 'N', 'H', 'W', 'cams', 'target', 'poses', 'box', 'G', 'd_min', 'd_max', 'stride', 'edge_permille', 'min_count', 'workspace', 'points',
        'counts', 'capacity', 'info', 'stream']
POINTERS = {'depth': 'const uint16_t *', 'cams': 'const float *', 'target': 'const float *', 'poses': 'const float *', 'box': 'const float *',
            'workspace': 'void *', 'points': 'float *', 'counts': 'int32_t *', 'info': 'int64_t *'}


def _declared(name):
    """[(type as written, argument name)] of the prototype of `name` in include/dbw_lens.h"""
    src = re.sub(r'/\*.*?\*/', '', AH.text('dbw_lens.h'), flags=re.S)
    ret, args = re.search(r'\b(\w+)\s+%s\s*\(([^;]*?)\)\s*;' % name, src, flags=re.S).groups()
    out = []
    for a in ' '.join(args.split()).split(','):
        m = re.fullmatch(r'\s*(.*?)(\w+)\s*', a)
        out.append((m.group(1).strip(), m.group(2)))
    return ret, out


def test_prototypes_match_the_binding_argument_by_argument():
    ret, args = _declared('dbw_lens_depth_cloud')
    assert ret == 'int' and [n for _, n in args] == ARGS
    bound = _lib.LENS_SIGNATURES['dbw_lens_depth_cloud']
    assert len(bound) == len(args)
    for (typ, name), c in zip(args, bound):
        if name in POINTERS:
            assert typ == POINTERS[name] and c is ctypes.c_void_p, name
        else:
            assert '*' not in typ and SCALARS[typ] is c, name
    ret, args = _declared('dbw_lens_depth_cloud_workspace_bytes')
    assert ret == 'size_t' and [t for t, _ in args] == ['int']
    assert _lib.LENS_OTHER_SIGNATURES['dbw_lens_depth_cloud_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int])
    assert AH.defines('dbw_lens.h')['DBW_LENS_ABI_VERSION'] == 1


def test_names_exports_and_the_size_query():
    for n in NEW:
        assert 'lens' in n and not any(w in n for w in OTHER_WORDS)
        assert n in AH.exported()
    lib = _lib.family('lens')
    assert lib.dbw_lens_depth_cloud.restype is ctypes.c_int and lib.dbw_lens_depth_cloud_workspace_bytes.restype is ctypes.c_size_t
    q = lib.dbw_lens_depth_cloud_workspace_bytes
    assert q(0) == 0 and q(257) == 0 and q(-3) == 0
    sizes = [q(G) for G in range(1, 257)]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    assert q(128) >= 28 * 128 ** 3                                   # a 32-bit count and three 64-bit sums a cell


def test_refused_arguments_return_their_text_before_any_launch():
    """Nothing here reaches a kernel: the device pointers are made-up addresses that are only looked at, never followed; the four host
    arrays are real, since the call reads them."""
    lib = _lib.family('lens')
    A = 1 << 20                                                     # an aligned, non-null address
    N = 3
    cams = np.zeros((N, 16), np.float32)
    cams[:, 1:5] = (30.0, 30.0, 16.0, 12.0)
    target = np.float32([16.0, 12.0, 1 / 30.0, 1 / 30.0])
    poses = np.tile(np.float32([1e-3, 0, 0, 0, 1e-3, 0, 0, 0, 1e-3, 0, 0, 0]), (N, 1))
    box = np.float32([-2.0, -2.0, -2.0, 8 * 1024 / 4.0])
    host = {'cams': cams, 'target': target, 'poses': poses, 'box': box}
    good = dict(depth=A, N=N, H=24, W=32, G=8, d_min=1, d_max=65535, stride=1, edge_permille=50, min_count=1, workspace=A, points=A, counts=A,
                capacity=512, info=A, stream=0)

    def refused(text, **change):
        a = dict(good, **{k: v for k, v in change.items() if k not in host})
        arrays = {k: np.ascontiguousarray(change.get(k, v), dtype=np.float32) if change.get(k, v) is not None else None for k, v in host.items()}
        a.update({k: (0 if v is None else v.ctypes.data) for k, v in arrays.items()})
        rc = lib.dbw_lens_depth_cloud(*[ctypes.c_void_p(a[n]) if n in POINTERS or n == 'stream' else a[n] for n in ARGS])
        assert rc < 0, change
        msg = lib.dbw_last_error().decode()
        assert msg.startswith('dbw_lens_depth_cloud: ') and text in msg, (change, msg)

    for name in ('depth', 'workspace', 'points', 'counts', 'info'):
        refused('null pointer', **{name: 0})
    for name in host:
        refused('null pointer', **{name: None})
    refused('workspace is not 16-byte aligned', workspace=A + 8)
    refused('depth: misaligned', depth=A + 1)
    refused('points, counts: misaligned', points=A + 2)
    refused('points, counts: misaligned', counts=A + 2)
    refused('info: misaligned', info=A + 4)
    refused('N below 1', N=0)
    refused('H, W below 1', H=0)
    refused('H, W below 1', W=0)
    refused('G must be in [1, 256]', G=0)
    refused('G must be in [1, 256]', G=257)
    refused('stride below 1', stride=0)
    refused('d_min must be in [1, d_max]', d_min=0)
    refused('d_min must be in [1, d_max]', d_min=301, d_max=300)
    refused('d_max above 65535', d_max=65536)
    refused('edge_permille must be in [0, 1000]', edge_permille=-1)
    refused('edge_permille must be in [0, 1000]', edge_permille=1001)
    refused('min_count below 1', min_count=0)
    refused('capacity below', capacity=511)                                    # G^3 = 512 < 3 * 24 * 32
    refused('capacity below', G=64, capacity=3 * 24 * 32 - 1)                  # 3 * 24 * 32 < G^3
    refused('capacity below', G=64, stride=3, capacity=3 * 8 * 11 - 1)         # ceil(24 / 3) * ceil(32 / 3)
    for name, a in host.items():
        for bad in (np.nan, np.inf):
            b = a.copy()
            b.reshape(-1)[-1 if name != 'cams' else 7] = bad
            refused(f'{name}: a value that is not finite', **{name: b})
    b = cams.copy()
    b[2, 15] = np.inf                                                          # the padding of a row too, as dbw_lens_rectify_u8 has it
    refused('cams: a value that is not finite', cams=b)
    for v in (0.0, -1.0):
        b = box.copy()
        b[3] = v
        refused('box: inv_step is not positive', box=b)
        b = cams.copy()
        b[1, 2] = v
        refused('cams: a focal length that is not positive', cams=b)
        b = target.copy()
        b[2] = v
        refused('target: a reciprocal focal length that is not positive', target=b)
    b = cams.copy()
    b[0, 0] = 2.0
    refused('cams: a model id that is neither 0 nor 1', cams=b)


def test_family_refuses_a_library_without_the_new_functions(monkeypatch):
    f = _lib.FAMILIES['lens']
    old = {n: (lambda *a: 0) for n in list(f.signatures) + list(f.other_signatures) if n not in NEW}
    stub = types.SimpleNamespace(dbw_lens_abi_version=lambda: 1, **old)
    monkeypatch.setattr(_lib, '_lib', stub)
    with pytest.raises(RuntimeError, match=r'has the lens family of include/dbw_lens\.h at revision 1 but not .*dbw_lens_depth_cloud.*rebuild it'):
        _lib.family('lens')
    for n in NEW:
        setattr(stub, n, lambda *a: 0)
    assert _lib.family('lens') is stub
