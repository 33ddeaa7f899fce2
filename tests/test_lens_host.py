"""CPU tests of the lens rectification's host side: the C boundary include/dbw_lens.h against its ctypes binding and the library, and
argument validation before any launch."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from dbw_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'dbw_lens.h')
CTYPE = {'int': ctypes.c_int, 'float': ctypes.c_float, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t, 'dbw_stream_t': ctypes.c_void_p}


def _protos(ret, header=HEADER):
    src = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r'\b%s\s+(dbw_\w+)\s*\(([^;{]*?)\)\s*;' % ret, src, flags=re.S):
        args = ' '.join(args.split())
        out[name] = [] if args in ('', 'void') else [ctypes.c_void_p if '*' in a else CTYPE[a.replace('const ', '').split()[0]] for a in args.split(',')]
    return out


def test_lens_header_is_plain_c99(tmp_path):
    src = tmp_path / 'lens.c'
    src.write_text('#include "dbw_lens.h"\nint main(void) { return DBW_LENS_ABI_VERSION == 1 && DBW_LENS_N_PARAMS == 12 ? 0 : 1; }\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-I', os.path.join(ROOT, 'include'), '-c', str(src), '-o',
                        str(tmp_path / 'lens.o')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_lens_header_matches_the_binding_and_the_library():
    ints = _protos('int')
    assert set(ints) == set(_lib.LENS_SIGNATURES) | {'dbw_lens_abi_version'} and not _protos('size_t')
    lib = _lib.load()
    for name, types in _lib.LENS_SIGNATURES.items():
        assert ints[name] == types, name
        assert getattr(lib, name).argtypes == types and getattr(lib, name).restype == ctypes.c_int
    src = open(HEADER).read()
    assert lib.dbw_lens_abi_version() == _lib.LENS_ABI_VERSION == int(re.search(r'#define DBW_LENS_ABI_VERSION (\d+)', src).group(1)) == 1
    assert _lib.LENS_N_PARAMS == int(re.search(r'#define DBW_LENS_N_PARAMS (\d+)', src).group(1)) == ops.lens_params((1, 1, 0, 0), (0,) * 6).numel()
    # the library exports exactly these names of the new boundary, and none of them reads like a name of the ingest's or the frame export's
    syms = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r' T (dbw_\w+)', syms))
    assert set(ints) <= exported and {n for n in exported if 'lens' in n or 'undistort' in n} == set(ints)
    assert not any(w in n for n in ints for w in ('resample', 'ingest', 'export', 'frames'))
    # the other five boundaries are what they were
    assert lib.dbw_abi_version() == _lib.ABI_VERSION == 7 and lib.dbw_viz_abi_version() == _lib.VIZ_ABI_VERSION == 1
    assert lib.dbw_eval_abi_version() == _lib.EVAL_ABI_VERSION == 1 and lib.dbw_export_abi_version() == _lib.EXPORT_ABI_VERSION == 1
    assert lib.dbw_ingest_abi_version() == _lib.INGEST_ABI_VERSION == 1
    others = (set(_lib.SIGNATURES) | set(_lib.OTHER_SIGNATURES) | set(_lib.EVAL_SIGNATURES) | set(_lib.VIZ_SIGNATURES) | set(_lib.VIZ_OTHER_SIGNATURES)
              | set(_lib.EXPORT_SIGNATURES) | set(_lib.INGEST_SIGNATURES) | set(_lib.INGEST_OTHER_SIGNATURES))
    assert not set(_lib.LENS_SIGNATURES) & others
    for h in ('dbw_hip.h', 'dbw_viz.h', 'dbw_eval.h', 'dbw_export.h', 'dbw_ingest.h'):
        text = open(os.path.join(ROOT, 'include', h)).read()
        assert 'undistort' not in text and 'dbw_lens' not in text, h


def _args(**over):
    """Arguments of dbw_images_undistort_u8 with the device pointers non-null (never dereferenced: each call below must fail validation, on
    the host) and a real host array of lens values."""
    lens = (ctypes.c_float * 12)(30.0, 30.0, 16.0, 12.0, 1 / 30.0, 1 / 30.0, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0)
    a = dict(src=ctypes.c_void_p(1 << 20), N=2, H=24, W=32, lens=ctypes.cast(lens, ctypes.c_void_p), out=ctypes.c_void_p(1 << 24), stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return list(a.values()), lens


def test_images_undistort_validates_before_any_launch():
    lib = _lib.load()
    f = lib.dbw_images_undistort_u8

    def rc(**over):
        args, keep = _args(**over)
        return f(*args)

    for over in (dict(src=None), dict(lens=None), dict(out=None)):
        assert rc(**over) == -1 and b'null pointer' in lib.dbw_last_error(), over
    for over in (dict(N=0), dict(N=-3)):
        assert rc(**over) == -1 and b'N below 1' in lib.dbw_last_error(), over
    for over in (dict(H=1), dict(W=1), dict(H=0), dict(W=-2)):
        assert rc(**over) == -1 and b'below 2 x 2' in lib.dbw_last_error(), over
    assert rc(H=1 << 16, W=1 << 16) == -1 and b'bad size' in lib.dbw_last_error()
    # overlapping buffers: the same one, and out beginning inside src or ending inside it (2 * 24 * 32 * 3 = 4608 bytes each)
    base = 1 << 20
    for out in (base, base + 4607, base - 4607):
        assert rc(out=ctypes.c_void_p(out)) == -1 and b'overlap' in lib.dbw_last_error(), out
    bad = (ctypes.c_float * 12)(*([30.0] * 6 + [float('nan')] + [0.0] * 5))
    assert rc(lens=ctypes.cast(bad, ctypes.c_void_p)) == -1 and b'not finite' in lib.dbw_last_error()
    with pytest.raises(RuntimeError, match='overlap'):
        _lib.call('dbw_images_undistort_u8', *_args(out=ctypes.c_void_p(base))[0])


def test_undistort_u8_has_no_cpu_path():
    with pytest.raises(RuntimeError, match='GPU'):
        ops.undistort_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (8.0, 8.0, 4.0, 4.0), (0.1, 0, 0, 0, 0, 0))
    with pytest.raises(ValueError):
        ops.lens_params((8.0, 8.0, 4.0), (0.0,) * 6)
    with pytest.raises(ValueError):
        ops.lens_params((8.0, 0.0, 4.0, 4.0), (0.0,) * 6)
