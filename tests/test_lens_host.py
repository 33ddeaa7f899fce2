"""CPU tests of the lens rectification's host side: argument validation of include/dbw_lens.h before any launch (the boundary against its
ctypes binding and the library: tests/test_abi_families.py)."""
import ctypes

import pytest
import torch

from dbw_amd import _lib, ops


def test_lens_params_fill_the_count_of_the_header():
    assert ops.lens_params((1, 1, 0, 0), (0,) * 6).numel() == _lib.LENS_N_PARAMS


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
