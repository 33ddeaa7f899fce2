"""CPU tests of the image ingest's host side: the host function dbw_resample_table of include/dbw_ingest.h against the host build of
csrc/resample_math.h, and argument validation before any launch (the boundary against its ctypes binding and the library:
tests/test_abi_families.py)."""
import ctypes

import numpy as np
import pytest
import torch

import resample_ref as RR
from dbw_amd import _lib, ops


@pytest.mark.parametrize('in_size,out_size', [(1600, 400), (768, 768), (53, 13), (24, 50), (400, 3), (260, 65)])
def test_the_library_table_equals_the_host_header_and_the_restatement(in_size, out_size):
    t = ops.resample_table(in_size, out_size)
    assert t.dtype == torch.int32 and not t.is_cuda
    assert np.array_equal(t.numpy(), RR.table_host(in_size, out_size)) and np.array_equal(t.numpy(), RR.table_numpy(in_size, out_size))
    assert ops.resample_table(in_size, out_size) is t                                     # built once per pair


def test_resample_table_sizes_and_errors():
    lib = _lib.load()
    assert lib.dbw_resample_table(1600, 400, None, 0) == 9 and lib.dbw_resample_table(768, 768, None, 0) == 3
    assert lib.dbw_resample_table(768, 384, None, 0) == 5 and lib.dbw_resample_table(400, 3, None, 0) == 2 * 134 + 1
    assert lib.dbw_resample_table(16, 40, None, 0) == 3
    for a, b in ((0, 4), (4, 0), (-1, 4)):
        assert lib.dbw_resample_table(a, b, None, 0) == -1 and b'bad size' in lib.dbw_last_error()
    buf = torch.zeros(4 * 7, dtype=torch.int32)
    assert lib.dbw_resample_table(8, 4, buf.data_ptr(), 4 * 7 - 1) == -1 and b'capacity' in lib.dbw_last_error() and not buf.any()
    assert lib.dbw_resample_table(8, 4, buf.data_ptr(), 4 * 7) == 5 and buf.any()


def test_workspace_bytes():
    lib = _lib.load()
    ws = lib.dbw_images_resample_workspace_bytes
    assert ws(49, 1200, 1600, 300, 400) == 49 * 1200 * 400 * 3             # 4x: the vertical pass reads every row
    assert ws(2, 16, 24, 16, 24) == 0 and ws(2, 23, 31, 7, 31) == 0        # no horizontal pass: no intermediate
    assert ws(2, 23, 31, 23, 8) == 2 * 23 * 8 * 3
    assert ws(0, 8, 8, 4, 4) == 0 and ws(1, 0, 8, 4, 4) == 0 and ws(1, 8, 8, 4, -4) == 0
    t = RR.table_numpy(16, 40)                                              # an up-scaling: the rows the vertical pass reads, from its table
    assert ws(3, 16, 24, 40, 50) == 3 * (t[-1, 0] + t[-1, 1] - t[0, 0]) * 50 * 3


def _args(**over):
    """Arguments of dbw_images_resample_u8 with the pointers non-null (never dereferenced: each call below must fail validation, on the host)."""
    p = ctypes.c_void_p(256)
    a = dict(src=p, N=2, Hin=16, Win=24, Hout=8, Wout=12, table_x=p, table_y=p, out_f32=p, out_u8=None, workspace=p, workspace_bytes=1 << 20,
             form=0, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return list(a.values())


def test_images_resample_validates_before_any_launch():
    lib = _lib.load()
    f = lib.dbw_images_resample_u8
    assert f(*_args(src=None)) == -1 and b'null pointer' in lib.dbw_last_error()
    assert f(*_args(out_f32=None)) == -1 and b'at least one' in lib.dbw_last_error()
    for over in (dict(Hin=0), dict(Win=-2), dict(Hout=0), dict(Wout=0), dict(N=-1), dict(Hin=1 << 16, Win=1 << 16)):
        assert f(*_args(**over)) == -1 and b'bad size' in lib.dbw_last_error(), over
    assert f(*_args(table_x=None)) == -1 and b'table_x' in lib.dbw_last_error()
    assert f(*_args(table_y=None)) == -1 and b'table_y' in lib.dbw_last_error()
    for form in (-1, 3, 7):
        assert f(*_args(form=form)) == -1 and b'unknown form' in lib.dbw_last_error(), form
    # the general form needs its workspace, the fused one does not take every ratio
    need = lib.dbw_images_resample_workspace_bytes(2, 16, 24, 8, 12)
    assert need == 2 * 16 * 12 * 3
    for over in (dict(workspace=None), dict(workspace_bytes=need - 1)):
        assert f(*_args(form=_lib.RESAMPLE_GENERAL, **over)) == -1 and b'workspace' in lib.dbw_last_error(), over
    assert f(*_args(form=_lib.RESAMPLE_FUSED, Hin=400, Win=8, Hout=3, Wout=8, table_x=None)) == -2 and b'fused form' in lib.dbw_last_error()
    assert f(*_args(Hin=400, Win=24, Hout=3, Wout=12, workspace=None)) == -1 and b'workspace' in lib.dbw_last_error()      # auto -> general
    assert f(*_args(N=0)) == 0 and f(*_args(N=0, form=_lib.RESAMPLE_GENERAL)) == 0      # nothing to do is not an error, and launches nothing
    with pytest.raises(RuntimeError, match='unknown form'):
        _lib.call('dbw_images_resample_u8', *_args(form=9))


def test_resample_u8_has_no_cpu_path():
    with pytest.raises(RuntimeError, match='GPU'):
        ops.resample_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (4, 4))
    with pytest.raises(ValueError):
        ops.resample_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (4, 4), out='f16')
