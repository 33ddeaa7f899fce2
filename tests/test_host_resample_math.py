"""CPU tests of the arithmetic of the image ingest (csrc/resample_math.h, the header the resample kernels compile) built for the host with
g++ -ffp-contract=off (tests/host_resample_math.cpp):
  * the two-pass resample reproduces tests/golden/resample_pil.npz -- the bytes Pillow's BILINEAR resize makes of the same seeded inputs
    (tests/golden/make_resample_golden.py) -- BIT FOR BIT, and live Pillow where it imports, the 1200x1600 -> 300x400 DTU shape included
    there; integer arithmetic on both sides, so there is no tolerance;
  * the coefficient tables equal a float64 restatement of Pillow's rule;
  * the fp32 conversion equals torch's uint8 -> float -> div(255) on all 256 values, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import resample_ref as RR

try:
    import PIL  # noqa: F401
    HAS_PIL = True
except ImportError:
    HAS_PIL = False


@pytest.fixture(scope='module')
def golden():
    return np.load(RR.GOLDEN)


def test_the_fixture_holds_every_shape(golden):
    assert set(golden.files) == set(RR.SHAPES) | {'pillow_version'}
    for tag, (_, size) in RR.SHAPES.items():
        assert golden[tag].shape == (*size, 3) and golden[tag].dtype == np.uint8, tag
    # the hard cases are in it: both ends of the byte range, one ratio of exactly 4, several tiles with odd remainders, one axis only
    assert golden['zeros'].max() == 0 and golden['ones'].min() == 255 and len(np.unique(golden['up'])) > 200


@pytest.mark.parametrize('tag', sorted(RR.SHAPES))
def test_resample_equals_pillow_byte_for_byte(golden, tag):
    a = RR.make_input(tag)
    size = RR.SHAPES[tag][1]
    f32, u8 = RR.resample_host(torch.from_numpy(a)[None], size, out='both')
    n_diff = int((u8[0].numpy() != golden[tag]).sum())
    print(f'{tag}: {a.shape[:2]} -> {size}: {n_diff} bytes differ from the fixture')
    assert n_diff == 0
    assert torch.equal(f32[0], RR.to_tensor(golden[tag]))                                  # the ToTensor layout and values
    if HAS_PIL:
        assert np.array_equal(u8[0].numpy(), RR.pil_resize(a, size)), 'live Pillow'
    # a batch: every image on its own
    if a.size < 50000:
        b = np.stack([a, a[::-1, ::-1].copy(), 255 - a])
        got = RR.resample_host(torch.from_numpy(b), size, out='u8')
        assert np.array_equal(got[0].numpy(), golden[tag])
        if HAS_PIL:
            assert all(np.array_equal(got[i].numpy(), RR.pil_resize(b[i], size)) for i in (1, 2))


@pytest.mark.skipif(not HAS_PIL, reason='the DTU shape is too large for a fixture: compared with live Pillow only')
def test_the_dtu_shape_equals_live_pillow():
    a = np.random.RandomState(24).randint(0, 256, (1200, 1600, 3)).astype(np.uint8)
    got = RR.resample_host(torch.from_numpy(a)[None], (300, 400), out='u8')[0].numpy()
    assert np.array_equal(got, RR.pil_resize(a, (300, 400)))


@pytest.mark.parametrize('in_size,out_size', [(1600, 400), (1200, 300), (768, 768), (960, 480), (37, 9), (53, 13), (40, 13), (64, 17), (16, 40),
                                              (24, 50), (31, 8), (23, 7), (48, 12), (150, 37), (260, 65), (400, 3), (1, 5), (5, 1)])
def test_table_rows_equal_the_double_precision_restatement(in_size, out_size):
    t, want = RR.table_host(in_size, out_size), RR.table_numpy(in_size, out_size)
    assert t.shape == want.shape and np.array_equal(t, want)
    xmin, n, k = t[:, 0], t[:, 1], t[:, 2:]
    assert (xmin >= 0).all() and (n >= 1).all() and (xmin + n <= in_size).all() and (n <= k.shape[1]).all()
    assert (np.diff(xmin) >= 0).all() and (np.diff(xmin + n) >= 0).all()                   # what the kernels' tile extents rely on
    assert (k >= 0).all() and (np.abs(k.sum(1).astype(np.int64) - (1 << 22)) <= n).all()   # each weight is off by at most half a unit
    assert all((k[i, n[i]:] == 0).all() for i in range(out_size))                          # zero padded
    if in_size == out_size:
        # an axis that keeps its size is the identity (its second tap weighs nothing): skipping it changes no byte
        assert (xmin == np.arange(in_size)).all() and (k[:, 0] == 1 << 22).all() and (k[:, 1:] == 0).all()


def test_table_refuses_bad_sizes_and_a_small_capacity():
    L = RR.lib()
    buf = np.zeros(16, np.int32)
    p = ctypes.c_void_p(buf.ctypes.data)
    assert L.host_resample_table(0, 4, None, ctypes.c_longlong(0)) < 0 and L.host_resample_table(4, -1, None, ctypes.c_longlong(0)) < 0
    assert L.host_resample_table(8, 4, None, ctypes.c_longlong(0)) == 5
    assert L.host_resample_table(8, 4, p, ctypes.c_longlong(16)) < 0 and (buf == 0).all()    # 4 rows of 7 do not fit


def test_clamp_and_rounding_constant():
    acc = np.array([0, (1 << 22) - 1, 1 << 22, 255 << 22, (256 << 22) - 1, 256 << 22, 2**31 - 1, -1, -(1 << 22), (1 << 21) + 127 * (1 << 22)],
                   np.int32)
    out = np.zeros(len(acc), np.uint8)
    assert RR.lib().host_resample_clip8(ctypes.c_void_p(acc.ctypes.data), ctypes.c_longlong(len(acc)), ctypes.c_void_p(out.ctypes.data)) == 0
    assert out.tolist() == [0, 0, 1, 255, 255, 255, 255, 0, 0, 127]


def test_to_float_equals_torch_on_all_256_values():
    v = torch.arange(256, dtype=torch.uint8)
    out = torch.empty(256)
    assert RR.lib().host_resample_to_float(ctypes.c_void_p(v.data_ptr()), ctypes.c_longlong(256), ctypes.c_void_p(out.data_ptr())) == 0
    assert torch.equal(out.view(torch.int32), torch.from_numpy(v.numpy()).float().div(255).view(torch.int32))
