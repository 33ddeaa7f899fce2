"""CPU tests of the scene parsing arithmetic (csrc/parse_math.h, the header scene_parse_kernel compiles) built for the host with g++
(tests/host_parse_math.cpp), against a few lines of numpy: the nearest rule and its ties, the coverage word up to bit 63, the counts of a
hand-made 4x4 picture, the label table of clipped faces and its validation; and of parse.SceneParse on hand-made tensors."""
import ctypes
import math

import numpy as np
import pytest
import torch

from dbw_amd import _lib
from dbw_amd.parse import SceneParse, default_palette
from host_build import host_lib


def lib():
    L = host_lib('parse_math')
    L.host_first_bad_label.restype = ctypes.c_longlong
    L.host_first_bad_label.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    L.host_clipped_labels.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p]
    L.host_parse_bit.restype = ctypes.c_ulonglong
    L.host_parse_covers.argtypes = [ctypes.c_ulonglong, ctypes.c_int]
    return L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def parse_pixels(ids, passed, pz, lab):
    """-> label (P) u8, depth (P) f32, cover (P) i64, face (P) i32, counts (64,2) i32 of the host build."""
    ids, passed, pz, lab = (np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(passed, np.uint8), np.ascontiguousarray(pz, np.float32),
                            np.ascontiguousarray(lab, np.int32))
    P, M = passed.shape
    assert pz.shape == (P, M) and ids.shape == (M,) and ids.max() < len(lab)
    label, depth, cover, face = np.empty(P, np.uint8), np.empty(P, np.float32), np.empty(P, np.int64), np.empty(P, np.int32)
    counts = np.empty((64, 2), np.int32)
    assert lib().host_parse_pixels(_p(ids), _p(passed), _p(pz), _p(lab), P, M, _p(label), _p(depth), _p(cover), _p(face), _p(counts)) == 0
    return label, depth, cover, face, counts


def numpy_parse(ids, passed, pz, lab):
    """The definition: nearest = minimum of (pz, face index) over the passing faces; cover = OR of 1 << label over them; counts = sums."""
    P, M = passed.shape
    label, depth, cover, face = np.full(P, 255, np.uint8), np.full(P, -1, np.float32), np.zeros(P, np.uint64), np.full(P, -1, np.int32)
    counts = np.zeros((64, 2), np.int32)
    for p in range(P):
        cand = sorted((float(pz[p, m]), int(ids[m])) for m in range(M) if passed[p, m])
        for _, f in cand:
            cover[p] |= np.uint64(1) << np.uint64(lab[f])
        if cand:
            depth[p], face[p] = cand[0]
            label[p] = lab[face[p]]
            counts[label[p], 1] += 1
        for l in range(64):
            counts[l, 0] += int((int(cover[p]) >> l) & 1)
    return label, depth, cover.view(np.int64), face, counts


def test_constants_are_the_headers():
    out = np.zeros(2, np.int32)
    lib().host_parse_constants(_p(out))
    assert out.tolist() == [_lib.VIZ_MAX_LABELS, _lib.VIZ_NO_LABEL] == [64, 255]


def test_nearest_rule_on_ties_in_either_arrival_order():
    """Equal pz: the lower face index wins, whether it arrives first (the kernels' order) or last; a nearer face wins whatever its index;
    -0.0 and +0.0 are one depth; a face that does not pass never wins, however near."""
    lab = np.arange(16) % 4
    cases = [([3, 7], [0.5, 0.5], 3), ([7, 3], [0.5, 0.5], 3), ([3, 7], [0.5, 0.25], 7), ([7, 3], [0.25, 0.5], 7),
             ([2, 5, 9], [0.75, 0.5, 0.5], 5), ([9, 5, 2], [0.5, 0.5, 0.75], 5), ([4, 1], [0.0, -0.0], 1), ([1, 4], [-0.0, 0.0], 1)]
    for ids, pz, want in cases:
        label, depth, cover, face, _ = parse_pixels(ids, np.ones((1, len(ids))), [pz], lab)
        ref = numpy_parse(np.array(ids), np.ones((1, len(ids)), bool), np.array([pz], np.float32) + 0.0, lab)
        assert face[0] == want == ref[3][0], (ids, pz)
        assert label[0] == lab[want] and depth[0] == np.float32(min(pz)) and cover[0] == ref[2][0]
    # the near face fails the inside test: it is neither the nearest nor in the word
    label, depth, cover, face, counts = parse_pixels([0, 1, 2], [[0, 1, 1]], [[0.1, 0.6, 0.4]], [5, 6, 7])
    assert face[0] == 2 and label[0] == 7 and depth[0] == np.float32(0.4) and cover[0] == (1 << 6) | (1 << 7)
    # nothing passes
    label, depth, cover, face, counts = parse_pixels([0, 1], [[0, 0]], [[0.1, 0.6]], [5, 6])
    assert label[0] == 255 and depth[0] == -1 and cover[0] == 0 and face[0] == -1 and not counts.any()


def test_coverage_words_reach_bit_63():
    for l in (0, 31, 32, 63):
        assert lib().host_parse_bit(l) == 1 << l
        assert lib().host_parse_covers(1 << l, l) == 1 and lib().host_parse_covers(~(1 << l) & (2 ** 64 - 1), l) == 0
    lab = [0, 31, 32, 63]
    label, depth, cover, face, counts = parse_pixels([0, 1, 2, 3], [[1, 1, 1, 1], [0, 0, 0, 1], [1, 0, 1, 0], [0, 1, 0, 0]],
                                                     [[0.4, 0.3, 0.2, 0.1], [0.4, 0.3, 0.2, 0.1], [0.4, 0.3, 0.2, 0.1], [0.4, 0.3, 0.2, 0.1]], lab)
    want = [(1 << 0) | (1 << 31) | (1 << 32) | (1 << 63), 1 << 63, (1 << 0) | (1 << 32), 1 << 31]
    assert [int(c) & (2 ** 64 - 1) for c in cover] == want
    assert cover[0] < 0 and cover[1] == -2 ** 63 and cover[2] > 0            # the sign bit of the int64 is label 63
    assert label.tolist() == [63, 63, 32, 31]
    assert counts[[0, 31, 32, 63]].tolist() == [[2, 0], [2, 1], [2, 1], [2, 2]] and counts.sum() == 12


def test_counts_of_a_hand_made_4x4_picture():
    """Three faces over 16 pixels: a ground (label 1) everywhere at depth 0.9, block A (label 2) on the left 2 columns at 0.5, block B
    (label 63) on the middle 2 columns at 0.7 -- B hides behind A on column 1."""
    passed = np.zeros((16, 3), np.uint8)
    passed[:, 0] = 1
    for p in range(16):
        x = p % 4
        passed[p, 1] = x < 2
        passed[p, 2] = 1 <= x < 3
    pz = np.tile(np.array([0.9, 0.5, 0.7], np.float32), (16, 1))
    lab = [1, 2, 63]
    got = parse_pixels([0, 1, 2], passed, pz, lab)
    ref = numpy_parse(np.arange(3), passed, pz, lab)
    for g, r in zip(got, ref):
        assert np.array_equal(g, r)
    counts = got[4]
    assert counts[1].tolist() == [16, 4] and counts[2].tolist() == [8, 8] and counts[63].tolist() == [8, 4]
    assert counts.sum() == 16 + 4 + 8 + 8 + 8 + 4
    # and a random one: 64 labels, 40 faces, a third of the pairs pass, depths drawn from 8 values so that ties are common
    rng = np.random.default_rng(7)
    M, P = 40, 64
    lab = rng.integers(0, 64, 100)
    ids = np.sort(rng.choice(100, M, replace=False))
    passed, pz = rng.random((P, M)) < 0.33, rng.integers(1, 9, (P, M)).astype(np.float32) / 8
    for order in (np.arange(M), rng.permutation(M)):
        got = parse_pixels(ids[order], passed[:, order], pz[:, order], lab)
        ref = numpy_parse(ids[order], passed[:, order], pz[:, order], lab)
        for g, r in zip(got, ref):
            assert np.array_equal(g, r)


def test_label_table_of_clipped_faces_and_its_validation():
    face_label = np.array([0, 1, 63, 7], np.int32)
    c2o = np.array([3, 3, 0, 2, 1, 1, 2, 0], np.int32)
    out = np.empty(8, np.int32)
    lib().host_clipped_labels(_p(face_label), _p(c2o), 8, 4, _p(out))
    assert out.tolist() == face_label[c2o].tolist()
    lib().host_clipped_labels(_p(face_label), None, 8, 4, _p(out))                      # unclipped: the views' faces one after the other
    assert out.tolist() == face_label.tolist() * 2
    wild = np.array([4, -1, 2 ** 31 - 1, -2 ** 31], np.int32)                           # unused rows hold anything: folded into the table
    lib().host_clipped_labels(_p(face_label), _p(wild), 4, 4, _p(out[:4]))
    assert out[:4].tolist() == [0, 7, 7, 0]
    assert lib().host_first_bad_label(_p(face_label), 4) == -1
    for bad in (64, -1, 255, -2 ** 31):
        t = np.array([0, 63, bad, 64], np.int32)
        assert lib().host_first_bad_label(_p(t), 4) == 2
        assert lib().host_first_bad_label(_p(t), 2) == -1


def _hand_parse():
    """2 views of 2x3 pixels, 62 blocks: block 61 is label 63, the sign bit of the word."""
    label = torch.tensor([[[0, 1, 2], [63, 63, 255]], [[1, 1, 1], [3, 2, 0]]], dtype=torch.uint8)
    bit = lambda *ls: sum(1 << l for l in ls) - (1 << 64 if 63 in ls else 0)          # noqa: E731  (as the int64 the kernel stores)
    cover = torch.tensor([[[bit(0), bit(0, 1), bit(0, 1, 2, 63)], [bit(1, 63), bit(63), 0]],
                          [[bit(1), bit(1, 3), bit(1, 2, 3)], [bit(1, 3), bit(1, 2), bit(0)]]], dtype=torch.int64)
    depth = torch.where(label == 255, torch.tensor(-1.0), torch.tensor(2.5))
    counts = torch.zeros(2, 64, 2, dtype=torch.int32)
    for v in range(2):
        for l in range(64):
            counts[v, l, 0] = int(((cover[v] >> l) & 1).sum())
            counts[v, l, 1] = int((label[v] == l).sum())
    return SceneParse(label, depth, cover, counts, 62, palette=default_palette(torch.rand(62, 3, generator=torch.Generator().manual_seed(1))))


def test_scene_parse_methods_on_hand_made_tensors():
    sp = _hand_parse()
    assert sp.cover[0, 0, 2] < 0 and sp.cover[0, 1, 1] == -2 ** 63
    assert sp.amodal(61).tolist() == [[[False, False, True], [True, True, False]], [[False] * 3, [False] * 3]]          # label 63
    assert sp.modal(61).tolist() == [[[False, False, False], [True, True, False]], [[False] * 3, [False] * 3]]
    assert sp.amodal(0).tolist() == [[[False, False, True], [False] * 3], [[False, False, True], [False, True, False]]]
    assert sp.modal(0).tolist() == [[[False, False, True], [False] * 3], [[False] * 3, [False, True, False]]]
    assert sp.amodal(1).sum() == 3 and sp.modal(1).sum() == 1
    assert sp.foreground().tolist() == [[[False, False, True], [True, True, False]], [[False] * 3, [True, True, False]]]
    amodal, visible = sp.areas()
    assert amodal.shape == (2, 62) and amodal[:, [0, 1, 61]].tolist() == [[1, 0, 3], [2, 3, 0]] and visible[:, [0, 1, 61]].tolist() == [[1, 0, 2], [1, 1, 0]]
    occ = sp.occlusion()
    assert occ.shape == (2, 62)
    assert occ[0, 0] == 0 and math.isnan(float(occ[0, 1])) and float(occ[0, 61]) == pytest.approx(1 / 3, abs=1e-12)
    assert float(occ[1, 0]) == 0.5 and float(occ[1, 1]) == pytest.approx(2 / 3, abs=1e-12) and math.isnan(float(occ[1, 61]))
    assert int(torch.isnan(occ).sum()) == 2 * 62 - 4
    for k in (-1, 62):
        with pytest.raises(IndexError):
            sp.amodal(k)
    with pytest.raises(ValueError, match='below 64'):
        SceneParse(sp.label, sp.depth, sp.cover, sp.counts, 63)
    img = sp.colors()
    assert img.shape == (2, 3, 2, 3) and img.dtype == torch.float32
    assert torch.equal(img[0, :, 0, 2], sp.palette[2]) and torch.equal(img[0, :, 1, 0], sp.palette[63]) and torch.equal(img[0, :, 1, 2], torch.ones(3))
    assert img[0, :, 0, 0].tolist() == pytest.approx([0.85] * 3) and img[0, :, 0, 1].tolist() == pytest.approx([0.55] * 3)      # the env in grey
    own = torch.zeros(4, 3)
    own[2] = torch.tensor([1., 0., 0.])
    assert sp.colors(own)[0, :, 0, 2].tolist() == [1, 0, 0] and sp.colors(own)[0, :, 1, 0].tolist() == [1, 1, 1]              # labels past the table: white


def test_write_parse_files(tmp_path):
    from dbw_amd import export
    sp = _hand_parse()
    written = export.write_parse(sp, tmp_path / 'parse')
    names = sorted(p.name for p in (tmp_path / 'parse').iterdir())
    assert names == sorted(['block_visibility.tsv'] + [f'{n}_{v:03d}.{e}' for v in range(2) for n, e in (('label', 'png'), ('depth', 'npy'), ('cover', 'npy'))])
    assert sorted(written) == sorted(str(tmp_path / 'parse' / n) for n in names)
    for v in range(2):
        assert np.array_equal(np.load(tmp_path / 'parse' / f'cover_{v:03d}.npy'), sp.cover[v].numpy())
        d = np.load(tmp_path / 'parse' / f'depth_{v:03d}.npy')
        assert d.dtype == np.float32 and np.array_equal(d, sp.depth[v].numpy())
    from PIL import Image
    png = np.asarray(Image.open(tmp_path / 'parse' / 'label_000.png'))
    assert png.shape == (2, 3, 3) and png[1, 2].tolist() == [255, 255, 255] and png[0, 0].tolist() == [int(0.85 * 255)] * 3
    rows = [line.rstrip('\n').split('\t') for line in open(tmp_path / 'parse' / 'block_visibility.tsv')]
    assert rows[0] == ['block', 'kept', 'amodal_0', 'visible_0', 'occlusion_0', 'amodal_1', 'visible_1', 'occlusion_1'] and len(rows) == 63
    assert rows[1] == ['0', '1', '1', '1', '0.00000', '2', '1', '0.50000'] and rows[2] == ['1', '1', '0', '0', 'nan', '3', '1', '0.66667']
    assert rows[62] == ['61', '1', '3', '2', '0.33333', '0', '0', 'nan']
    both = export.join_parses([sp, sp])
    assert both.label.shape[0] == 4 and torch.equal(both.cover[2:], sp.cover) and both.n_blocks == 62
