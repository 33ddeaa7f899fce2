"""GPU tests of the per-frame rectification: ops.rectify_u8 / ops.rectify_valid_u8 (dbw_lens_rectify_u8, dbw_lens_rectify_valid_u8) against
the host build of the same header (tests/rectify_ref.py, itself held to an fp64 restatement on the CPU by
tests/test_host_rectify_math.py), dataset.CustomScene(cameras='per_frame') on a synthetic fisheye capture with per-frame intrinsics, and
one run of the command line on it.  `-m gpu`.

Bounds: none.  The kernel and the host build compile one header with one rounding per fp32 operation (-ffp-contract=off; the division and
the square root of the fisheye map are rounded correctly in both builds, the arctangent is written in the header): bytes are compared
EXACTLY."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lens_ref as LR                                           # noqa: E402
import rectify_ref as RF                                        # noqa: E402
import resample_ref as RR                                       # noqa: E402
from dbw_amd import _lib, ops, train                            # noqa: E402
from dbw_amd import dataset as DS                               # noqa: E402

DEV = 'cuda:0'
GUARD, PAD = 0xA5, 64


def _rectify_guarded(src, rows, target, out_shift=0):
    """dbw_lens_rectify_u8 with the output PAD (+ out_shift) bytes inside a buffer filled with GUARD, 64 bytes or more on each side: the
    return code, the output as numpy and whether every guard byte is intact."""
    N, H, W, _ = src.shape
    n = N * H * W * 3
    buf = torch.full((n + 2 * PAD + out_shift,), GUARD, dtype=torch.uint8, device=DEV)
    out = buf[PAD + out_shift:PAD + out_shift + n]
    assert out.data_ptr() % 4 == out_shift % 4
    rows, target = torch.as_tensor(rows).contiguous(), torch.as_tensor(target).contiguous()
    rc = _lib.load().dbw_lens_rectify_u8(src.data_ptr(), N, H, W, rows.data_ptr(), target.data_ptr(), out.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    intact = bool((host[:PAD + out_shift] == GUARD).all() and (host[PAD + out_shift + n:] == GUARD).all())
    return rc, host[PAD + out_shift:PAD + out_shift + n].reshape(N, H, W, 3), intact


@pytest.mark.parametrize('k', range(3))
@pytest.mark.parametrize('model', (RF.RADTAN, RF.FISHEYE))
@pytest.mark.parametrize('H,W', RF.SHAPES)
def test_rectify_u8_equals_the_host_build_byte_for_byte(H, W, model, k):
    dist = RF.coeff_sets(model)[k]
    a = LR.frames(5, H, W, seed=k)
    src = torch.from_numpy(a).to(DEV)
    for zoom in (1.0, 1.14):                                    # the zoom of lens='mask', where camera C reads outside, and one near the crop's
        rows, target = RF.five_frames(H, W, model, dist, zoom)
        want = RF.rectify_host(a, rows, target)
        got = ops.rectify_u8(src, torch.from_numpy(rows), torch.from_numpy(target))
        assert got.shape == (5, H, W, 3) and got.dtype == torch.uint8 and got.is_cuda and got.data_ptr() != src.data_ptr()
        n_diff = int((got.cpu().numpy() != want).sum())
        print(f'{H}x{W} model {model} set {k} zoom {zoom}: {n_diff} of {want.size} bytes differ from the host build')
        assert n_diff == 0
        assert torch.equal(src.cpu(), torch.from_numpy(a))                                  # the source is left alone
        # the output between guards, its first byte at each of the four alignments: the same bytes, and none outside
        for shift in (0, 1, 2, 3):
            rc, out, intact = _rectify_guarded(src, rows, target, out_shift=shift)
            assert rc == 0 and intact and np.array_equal(out, want), shift
    # a source sliced at one byte: no source row dword aligned
    flat = torch.zeros(a.size + 1, dtype=torch.uint8, device=DEV)
    flat[1:] = src.reshape(-1)
    off = flat[1:].view(*a.shape)
    assert off.data_ptr() % 4 == 1
    rc, out, intact = _rectify_guarded(off, rows, target, out_shift=3)
    assert rc == 0 and intact and np.array_equal(out, want)


@pytest.mark.parametrize('k', range(len(LR.COEFFS)))
@pytest.mark.parametrize('H,W', RF.SHAPES)
def test_equal_radial_tangential_cameras_give_the_bytes_of_undistort_u8(H, W, k):
    intr, dist = LR.intrinsics(H, W), LR.COEFFS[k]
    zoom = DS.lens_zoom(H, W, intr, dist)
    src = torch.from_numpy(LR.frames(5, H, W, seed=k)).to(DEV)
    got = ops.rectify_u8(src, ops.lens_table([intr] * 5, [dist] * 5, [0] * 5), ops.lens_target(intr, zoom))
    assert torch.equal(got, ops.undistort_u8(src, intr, dist, zoom))
    valid = ops.rectify_valid_u8(H, W, ops.lens_table([intr] * 2, [dist] * 2, [0] * 2), ops.lens_target(intr, 1.0), device=DEV)
    assert torch.equal(valid[0], ops.lens_valid_u8(H, W, intr, dist, 1.0, device=DEV)) and torch.equal(valid[0], valid[1])


@pytest.mark.parametrize('model', (RF.RADTAN, RF.FISHEYE))
def test_more_frames_than_a_launch_takes_and_a_permuted_chunk(model):
    """33 frames of 5x8: a launch carries the rows of 32 frames, the last frame goes out in a launch of its own with the pointers moved on.
    The same chunk in another order with the rows permuted alike gives the frames in that order."""
    H, W, N = 5, 8, 33
    cams = list(RF.cameras(H, W).values())
    sets = RF.coeff_sets(model)
    intrs, dists = [cams[n % 4] for n in range(N)], [sets[n % 3] for n in range(N)]
    rows, target = RF.table(intrs, dists, [model] * N), RF.target(RF.median_target(H, W), 1.05)
    a = LR.frames(N, H, W, seed=2)
    want = RF.rectify_host(a, rows, target)
    src = torch.from_numpy(a).to(DEV)
    rc, out, intact = _rectify_guarded(src, rows, target, out_shift=1)
    assert rc == 0 and intact and np.array_equal(out, want)
    assert np.array_equal(ops.rectify_valid_u8(H, W, torch.from_numpy(rows), torch.from_numpy(target), device=DEV).cpu().numpy(),
                          RF.valid_host(H, W, rows, target))
    perm = np.random.RandomState(0).permutation(N)
    got = ops.rectify_u8(src[torch.from_numpy(perm).to(DEV)], torch.from_numpy(rows[perm]), torch.from_numpy(target))
    assert np.array_equal(got.cpu().numpy(), want[perm])


def test_narrow_rows_and_a_row_wider_than_a_wave():
    """W = 2, 3, 4: a row of one ragged quad / of exactly one quad.  6x263: 66 quads, the last ragged -- two waves per row, the dword across
    the wave boundary left to bytes; two blocks of rows, the second half empty."""
    for H, W in ((5, 2), (5, 3), (5, 4), (6, 263)):
        cams = RF.cameras(H, W)
        intrs = [cams[c] for c in ('A', 'B', 'C')]
        a = LR.frames(3, H, W, seed=W)
        src = torch.from_numpy(a).to(DEV)
        for model in (RF.RADTAN, RF.FISHEYE):
            rows, target = RF.table(intrs, [RF.coeff_sets(model)[1]] * 3, [model] * 3), RF.target(cams['A'], 1.05)
            want = RF.rectify_host(a, rows, target)
            for shift in (0, 1, 2, 3):
                rc, out, intact = _rectify_guarded(src, rows, target, out_shift=shift)
                assert rc == 0 and intact and np.array_equal(out, want), (H, W, model, shift)


@pytest.mark.parametrize('H,W', RF.SHAPES)
def test_rectify_valid_u8_equals_the_host_maps(H, W):
    for model in (RF.RADTAN, RF.FISHEYE):
        for dist in RF.coeff_sets(model):
            rows, target = RF.five_frames(H, W, model, dist, 1.0)
            got = ops.rectify_valid_u8(H, W, torch.from_numpy(rows), torch.from_numpy(target), device=DEV)
            assert got.shape == (5, H, W) and got.dtype == torch.uint8
            want = RF.valid_host(H, W, rows, target)
            assert np.array_equal(got.cpu().numpy(), want) and set(np.unique(want)) <= {0, 255}
            if model == RF.FISHEYE:
                assert 0.8 < (want[2] == 255).mean() < 0.9 and (want[1] == 255).all()       # camera C leaves a border, B none
    nan = RF.five_frames(H, W, RF.FISHEYE, RF.coeff_sets(RF.FISHEYE)[0])[0]
    nan[3, 5] = np.nan
    with pytest.raises(RuntimeError, match='not finite'):
        ops.rectify_valid_u8(H, W, torch.from_numpy(nan), ops.lens_target(RF.median_target(H, W)), device=DEV)


def test_refusals_arrive_before_any_launch():
    H, W = RF.SHAPES[0]
    a = LR.frames(5, H, W, seed=1)
    src = torch.from_numpy(a).to(DEV)
    good, target = RF.five_frames(H, W, RF.FISHEYE, RF.coeff_sets(RF.FISHEYE)[0])
    lib = _lib.load()

    def refused(rows, tgt, text):
        rc, out, intact = _rectify_guarded(src, rows, tgt)
        assert rc == -1 and text in lib.dbw_last_error(), (rc, lib.dbw_last_error())
        assert intact and (out == GUARD).all() and torch.equal(src.cpu(), torch.from_numpy(a))

    for col in (0, 3, 7, 13):                                                               # (the padding too)
        bad = good.copy()
        bad[4, col] = np.nan
        refused(bad, target, b'not finite')
    bad = good.copy()
    bad[2, 6] = np.inf
    refused(bad, target, b'not finite')
    bad = good.copy()
    bad[1, 0] = 2.0
    refused(bad, target, b'model id')
    bad[1, 0] = 0.5
    refused(bad, target, b'model id')
    for col in (1, 2):
        bad = good.copy()
        bad[3, col] = 0.0
        refused(bad, target, b'focal length')
    bad_t = target.copy()
    bad_t[2] = np.nan
    refused(good, bad_t, b'not finite')
    bad_t[2] = 0.0
    refused(good, bad_t, b'not positive')
    rows, tgt = torch.from_numpy(good), torch.from_numpy(target)
    n = a.size
    for out_ptr in (src.data_ptr(), src.data_ptr() + n - 1, src.data_ptr() - n + 1):
        with pytest.raises(RuntimeError, match='overlap'):
            _lib.call('dbw_lens_rectify_u8', src.data_ptr(), 5, H, W, rows.data_ptr(), tgt.data_ptr(), out_ptr, None)
    assert torch.equal(src.cpu(), torch.from_numpy(a))
    # the binding's own checks, those of undistort_u8
    assert ops.rectify_u8(torch.zeros(0, 8, 8, 3, dtype=torch.uint8, device=DEV), torch.zeros(0, 16), tgt).shape == (0, 8, 8, 3)
    with pytest.raises(TypeError):
        ops.rectify_u8(torch.zeros(5, 8, 8, 3, device=DEV), rows, tgt)
    with pytest.raises(ValueError):
        ops.rectify_u8(torch.zeros(5, 3, 8, 8, dtype=torch.uint8, device=DEV), rows, tgt)
    with pytest.raises(ValueError, match='2 x 2'):
        ops.rectify_u8(torch.zeros(5, 1, 8, 3, dtype=torch.uint8, device=DEV), rows, tgt)
    with pytest.raises(ValueError, match='table_rows'):
        ops.rectify_u8(src, rows[:4], tgt)
    with pytest.raises(RuntimeError, match='GPU'):
        ops.rectify_u8(torch.zeros(5, 8, 8, 3, dtype=torch.uint8), rows, tgt)


# ---- the scene loader -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def capture(tmp_path_factory):
    root = tmp_path_factory.mktemp('data')
    frames, intrs, dists, models = RF.write_fisheye_capture(root, 'rig', with_points=True)
    return root, frames, intrs, dists, models


@pytest.mark.parametrize('lens', ['crop', 'mask'])
def test_a_fisheye_scene_with_per_frame_intrinsics(capture, lens):
    root, frames, intrs, dists, models = capture
    scene = DS.CustomScene(root, 'rig', 'train', downscale_factor=2, cameras='per_frame', lens=lens)
    tgt = tuple(float(v) for v in np.median(intrs, axis=0))
    zoom = DS.rectify_zoom(24, 32, intrs, dists, models, tgt) if lens == 'crop' else 1.0
    assert len(scene) == 6 and scene.img_size == (12, 16) and scene.intr == tgt and scene.zoom == zoom and (zoom > 1.1) == (lens == 'crop')
    views = scene.views(DEV, keep_raw=True, chunk=4)                            # two uploads: 4 + 2 frames
    assert set(views) == {'imgs', 'K', 'R', 'T', 'raw'} | ({'masks'} if lens == 'mask' else set()) and all(v.is_cuda for v in views.values())
    rows, t32 = RF.table(intrs, dists, models), RF.target(tgt, zoom)
    raw = torch.from_numpy(frames)
    want = RR.resample_host(RF.rectify_host(raw, rows, t32), (12, 16))
    assert views['imgs'].shape == (6, 3, 12, 16) and torch.equal(views['imgs'].cpu().view(torch.int32), want.view(torch.int32))
    assert torch.equal(views['raw'].cpu(), raw)
    # K is the target's: one matrix for all views, built by the lines of the shared mode (half the shorter side is the unit)
    K = views['K'].cpu()
    assert all(torch.equal(K[0], K[v]) for v in range(6))
    want_K = torch.tensor([zoom * tgt[0] / 12.0, zoom * tgt[1] / 12.0, -(tgt[2] - 16.0) / 12.0, -(tgt[3] - 12.0) / 12.0], dtype=torch.float64).float()
    assert torch.equal(torch.stack([K[0, 0, 0], K[0, 1, 1], K[0, 0, 2], K[0, 1, 2]]), want_K)
    if lens == 'mask':
        valid = RF.valid_host(24, 32, rows, t32)
        warped = RF.rectify_host(np.full((6, 24, 32, 3), 255, np.uint8), rows, t32) & valid[..., None]
        small = RR.resample_host(torch.from_numpy(warped), (12, 16), out='u8')
        want_masks = (small[..., 0] == 255).to(torch.float32)[:, None]
        assert torch.equal(views['masks'].cpu(), want_masks) and 0 < float(want_masks[2].mean()) < 1 and float(want_masks[1].mean()) == 1


def test_the_command_line_trains_on_per_frame_cameras(capture, tmp_path):
    import yaml
    root = capture[0]
    cfg = {'dataset': {'name': 'custom', 'tag': 'rig', 'downscale_factor': 2, 'cameras': 'per_frame', 'lens': 'mask'},
           'model': {'name': 'dbw', 'mesh': {'n_blocks': 2, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': 16},
                     'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                     'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True,
                                    'opacity_noise': False},
                     'loss': {'rgb_weight': 1, 'perceptual_weight': 0.1, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}},
           'training': {'batch_size': 2, 'n_epoches': 3, 'seed': 3, 'optimizer': {'name': 'adam', 'lr': 1e-3}, 'scheduler': {'name': 'multi_step'}}}
    path = tmp_path / 'rig.yml'
    with open(path, 'w') as f:
        yaml.safe_dump(cfg, f)
    scores = train.main(['--config', str(path), '--tag', 'run', '--data-root', str(root), '--runs-root', str(tmp_path / 'runs'),
                         '--no-perceptual', '--epochs', '1', '--device', DEV])
    print({k: v for k, v in scores.items() if not isinstance(v, dict)})
    # every score is finite but LPIPS, which quantitative_eval reports as NaN where no perceptual network is installed (--no-perceptual)
    assert all(np.isfinite(float(v)) for k, v in scores.items() if k != 'LPIPS' and not isinstance(v, dict)) and scores['PSNR'] > 0
    assert np.isnan(scores['LPIPS']) and (tmp_path / 'runs' / 'custom' / 'run' / 'model.pkl').exists()
