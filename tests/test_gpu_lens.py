"""GPU tests of the lens rectification: ops.undistort_u8 (dbw_images_undistort_u8) against the host build of the same header
(tests/lens_ref.py, itself held to an fp64 restatement on the CPU by tests/test_host_lens_math.py), the custom-scene loader of
dbw_amd/dataset.py on a synthetic capture, and one run of the command line on it.  `-m gpu`.

Bounds: none.  The kernel and the host build compile one header with one rounding per fp32 operation (-ffp-contract=off, no division, no
library call): bytes are compared EXACTLY."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lens_ref as LR                                           # noqa: E402
import resample_ref as RR                                       # noqa: E402
from custom_fixture import write_capture                        # noqa: E402
from dbw_amd import _lib, ops, train                            # noqa: E402
from dbw_amd import dataset as DS                               # noqa: E402

DEV = 'cuda:0'
GUARD, PAD = 0xA5, 64


def _undistort_guarded(src, intr, dist, zoom, out_shift=0):
    """dbw_images_undistort_u8 on the arguments ops.undistort_u8 makes, with the output PAD (+ out_shift) bytes inside a buffer filled with
    GUARD, 64 bytes or more on each side: the output as numpy, after the guards were checked."""
    N, H, W, _ = src.shape
    n = N * H * W * 3
    buf = torch.full((n + 2 * PAD + out_shift,), GUARD, dtype=torch.uint8, device=DEV)
    out = buf[PAD + out_shift:PAD + out_shift + n]
    assert out.data_ptr() % 4 == out_shift % 4
    lens = ops.lens_params(intr, dist, zoom)
    _lib.call('dbw_images_undistort_u8', src.data_ptr(), N, H, W, lens.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:PAD + out_shift] == GUARD).all() and (host[PAD + out_shift + n:] == GUARD).all(), 'a byte outside the output was written'
    return host[PAD + out_shift:PAD + out_shift + n].reshape(N, H, W, 3)


@pytest.mark.parametrize('k', range(len(LR.COEFFS)))
@pytest.mark.parametrize('H,W', LR.SHAPES)
def test_undistort_u8_equals_the_host_build_byte_for_byte(H, W, k):
    intr, dist = LR.intrinsics(H, W), LR.COEFFS[k]
    zoom = DS.lens_zoom(H, W, intr, dist)
    a = LR.frames(3, H, W, seed=k)
    want = LR.undistort_host(a, intr, dist, zoom)
    src = torch.from_numpy(a).to(DEV)
    got = ops.undistort_u8(src, intr, dist, zoom)
    assert got.shape == (3, H, W, 3) and got.dtype == torch.uint8 and got.is_cuda and got.data_ptr() != src.data_ptr()
    n_diff = int((got.cpu().numpy() != want).sum())
    print(f'{H}x{W} set {k}, zoom {zoom:.4f}: {n_diff} of {want.size} bytes differ from the host build')
    assert n_diff == 0
    assert torch.equal(src.cpu(), torch.from_numpy(a))                                      # the source is left alone
    # the output between guards, its first byte at each of the four alignments: the same bytes, and none outside
    for shift in (0, 1, 2, 3):
        assert np.array_equal(_undistort_guarded(src, intr, dist, zoom, out_shift=shift), want), shift


@pytest.mark.parametrize('H,W', LR.SHAPES)
def test_a_source_sliced_at_one_byte_and_more_frames_than_a_lane_walks(H, W):
    """No source row dword aligned; 9 frames: three frame groups, a lane of the first walks three frames, one of the last a single one."""
    intr, dist = LR.intrinsics(H, W), LR.COEFFS[0]
    zoom = DS.lens_zoom(H, W, intr, dist)
    a = LR.frames(9, H, W, seed=11)
    flat = torch.zeros(a.size + 1, dtype=torch.uint8, device=DEV)
    flat[1:] = torch.from_numpy(a).reshape(-1).to(DEV)
    src = flat[1:].view(*a.shape)
    assert src.data_ptr() % 4 == 1
    want = LR.undistort_host(a, intr, dist, zoom)
    assert np.array_equal(ops.undistort_u8(src, intr, dist, zoom).cpu().numpy(), want)
    assert np.array_equal(_undistort_guarded(src, intr, dist, zoom, out_shift=3), want)
    # one frame, and a row of one ragged quad only (W = 3) / of exactly one quad (W = 4)
    assert np.array_equal(ops.undistort_u8(src[:1], intr, dist, zoom).cpu().numpy(), want[:1])
    for w in (3, 4, 2):
        b = LR.frames(2, 5, w, seed=w)
        i2 = LR.intrinsics(5, w)
        assert np.array_equal(_undistort_guarded(torch.from_numpy(b).to(DEV), i2, dist, 1.1, out_shift=1), LR.undistort_host(b, i2, dist, 1.1)), w


def test_a_row_wider_than_a_wave_and_than_a_block():
    """W = 263: 66 quads, the last ragged -- two waves per row, the dword across the wave boundary left to bytes; H = 6: two blocks of rows,
    the second half empty.  With no distortion and no zoom the frames come back as they are."""
    H, W = 6, 263
    intr, dist = LR.intrinsics(H, W), LR.COEFFS[2]
    a = LR.frames(2, H, W, seed=5)
    src = torch.from_numpy(a).to(DEV)
    for shift in (0, 1, 2, 3):
        assert np.array_equal(_undistort_guarded(src, intr, dist, 1.05, out_shift=shift), LR.undistort_host(a, intr, dist, 1.05)), shift
    assert np.array_equal(ops.undistort_u8(src, intr, (0.0,) * 6, 1.0).cpu().numpy(), a)


def test_errors_and_the_empty_batch():
    intr, dist = LR.intrinsics(8, 8), LR.COEFFS[0]
    assert ops.undistort_u8(torch.zeros(0, 8, 8, 3, dtype=torch.uint8, device=DEV), intr, dist).shape == (0, 8, 8, 3)
    with pytest.raises(TypeError):
        ops.undistort_u8(torch.zeros(1, 8, 8, 3, device=DEV), intr, dist)
    with pytest.raises(ValueError):
        ops.undistort_u8(torch.zeros(1, 3, 8, 8, dtype=torch.uint8, device=DEV), intr, dist)
    with pytest.raises(ValueError, match='2 x 2'):
        ops.undistort_u8(torch.zeros(1, 1, 8, 3, dtype=torch.uint8, device=DEV), intr, dist)
    src = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=DEV)
    lens = ops.lens_params(intr, dist)
    with pytest.raises(RuntimeError, match='overlap'):
        _lib.call('dbw_images_undistort_u8', src.data_ptr(), 2, 8, 8, lens.data_ptr(), src.data_ptr() + 8 * 8 * 3, None)


# ---- the scene loader -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def capture(tmp_path_factory):
    root = tmp_path_factory.mktemp('data')
    frames, _ = write_capture(root, 'desk', n=6, H=24, W=32, dist=LR.COEFFS[0], with_points=True)
    return root, frames


def test_custom_scene_views_are_rectified_then_resized(capture):
    root, frames = capture
    scene = DS.CustomScene(root, 'desk', 'train', downscale_factor=2)
    assert len(scene) == 6 and scene.img_size == (12, 16) and scene.zoom > 1.05
    views = scene.views(DEV, keep_raw=True, chunk=4)                            # two uploads: 4 + 2 frames
    assert set(views) == {'imgs', 'K', 'R', 'T', 'raw'} and all(v.is_cuda for v in views.values())
    raw = torch.from_numpy(frames)
    want = RR.resample_host(LR.undistort_host(raw, scene.intr, scene.dist, scene.zoom), (12, 16))
    assert views['imgs'].shape == (6, 3, 12, 16) and torch.equal(views['imgs'].cpu().view(torch.int32), want.view(torch.int32))
    assert torch.equal(views['raw'].cpu(), raw)                                 # what came off disk, not the rectified frames
    off = DS.CustomScene(root, 'desk', 'train', downscale_factor=2, undistort=False).views(DEV)
    assert torch.equal(off['imgs'].cpu().view(torch.int32), RR.resample_host(raw, (12, 16)).view(torch.int32))
    assert not torch.equal(off['imgs'], views['imgs'])


def test_the_command_line_trains_on_a_custom_scene(capture, tmp_path):
    import yaml
    root, _ = capture
    cfg = {'dataset': {'name': 'custom', 'tag': 'desk', 'downscale_factor': 2},
           'model': {'name': 'dbw', 'mesh': {'n_blocks': 2, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': 16},
                     'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                     'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True,
                                    'opacity_noise': False},
                     'loss': {'rgb_weight': 1, 'perceptual_weight': 0.1, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}},
           'training': {'batch_size': 2, 'n_epoches': 3, 'seed': 3, 'optimizer': {'name': 'adam', 'lr': 1e-3}, 'scheduler': {'name': 'multi_step'}}}
    path = tmp_path / 'desk.yml'
    with open(path, 'w') as f:
        yaml.safe_dump(cfg, f)
    scores = train.main(['--config', str(path), '--tag', 'run', '--data-root', str(root), '--runs-root', str(tmp_path / 'runs'),
                         '--no-perceptual', '--epochs', '1', '--device', DEV])
    print({k: v for k, v in scores.items() if not isinstance(v, dict)})
    # every score is finite but LPIPS, which quantitative_eval reports as NaN where no perceptual network is installed (--no-perceptual)
    assert all(np.isfinite(float(v)) for k, v in scores.items() if k != 'LPIPS' and not isinstance(v, dict)) and scores['PSNR'] > 0
    assert np.isnan(scores['LPIPS']) and {'n_blocks', 'L_tot', 'L_rec', 'PSNR', 'SSIM', 'alpha0', 'alpha1'} <= set(scores)
    run_dir = tmp_path / 'runs' / 'custom' / 'run'
    assert (run_dir / 'model.pkl').exists() and (run_dir / 'final_scores.tsv').exists()
    ckpt = torch.load(run_dir / 'model.pkl', map_location='cpu', weights_only=False)
    assert ckpt['model_name'] == 'dbw' and ckpt['epoch'] == 1
