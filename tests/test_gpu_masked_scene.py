"""GPU tests of the validity masks a scene hands to the trainer: dataset.ImageStore's masks, CustomScene(masks=, lens=),
DTUScene(masks=) and dbw_lens_valid_u8.

Captures of 6 frames of 24 x 32 through the three test lenses (tests/lens_ref.py), written with custom_fixture.write_capture; the mask
PNGs are written here and named by each frame's mask_path.  views()['masks'] of CustomScene(masks=True, lens='mask') is byte-equal to the
restatement on the host: the mask expanded to three channels through lens_ref.undistort_host at zoom 1, ANDed with the host build of the
lens predicate (masked_loss_ref.lens_valid_host), then Pillow's resize, valid where the byte is 255.  lens='mask' keeps zoom == 1 and K
accordingly; a frame without mask_path is valid wherever the lens is; the defaults return no 'masks' key and the bytes of today's imgs;
a mask/ folder under a DTU-layout scene is read with masks=True."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import lens_ref as LR
import masked_loss_ref as MR
import resample_ref as RR
from custom_fixture import write_capture
from dataset_fixture import write_scene
from dbw_amd import dataset as DS, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N, H, W = 6, 24, 32
NO_MASK = 4                                          # the frame whose entry has no mask_path


def _mask_image(i):
    """(H,W) uint8: a photographer's shadow that moves with the frame, and a grey value that counts as valid (nonzero)."""
    a = np.full((H, W), 255, np.uint8)
    a[6 + i:15 + i, 3 * i:3 * i + 9] = 0
    a[0:3, 20:30] = 90
    return a


@pytest.fixture(scope='module', params=range(len(LR.COEFFS)), ids=['pincushion', 'barrel', 'mixed'])
def capture(request, tmp_path_factory):
    dist = LR.COEFFS[request.param]
    root = tmp_path_factory.mktemp(f'masked{request.param}')
    per_frame = {i: {'mask_path': f'masks/mask_{i + 1:05d}.png'} for i in range(N) if i != NO_MASK}
    frames, _ = write_capture(root, 'desk', n=N, H=H, W=W, dist=dist, per_frame=per_frame)
    os.makedirs(os.path.join(str(root), 'custom', 'desk', 'masks'))
    for i in per_frame:
        Image.fromarray(_mask_image(i), 'L').save(os.path.join(str(root), 'custom', 'desk', per_frame[i]['mask_path']))
    return root, frames, dist


def _host_masks(scene, size, zoom, with_files=True, with_lens=True):
    """The restatement on the host -> (N,1,h,w) fp32."""
    valid = MR.lens_valid_host(H, W, LR.lens_array(scene.intr, scene.dist, 1.0)) if with_lens else np.full((H, W), 255, np.uint8)
    out = []
    for i in range(N):
        a = np.where(_mask_image(i) != 0, 255, 0).astype(np.uint8) if (with_files and i != NO_MASK) else np.full((H, W), 255, np.uint8)
        a3 = np.repeat(a[None, :, :, None], 3, 3)
        if any(c != 0 for c in scene.dist):
            a3 = LR.undistort_host(a3, scene.intr, scene.dist, zoom)
        a3 = a3[0] & valid[:, :, None]
        out.append((RR.pil_resize(np.ascontiguousarray(a3), size)[..., 0] == 255).astype(np.float32))
    return torch.from_numpy(np.stack(out))[:, None]


def test_lens_valid_kernel_is_the_host_predicate(capture):
    _, _, dist = capture
    for (h, w) in LR.SHAPES:
        intr = LR.intrinsics(h, w)
        got = ops.lens_valid_u8(h, w, intr, dist, 1.0, device=DEV)
        assert got.dtype == torch.uint8 and got.shape == (h, w)
        assert np.array_equal(got.cpu().numpy(), MR.lens_valid_host(h, w, LR.lens_array(intr, dist, 1.0)))
    with pytest.raises(ValueError):
        ops.lens_valid_u8(0, 4, LR.intrinsics(4, 4), dist, device=DEV)


def test_masks_and_lens_mask_against_the_host(capture):
    root, frames, dist = capture
    scene = DS.CustomScene(root, 'desk', 'train', downscale_factor=2, masks=True, lens='mask')
    assert scene.zoom == 1.0 and scene.img_size == (12, 16)
    fx, fy = scene.intr[:2]                                                                # K at zoom 1: the lens' own focal lengths
    assert abs(float(scene.K[0, 0, 0]) - fx / (min(W, H) / 2.0)) < 1e-6 and abs(float(scene.K[0, 1, 1]) - fy / (min(W, H) / 2.0)) < 1e-6
    views = scene.views(DEV, chunk=4)                                                      # two uploads: 4 + 2 frames
    assert set(views) == {'imgs', 'K', 'R', 'T', 'masks'} and views['masks'].shape == (N, 1, 12, 16) and views['masks'].dtype == torch.float32
    want = _host_masks(scene, (12, 16), 1.0)
    assert torch.equal(views['masks'].cpu(), want)
    assert 0 < want.sum() < want.numel()                                                   # (the shadow is invalid, the rest is not)
    raw = torch.from_numpy(frames)
    want_imgs = RR.resample_host(LR.undistort_host(raw, scene.intr, scene.dist, 1.0), (12, 16))
    assert torch.equal(views['imgs'].cpu().view(torch.int32), want_imgs.view(torch.int32))
    # a frame without mask_path is valid wherever the lens is
    lens_only = DS.CustomScene(root, 'desk', 'train', downscale_factor=2, lens='mask').views(DEV)
    assert torch.equal(views['masks'][NO_MASK], lens_only['masks'][NO_MASK])
    assert torch.equal(lens_only['masks'].cpu(), _host_masks(scene, (12, 16), 1.0, with_files=False))
    assert bool((lens_only['masks'] == lens_only['masks'][:1]).all())                      # one lens map for every frame


def test_masks_with_the_cropping_zoom(capture):
    root, _, _ = capture
    scene = DS.CustomScene(root, 'desk', 'train', downscale_factor=2, masks=True)          # lens='crop': the frames' own zoom, no lens map
    views = scene.views(DEV)
    assert torch.equal(views['masks'].cpu(), _host_masks(scene, (12, 16), scene.zoom, with_lens=False))
    assert bool((views['masks'][NO_MASK] == 1).all())


def test_defaults_are_unchanged(capture):
    root, frames, _ = capture
    scene = DS.CustomScene(root, 'desk', 'train', downscale_factor=2)
    views = scene.views(DEV)
    assert set(views) == {'imgs', 'K', 'R', 'T'}
    want = RR.resample_host(LR.undistort_host(torch.from_numpy(frames), scene.intr, scene.dist, scene.zoom), (12, 16))
    assert torch.equal(views['imgs'].cpu().view(torch.int32), want.view(torch.int32))
    with pytest.raises(ValueError, match='lens'):
        DS.CustomScene(root, 'desk', 'train', lens='fisheye')
    with pytest.raises(ValueError, match='store'):                                         # one store serves one mask treatment
        DS.CustomScene(root, 'desk', 'test', downscale_factor=2, masks=True, store=scene.store)


def test_lens_mask_never_raises_the_zoom_error(tmp_path):
    dist = (12.0, 0.0, 0.0, 0.0, 0.0, 0.0)                                                 # a border that leaves the source even at a zoom of 2
    write_capture(tmp_path, 'wide', n=2, H=H, W=W, dist=dist)
    with pytest.raises(ValueError, match='zoom'):
        DS.CustomScene(tmp_path, 'wide', 'train')
    views = DS.CustomScene(tmp_path, 'wide', 'train', lens='mask').views(DEV)
    share = float(views['masks'].mean())
    assert 0.05 < share < 0.5                                                              # (0.26 of the raw frame reads inside the source)


def test_dtu_layout_mask_folder(tmp_path):
    frames = write_scene(tmp_path, 'DTU', 'scan7', n_views=4, H=H, W=W, with_points=False)
    with pytest.raises(FileNotFoundError):
        DS.DTUScene(tmp_path, 'scan7', (12, 16), 'train', masks=True)
    mask_dir = os.path.join(str(tmp_path), 'DTU', 'scan7', 'mask')
    os.makedirs(mask_dir)
    made = []
    for i in range(4):
        a = np.zeros((H, W), np.uint8)
        a[4 + i:20, 5:25 - i] = 255                                                        # the object
        made.append(a)
        Image.fromarray(np.repeat(a[:, :, None], 3, 2), 'RGB').save(os.path.join(mask_dir, f'{i:03d}.png'))      # (IDR writes RGB masks)
    scene = DS.DTUScene(tmp_path, 'scan7', (12, 16), 'train', masks=True)
    views = scene.views(DEV)
    want = torch.from_numpy(np.stack([(RR.pil_resize(np.repeat(a[:, :, None], 3, 2), (12, 16))[..., 0] == 255).astype(np.float32) for a in made]))
    assert torch.equal(views['masks'].cpu(), want[:, None]) and 0 < want.sum() < want.numel()
    plain = DS.DTUScene(tmp_path, 'scan7', (12, 16), 'train').views(DEV)
    assert 'masks' not in plain and torch.equal(plain['imgs'], views['imgs'])
    os.remove(os.path.join(mask_dir, '003.png'))
    with pytest.raises(ValueError, match='3 masks for 4 images'):
        DS.DTUScene(tmp_path, 'scan7', (12, 16), 'train', masks=True)
