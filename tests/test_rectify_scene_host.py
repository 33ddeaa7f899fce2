"""CPU tests of dataset.CustomScene(cameras='per_frame') on synthetic captures written into tmp_path (tests/custom_fixture.py): the two
kinds of capture the 'shared' mode refuses, what stays refused, equal cameras against the 'shared' scene, and the per-frame treatment of
the store.  ops.rectify_u8, ops.rectify_valid_u8 and ops.resample_u8 have no CPU path: stand-ins built on the host builds of the same
headers (tests/rectify_ref.py, tests/resample_ref.py) take their place where frames are made; tests/test_gpu_rectify.py runs the real
ones."""
import numpy as np
import pytest
import torch

import lens_ref as LR
import rectify_ref as RF
import resample_ref as RR
from custom_fixture import write_capture
from dbw_amd import dataset as DS
from dbw_amd import ops


def test_the_captures_the_shared_mode_refuses_load_per_frame(tmp_path):
    write_capture(tmp_path, 'fish', n=2, camera_model='OPENCV_FISHEYE')
    with pytest.raises(NotImplementedError, match="OPENCV_FISHEYE.*cameras='per_frame'"):
        DS.CustomScene(tmp_path, 'fish', 'train')
    fish = DS.CustomScene(tmp_path, 'fish', 'train', cameras='per_frame')
    assert fish.models.tolist() == [1, 1] and fish.intr == LR.intrinsics(24, 32) and fish.dist == LR.COEFFS[0] and fish.prepare is not None
    assert fish.intrs.shape == (2, 4) and fish.dists.shape == (2, 6) and fish.store.per_frame
    assert fish.zoom == DS.rectify_zoom(24, 32, fish.intrs, fish.dists, fish.models, fish.intr)
    write_capture(tmp_path, 'perframe', n=3, per_frame={1: {'fl_x': 31.0}})
    with pytest.raises(NotImplementedError, match="per-frame intrinsics differ \\('fl_x'\\).*cameras='per_frame'"):
        DS.CustomScene(tmp_path, 'perframe', 'train')
    pf = DS.CustomScene(tmp_path, 'perframe', 'train', cameras='per_frame')
    fx, fy, cx, cy = LR.intrinsics(24, 32)
    assert pf.intrs[:, 0].tolist() == [fx, 31.0, fx] and (pf.intrs[:, 1:] == [fy, cx, cy]).all() and pf.models.tolist() == [0, 0, 0]
    assert pf.intr == (fx, fy, cx, cy) and pf.dist == LR.COEFFS[0]                     # the median; the coefficients are shared
    assert pf.zoom == DS.rectify_zoom(24, 32, pf.intrs, pf.dists, pf.models, pf.intr) > 1
    assert tuple(pf.K.shape) == (3, 4, 4) and torch.equal(pf.K[0], pf.K[1])
    # a coefficient on one frame only: the others have the top level's, and dist is no longer one tuple
    write_capture(tmp_path, 'k', n=3, per_frame={2: {'k1': 0.1, 'k3': 0.01}})
    k = DS.CustomScene(tmp_path, 'k', 'train', cameras='per_frame')
    assert k.dists[:, 0].tolist() == [0.12, 0.12, 0.1] and k.dists[:, 2].tolist() == [0.0, 0.0, 0.01] and k.dist is None
    with pytest.raises(ValueError, match="cameras: 'shared' or 'per_frame'"):
        DS.CustomScene(tmp_path, 'k', 'train', cameras='each')


def test_what_stays_refused(tmp_path):
    write_capture(tmp_path, 'equi', n=2, camera_model='EQUIRECTANGULAR')
    with pytest.raises(NotImplementedError, match='EQUIRECTANGULAR'):
        DS.CustomScene(tmp_path, 'equi', 'train', cameras='per_frame')
    write_capture(tmp_path, 'size', n=3, frame_size={2: (24, 30)})
    with pytest.raises(ValueError, match=r"frame_00003.png: \(24, 30\), transforms.json says \(24, 32\)"):
        DS.CustomScene(tmp_path, 'size', 'train', cameras='per_frame')
    write_capture(tmp_path, 'w', n=3, per_frame={1: {'w': 30}})
    with pytest.raises(NotImplementedError, match="per-frame intrinsics differ \\('w'\\)"):
        DS.CustomScene(tmp_path, 'w', 'train', cameras='per_frame')
    write_capture(tmp_path, 'perframe', n=3, per_frame={1: {'fl_x': 31.0}})
    with pytest.raises(ValueError, match='undistort=False.*no single K'):
        DS.CustomScene(tmp_path, 'perframe', 'train', cameras='per_frame', undistort=False)
    # a source far narrower than the others: no crop below a zoom of 2, and the message names lens='mask', which loads
    write_capture(tmp_path, 'narrow', n=3, per_frame={1: {'fl_x': 90.0, 'fl_y': 90.0}})
    with pytest.raises(ValueError, match="lens='mask'"):
        DS.CustomScene(tmp_path, 'narrow', 'train', cameras='per_frame')
    assert DS.CustomScene(tmp_path, 'narrow', 'train', cameras='per_frame', lens='mask').zoom == 1.0


@pytest.mark.parametrize('dist', [LR.COEFFS[0], LR.COEFFS[1], (0.0,) * 6])
def test_equal_cameras_are_the_shared_scene(tmp_path, dist):
    fx = LR.intrinsics(24, 32)[0]
    write_capture(tmp_path, 'same', n=4, dist=dist, per_frame={i: {'fl_x': fx, 'k1': dist[0]} for i in range(4)})
    for kw in (dict(), dict(lens='mask'), dict(undistort=False)):
        a, b = DS.CustomScene(tmp_path, 'same', 'train', **kw), DS.CustomScene(tmp_path, 'same', 'train', cameras='per_frame', **kw)
        assert b.intr == a.intr and b.zoom == a.zoom and b.dist == a.dist and torch.equal(b.K, a.K), kw
        assert (b.prepare is None) == (a.prepare is None) and b.store.has_masks == a.store.has_masks, kw
        assert torch.equal(b.R, a.R) and torch.equal(b.T, a.T) and b.view_ids == a.view_ids
    # a store built for one mode is refused by the other
    a, b = DS.CustomScene(tmp_path, 'same', 'train'), DS.CustomScene(tmp_path, 'same', 'train', cameras='per_frame')
    with pytest.raises(ValueError, match='store'):
        DS.CustomScene(tmp_path, 'same', 'test', store=a.store, cameras='per_frame')
    with pytest.raises(ValueError, match='store'):
        DS.CustomScene(tmp_path, 'same', 'test', store=b.store)
    assert DS.CustomScene(tmp_path, 'same', 'test', store=b.store, cameras='per_frame').store is b.store


@pytest.mark.parametrize('lens', ['crop', 'mask'])
def test_the_store_rectifies_every_frame_by_its_own_camera(tmp_path, monkeypatch, lens):
    """The chunks reach ops.rectify_u8 with the rows of THEIR frames (chunks of 4 + 2 of 6 frames), the masks go through the same warp and
    are ANDed with their frame's validity map."""
    frames, intrs, dists, models = RF.write_fisheye_capture(tmp_path, 'rig')
    calls = []

    def rectify(raw, rows, target):
        calls.append(rows.clone())
        return RF.rectify_host(raw, rows, target)
    monkeypatch.setattr(ops, 'rectify_u8', rectify)
    monkeypatch.setattr(ops, 'rectify_valid_u8', lambda H, W, rows, target, device='cuda': torch.from_numpy(RF.valid_host(H, W, rows, target)))
    monkeypatch.setattr(ops, 'resample_u8', lambda src, size, out='f32', form='auto': RR.resample_host(src, size, out=out))
    scene = DS.CustomScene(tmp_path, 'rig', 'train', downscale_factor=2, cameras='per_frame', lens=lens)
    assert np.array_equal(scene.intrs, intrs) and np.array_equal(scene.dists, dists) and np.array_equal(scene.models, models)
    tgt = tuple(float(v) for v in np.median(intrs, axis=0))
    zoom = DS.rectify_zoom(24, 32, intrs, dists, models, tgt) if lens == 'crop' else 1.0
    assert scene.intr == tgt and scene.zoom == zoom and (zoom > 1.1) == (lens == 'crop')
    rows, t32 = RF.table(intrs, dists, models), RF.target(tgt, zoom)
    views = scene.views('cpu', chunk=4)
    ids = scene.ids()
    of_frames = calls[::2] if lens == 'mask' else calls                                 # (under 'mask' every chunk's masks take the same warp)
    assert ids == list(range(6)) and [c.shape[0] for c in of_frames] == [4, 2] and len(calls) == (4 if lens == 'mask' else 2)
    assert np.array_equal(torch.cat(of_frames).numpy(), rows)
    want = RR.resample_host(torch.from_numpy(RF.rectify_host(frames, rows, t32)), (12, 16))
    assert torch.equal(views['imgs'].view(torch.int32), want.view(torch.int32))
    # K is the target's, zoomed
    assert abs(float(scene.K[0, 0, 0]) - zoom * tgt[0] / 12.0) < 1e-5 and abs(float(scene.K[0, 1, 1]) - zoom * tgt[1] / 12.0) < 1e-5
    if lens == 'crop':
        assert 'masks' not in views
        return
    valid = RF.valid_host(24, 32, rows, t32)
    assert valid[2].mean() < 255 * 0.9 and (valid[1] == 255).all()                      # camera C cannot fill its frame, B can
    warped = RF.rectify_host(np.full((6, 24, 32, 3), 255, np.uint8), rows, t32) & valid[..., None]
    small = RR.resample_host(torch.from_numpy(warped), (12, 16), out='u8')
    want_masks = (small[..., 0] == 255).to(torch.float32)[:, None]
    assert torch.equal(views['masks'], want_masks) and 0 < float(want_masks[2].mean()) < 1 and float(want_masks[1].mean()) == 1


def test_the_shipped_example_config_builds_the_scenes(tmp_path):
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(DS.__file__)), '..', 'configs', 'custom_per_frame.yml')
    cfg = DS.load_config(path)
    assert cfg['dataset'] == {'name': 'custom', 'tag': 'my_capture', 'downscale_factor': 2, 'cameras': 'per_frame', 'lens': 'mask'}
    RF.write_fisheye_capture(tmp_path, 'my_capture')
    train, val, test = DS.create_train_val_test(cfg, tmp_path)
    assert train.cameras == 'per_frame' and train.zoom == 1.0 and train.store.has_masks and train.store.per_frame
    assert train.store is val.store is test.store and (train.models == 1).all()
