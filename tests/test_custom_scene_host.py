"""CPU tests of the custom-scene loader (dataset.CustomScene) on a synthetic capture written into tmp_path (tests/custom_fixture.py): the
dataset kind and its shared store, K / R / T against the projection-matrix route the DTU loader takes, the pose normalisation, the
splits, the refusals, and the lens treatment chosen for the store.  ops.resample_u8 and ops.undistort_u8 have no CPU path: stand-ins built
on the host builds of the same headers (tests/resample_ref.py, tests/lens_ref.py) take their place where frames are made;
tests/test_gpu_lens.py runs the real ones."""
import json
import os

import numpy as np
import pytest
import torch

import lens_ref as LR
import resample_ref as RR
from custom_fixture import write_capture
from dbw_amd import dataset as DS
from dbw_amd import ops
from dbw_amd.cameras import pytorch3d_KRT_from_proj


def test_custom_is_a_dataset_kind_and_the_splits_share_one_store(tmp_path):
    write_capture(tmp_path, 'desk', n=11)
    assert DS.get_scene_class('custom') is DS.CustomScene and DS.CustomScene.name == 'custom'
    cfg = {'dataset': {'name': 'custom', 'tag': 'desk', 'downscale_factor': 2}, 'training': {'batch_size': 2}}
    train, val, test = DS.create_train_val_test(cfg, tmp_path)
    assert all(isinstance(s, DS.CustomScene) for s in (train, val, test)) and train.store is val.store is test.store
    assert (len(train), len(val), len(test)) == (10, 0, 1) and train.raw_img_size == (24, 32) and train.img_size == (12, 16)
    assert train.store.prepare is not None and train.zoom == DS.lens_zoom(24, 32, LR.intrinsics(24, 32), LR.COEFFS[0]) > 1
    with pytest.raises(NotImplementedError, match='nerfstudio'):                 # the reference's own kind stays refused
        DS.get_scene_class('nerfstudio')


def test_img_size_and_extensionless_paths(tmp_path):
    write_capture(tmp_path, 'a', n=3, H=23, W=37, with_extension=False)
    s = DS.CustomScene(tmp_path, 'a', 'train', downscale_factor=2)
    assert s.img_size == (round(23 / 2), round(37 / 2)) == (12, 18) and s.raw_img_size == (23, 37)            # nerfstudio.py:55
    assert [os.path.basename(str(f)) for f in s.input_files] == [f'frame_{i:05d}.png' for i in (1, 2, 3)] and all(f.is_absolute() for f in s.input_files)
    assert DS.CustomScene(tmp_path, 'a', 'train').img_size == (23, 37)
    assert DS.CustomScene(tmp_path, 'a', 'train', img_size=[8, 12]).img_size == (8, 12) and DS.CustomScene(tmp_path, 'a', 'train', img_size=8).img_size == (8, 8)


def test_KRT_equal_the_projection_matrix_route(tmp_path):
    """P = K_cv [R_cv | t_cv] of the same camera -- the OpenCV world-to-camera is the OpenGL camera-to-world with the camera's y and z axes
    negated, inverted -- through cameras.pytorch3d_KRT_from_proj, the route of the DTU loader."""
    H, W = 24, 32
    _, c2w = write_capture(tmp_path, 'k', n=6, H=H, W=W, dist=(0.0,) * 6)
    s = DS.CustomScene(tmp_path, 'k', 'train', normalize='none')
    assert s.zoom == 1.0 and torch.equal(s.scale_mat, torch.eye(4))
    fx, fy, cx, cy = LR.intrinsics(H, W)
    Kcv = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    for i in range(6):
        cv = c2w[i].copy()
        cv[:3, 1:3] *= -1
        w2c = np.linalg.inv(cv)
        K, R, T = pytorch3d_KRT_from_proj(Kcv @ w2c[:3, :4], (H, W))
        for got, want in ((s.K[i], K), (s.R[i], R), (s.T[i], T)):
            assert float((got - want).abs().max()) <= 1e-5, i
    assert s.K.shape == (6, 4, 4) and s.R.shape == (6, 3, 3) and s.T.shape == (6, 3) and s.K.dtype == s.R.dtype == s.T.dtype == torch.float32


def test_the_zoom_scales_the_training_focal_lengths(tmp_path):
    write_capture(tmp_path, 'z', n=3)
    a, b = DS.CustomScene(tmp_path, 'z', 'train'), DS.CustomScene(tmp_path, 'z', 'train', undistort=False)
    assert a.zoom > 1.05 and b.zoom == 1.0
    assert torch.allclose(a.K[0, 0, 0], b.K[0, 0, 0] * a.zoom, rtol=1e-6) and torch.allclose(a.K[0, 1, 1], b.K[0, 1, 1] * a.zoom, rtol=1e-6)
    assert torch.equal(a.K[0, :2, 2], b.K[0, :2, 2]) and torch.equal(a.R, b.R) and torch.equal(a.T, b.T)


def _centres(scene):
    return scene.cam2world[:, :3, 3].double().numpy()


def test_pose_normalisation(tmp_path):
    _, c2w = write_capture(tmp_path, 'n', n=7, with_points=True)
    s = DS.CustomScene(tmp_path, 'n', 'train')
    c = _centres(s)
    assert np.abs(c.mean(0)).max() <= 1e-6 and abs(np.abs(c).max() - 1) <= 1e-6
    up = s.cam2world[:, :3, 1].double().numpy().mean(0)
    assert np.abs(up / np.linalg.norm(up) - [0, 0, 1]).max() <= 1e-6
    rot = s.cam2world[:, :3, :3].double().numpy()
    assert np.abs(rot @ rot.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-6            # the scale went to the translations only
    back = c @ s.scale_mat[:3, :3].double().numpy().T + s.scale_mat[:3, 3].double().numpy()
    assert np.abs(back - c2w[:, :3, 3]).max() <= 1e-5 * np.abs(c2w[:, :3, 3]).max()
    # R, T are those of the normalised cameras: a camera's centre is -T R^T ... in the flipped axes, X_cam = X_world @ R + T is 0 there
    assert float((s.cam2world[:, :3, 3].unsqueeze(1) @ s.R + s.T.unsqueeze(1)).abs().max()) <= 1e-5
    # the points follow the cameras
    from dbw_amd.eval3d import read_ply_points
    pts = np.asarray(read_ply_points(tmp_path / 'custom' / 'n' / 'points.ply'), dtype=np.float64)
    assert s.pc_gt.shape == (30, 3)
    back = s.pc_gt.double().numpy() @ s.scale_mat[:3, :3].double().numpy().T + s.scale_mat[:3, 3].double().numpy()
    assert np.abs(back - pts).max() <= 1e-5 * np.abs(pts).max()
    assert torch.equal(DS.CustomScene(tmp_path, 'n', 'train', normalize='none').pc_gt, torch.from_numpy(pts).float())
    with pytest.raises(ValueError, match='normalize'):
        DS.CustomScene(tmp_path, 'n', 'train', normalize='auto')


def test_opposite_and_coinciding_up_vectors():
    for up in ([0, 0, 1.0], [0, 0, -1.0], [0.6, 0, -0.8], [0, 1.0, 0]):
        R = DS._rotation_to_z(np.array(up))
        assert np.abs(R @ np.array(up) - [0, 0, 1]).max() <= 1e-12 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1) <= 1e-12


def test_a_dataparser_file_is_honoured_instead(tmp_path):
    transform = np.array([[0, 1, 0, 0.5], [-1, 0, 0, -2.0], [0, 0, 1, 0.25]], dtype=np.float64)
    _, c2w = write_capture(tmp_path, 'd', n=4, dataparser=(transform, 0.125), with_points=True)
    s = DS.CustomScene(tmp_path, 'd', 'train')
    want = (transform[:, :3] @ c2w[:, :3, 3].T).T + transform[:, 3]
    assert np.abs(_centres(s) - want * 0.125).max() <= 1e-6
    assert np.abs(s.cam2world[:, :3, :3].double().numpy() - transform[:, :3] @ c2w[:, :3, :3]).max() <= 1e-6
    back = _centres(s) @ s.scale_mat[:3, :3].double().numpy().T + s.scale_mat[:3, 3].double().numpy()
    assert np.abs(back - c2w[:, :3, 3]).max() <= 1e-5 * np.abs(c2w[:, :3, 3]).max()


@pytest.mark.parametrize('N,train,test', [(6, [0, 1, 2, 3, 4, 5], []), (10, [0, 1, 2, 3, 4, 5, 6, 7, 9], [8]),
                                          (11, [0, 1, 2, 3, 4, 5, 6, 7, 8, 10], [9]), (23, None, None)])
def test_splits(tmp_path, N, train, test):
    write_capture(tmp_path, 'desk', n=N, H=4, W=6, dist=(0.0,) * 6)
    mk = lambda split, **kw: DS.CustomScene(tmp_path, 'desk', split, **kw)
    tr, va, te = mk('train'), mk('val'), mk('test')
    n_train = int(np.ceil(0.9 * N))
    assert len(tr) == n_train and tr.view_ids == np.linspace(0, N - 1, n_train).astype(int).tolist() and len(va) == 0 and va.view_ids == []
    assert not set(tr.view_ids) & set(te.view_ids) and sorted(tr.view_ids + te.view_ids) == list(range(N)) and len(te) == N - n_train
    if train is not None:
        assert tr.view_ids == train and te.view_ids == test
    else:                                                               # 21 + 2: the test ids are shuffled under the seed len(tag)
        rest = [i for i in range(N) if i not in tr.view_ids]
        np.random.RandomState(len('desk')).shuffle(rest)
        assert te.view_ids == rest and len(rest) == 2
    ids = [4, 0, 2]
    assert mk('train', view_ids=ids).view_ids == ids and mk('test', view_ids=ids).view_ids == te.view_ids and mk('val', view_ids=ids).view_ids == []


def test_refusals(tmp_path):
    write_capture(tmp_path, 'fish', n=2, camera_model='OPENCV_FISHEYE')
    with pytest.raises(NotImplementedError, match='OPENCV_FISHEYE'):
        DS.CustomScene(tmp_path, 'fish', 'train')
    write_capture(tmp_path, 'equi', n=2, camera_model='EQUIRECTANGULAR')
    with pytest.raises(NotImplementedError, match='EQUIRECTANGULAR'):
        DS.CustomScene(tmp_path, 'equi', 'train')
    write_capture(tmp_path, 'perframe', n=3, per_frame={1: {'fl_x': 31.0}})
    with pytest.raises(NotImplementedError, match="per-frame intrinsics differ \\('fl_x'\\)"):
        DS.CustomScene(tmp_path, 'perframe', 'train')
    write_capture(tmp_path, 'size', n=3, frame_size={2: (24, 30)})
    with pytest.raises(ValueError, match=r"frame_00003.png: \(24, 30\), transforms.json says \(24, 32\)"):
        DS.CustomScene(tmp_path, 'size', 'train')
    write_capture(tmp_path, 'gone', n=3)
    os.remove(tmp_path / 'custom' / 'gone' / 'images' / 'frame_00002.png')
    with pytest.raises(FileNotFoundError, match='frame_00002.png does not exist'):
        DS.CustomScene(tmp_path, 'gone', 'train')
    write_capture(tmp_path, 'gone2', n=3, with_extension=False)
    os.remove(tmp_path / 'custom' / 'gone2' / 'images' / 'frame_00001.png')
    with pytest.raises(FileNotFoundError, match='frame_00001: no file with one of the extensions'):
        DS.CustomScene(tmp_path, 'gone2', 'train')
    with pytest.raises(FileNotFoundError, match='transforms.json does not exist'):
        DS.CustomScene(tmp_path, 'nowhere', 'train')
    # equal per-frame intrinsics, a missing camera_model and PINHOLE are fine
    fx = LR.intrinsics(24, 32)[0]
    write_capture(tmp_path, 'same', n=3, camera_model=None, per_frame={i: {'fl_x': fx, 'w': 32} for i in range(3)})
    assert DS.CustomScene(tmp_path, 'same', 'train').intr == LR.intrinsics(24, 32)
    write_capture(tmp_path, 'pin', n=3, camera_model='PINHOLE')
    assert DS.CustomScene(tmp_path, 'pin', 'train').prepare is None


def test_the_lens_treatment_of_the_store(tmp_path, monkeypatch):
    frames, _ = write_capture(tmp_path, 'l', n=5, dist=LR.COEFFS[2])
    write_capture(tmp_path, 'flat', n=2, dist=(0.0,) * 6)
    flat, off = DS.CustomScene(tmp_path, 'flat', 'train'), DS.CustomScene(tmp_path, 'l', 'train', undistort=False)
    assert flat.prepare is None and flat.store.prepare is None and flat.zoom == 1.0
    assert off.prepare is None and off.store.prepare is None and off.zoom == 1.0 and off.dist == LR.COEFFS[2]      # (k3, k4 read where given)
    on = DS.CustomScene(tmp_path, 'l', 'train')
    assert on.store.prepare is on.prepare is not None and on.dist == LR.COEFFS[2] and on.intr == LR.intrinsics(24, 32)
    with pytest.raises(ValueError, match='store'):
        DS.CustomScene(tmp_path, 'l', 'test', store=off.store)
    # the store rectifies, then resizes, and keeps what came off disk: the two ops replaced by the host builds of their headers
    calls = []

    def undistort(raw, intr, dist, zoom=1.0):
        calls.append((tuple(raw.shape), intr, dist, zoom))
        return LR.undistort_host(raw, intr, dist, zoom)
    monkeypatch.setattr(ops, 'undistort_u8', undistort)
    monkeypatch.setattr(ops, 'resample_u8', lambda src, size, out='f32', form='auto': RR.resample_host(src, size, out=out))
    on = DS.CustomScene(tmp_path, 'l', 'train', downscale_factor=2)
    views = on.views('cpu', keep_raw=True, chunk=3)
    assert calls == [((3, 24, 32, 3), on.intr, on.dist, on.zoom), ((2, 24, 32, 3), on.intr, on.dist, on.zoom)]
    want = RR.resample_host(LR.undistort_host(torch.from_numpy(frames), on.intr, on.dist, on.zoom), (12, 16))
    assert torch.equal(views['imgs'], want) and torch.equal(views['raw'], torch.from_numpy(frames))
    off = DS.CustomScene(tmp_path, 'l', 'train', downscale_factor=2, undistort=False)
    assert torch.equal(off.views('cpu')['imgs'], RR.resample_host(torch.from_numpy(frames), (12, 16))) and len(calls) == 2
    assert not torch.equal(off.views('cpu')['imgs'], want)
