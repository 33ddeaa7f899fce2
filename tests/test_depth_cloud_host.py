"""CPU: ops.depth_cloud_host (the numpy path of the depth cloud) byte for byte against the host build of csrc/depth_math.h with its integer
accumulation (tests/depth_ref.py) on every shape of the GPU list, the cloud of an analytic capture (tests/depth_fixture.py) against the
capture's surfaces and ground plane, and dataset.CustomScene(cloud=...) with the config path of dbw_amd/train.py as far as it runs
without a device."""
import numpy as np
import pytest
import torch

import depth_fixture as DF
import depth_ref as DR
import dbw_amd
from dbw_amd import dataset as DS
from dbw_amd import eval3d, ops, train
from test_worldfit_host import BOUND_NORMAL_DEG, BOUND_OFFSET_R0


@pytest.mark.parametrize('c', DR.CASES, ids=DR.case_id)
def test_the_numpy_path_gives_the_bytes_of_the_header(c):
    depth, cams, target, poses = DR.case(c['N'], c['H'], c['W'], c['kind'])
    want = DR.cloud_host(depth, cams, target, poses, DR.box(-2.0, 2.0, c['G']), c['G'], 1, 65535, c['stride'], c['permille'], c['min_count'])
    got = ops.depth_cloud_host(depth, cams, target, poses, -2.0, 2.0, grid=c['G'], stride=c['stride'], edge=c['permille'] / 1000, min_count=c['min_count'],
                               return_info=True)
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[0].shape == (len(got[1]), 3)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2].tolist()
    # a CPU tensor of the 16 bits is the same input
    again = ops.depth_cloud_host(torch.from_numpy(depth.view(np.int16)), cams, target, poses, -2.0, 2.0, grid=c['G'], stride=c['stride'],
                                 edge=c['permille'] / 1000, min_count=c['min_count'])
    assert again[0].tobytes() == want[0].tobytes() and again[1].tobytes() == want[1].tobytes()


def test_the_range_in_depth_steps_and_the_box():
    depth, cams, target, poses = DR.case(3, 24, 32, 'radtan')
    want = DR.cloud_host(depth, cams, target, poses, DR.box(-1.5, 1.5, 8), 8, 2000, 2600, 1, 0, 1)
    got = ops.depth_cloud_host(depth, cams, target, poses, -1.5, (1.5, 1.5, 1.5), grid=8, d_range=(2000, 2600), return_info=True)
    assert got[0].tobytes() == want[0].tobytes() and got[2] == want[2].tolist() and 0 < got[2][1] < int(((depth >= 2000) & (depth <= 2600)).sum()) + 1
    assert np.array_equal(ops.depth_box(-1.5, 1.5, 8), DR.box(-1.5, 1.5, 8))
    with pytest.raises(ValueError, match='corners of a cube'):
        ops.depth_box((-1, -1, -1), (1, 1, 2), 8)
    with pytest.raises(ValueError, match='grid: 1 .. 256'):
        ops.depth_box(-1, 1, 257)
    with pytest.raises(ValueError, match='d_range'):
        ops.depth_cloud_host(depth, cams, target, poses, -2, 2, d_range=(0, 10))
    with pytest.raises(ValueError, match=r'cams: \(3,16\)'):
        ops.depth_cloud_host(depth, cams[:2], target, poses, -2, 2)


def _scene_points(scene, points):
    """points of the normalised frame back in the file's frame, in metres"""
    S = scene.scale_mat.double().numpy()
    return np.asarray(points, np.float64) @ S[:3, :3].T + S[:3, 3]


@pytest.mark.parametrize('lens', ('pinhole', 'radtan'))
def test_the_cloud_of_an_analytic_capture_lies_on_its_surfaces(tmp_path, lens):
    """Every point within one cell diagonal + the largest depth difference between 4-neighbouring pixels of the fixture (both measured
    depths) + one depth unit of a surface, in metres of the file's frame; the ground plane of world_frame within the bounds
    tests/test_worldfit_host.py holds the fit of a .ply to."""
    dist = DF.MILD if lens == 'radtan' else (0.0,) * 6
    depth, metres, c2w = DF.write_depth_capture(tmp_path, 'cap', dist=dist)
    scene = DS.CustomScene(tmp_path, 'cap', 'train', cloud='depth')
    pts = scene.cloud()
    assert pts.dtype == torch.float32 and pts.shape[1] == 3 and scene.cloud() is pts                  # built once
    info = scene.cloud_info
    assert info['frames'] == 6 and info['points'] == len(pts) > 300 and 0 < info['samples'] <= int((depth > 0).sum())
    F = np.linalg.inv(scene.scale_mat.double().numpy())
    s = float(np.cbrt(np.linalg.det(F[:3, :3])))                                                       # metres -> normalised
    cell_diag = np.sqrt(3.0) * (2 * 2.0 / 128) / s
    d = depth.astype(np.float64) * DF.UNIT
    both_h, both_v = (depth[:, :, 1:] > 0) & (depth[:, :, :-1] > 0), (depth[:, 1:] > 0) & (depth[:, :-1] > 0)
    step = max(float(np.abs(d[:, :, 1:] - d[:, :, :-1])[both_h].max()), float(np.abs(d[:, 1:] - d[:, :-1])[both_v].max()))
    tol = cell_diag + step + DF.UNIT
    off = DF.surface_distance(_scene_points(scene, pts.numpy()))
    print(f'{lens}: {len(pts)} points from {info["samples"]} samples ({info["outside"]} outside the cube); off the surfaces by at most {off.max():.4f} m, '
          f'median {np.median(off):.4f} m; tolerance {tol:.4f} m = cell diagonal {cell_diag:.4f} + neighbour step {step:.4f} + unit {DF.UNIT}')
    assert off.max() <= tol
    assert np.median(off) <= cell_diag                                                                 # (and most of them far closer than that)
    # the boxes are in the cloud, not only the ground
    assert (_scene_points(scene, pts.numpy())[:, 2] > 0.3).sum() > 20

    fr = scene.world_frame()
    n = F[:3, :3] @ np.array([0.0, 0.0, 1.0]) / s
    foot = F[:3, 3]                                                                                    # the image of the origin, a point of the plane
    nf, df = fr.plane
    ang = float(np.degrees(np.arccos(np.clip(nf @ n, -1, 1))))
    offset = abs(df - float(n @ foot)) / fr.r0
    print(f'{lens}: ground plane normal off by {ang:.5f} deg (bound {BOUND_NORMAL_DEG:.5f}), offset by {offset:.5f} r0 (bound {BOUND_OFFSET_R0:.5f})')
    assert ang <= BOUND_NORMAL_DEG and offset <= BOUND_OFFSET_R0


def test_scene_options_and_refusals(tmp_path):
    depth, _, _ = DF.write_depth_capture(tmp_path, 'cap')
    with pytest.raises(ValueError, match="cloud: 'colour' is not one of source, unit, range, grid, bound, stride, edge, min_count"):
        DS.CustomScene(tmp_path, 'cap', 'train', cloud={'source': 'depth', 'colour': 1})
    with pytest.raises(ValueError, match="cloud: 'file', 'depth' or a mapping"):
        DS.CustomScene(tmp_path, 'cap', 'train', cloud='points')
    with pytest.raises(ValueError, match="cloud.source: 'file' or 'depth'"):
        DS.CustomScene(tmp_path, 'cap', 'train', cloud={'source': 'sfm'})
    # the defaults, and the unit of the file
    scene = DS.CustomScene(tmp_path, 'cap', 'train', cloud='depth')
    D = scene._depth
    assert scene.cloud_options == {'unit': None, 'range': (0.1, 10.0), 'grid': 128, 'bound': 2.0, 'stride': 1, 'edge': 0.05, 'min_count': 2}
    assert D['unit'] == DF.UNIT and D['d_range'] == (100, 10000) and D['size'] == (48, 64) and (D['lo'], D['hi']) == (-2.0, 2.0)
    # a depth size that differs from the images': the intrinsics scale with it
    assert scene.raw_img_size == (24, 32)
    fx, fy, cx, cy = scene.intr
    assert np.array_equal(D['cams'].numpy()[:, 1:5], np.tile(np.float32([2 * fx, 2 * fy, 2 * cx, 2 * cy]), (6, 1)))
    assert np.array_equal(D['target'].numpy(), ops.lens_target((2 * fx, 2 * fy, 2 * cx, 2 * cy)).numpy())
    # the pose rows: the camera's axes (x, -y, -z) of the normalised cam2world, in depth steps
    F = np.linalg.inv(scene.scale_mat.double().numpy())
    s = float(np.cbrt(np.linalg.det(F[:3, :3])))
    c2w = scene.cam2world.double().numpy()
    want = np.concatenate([(c2w[:, :3, :3] * np.array([1.0, -1.0, -1.0]) * (DF.UNIT * s)).reshape(6, 9), c2w[:, :3, 3]], 1)
    assert np.abs(D['poses'] - want).max() <= 2.0 ** -22 * np.abs(want).max()                        # (cam2world is kept in fp32)
    # the mapping form
    m = DS.CustomScene(tmp_path, 'cap', 'train', cloud={'source': 'depth', 'unit': 2e-3, 'range': [0.5, 8], 'grid': 32, 'bound': 1.5, 'stride': 2,
                                                         'edge': 0.1, 'min_count': 1})
    D = m._depth
    assert (D['unit'], D['d_range'], D['grid'], D['lo'], D['hi'], D['stride'], D['edge'], D['min_count']) == (2e-3, (250, 4000), 32, -1.5, 1.5, 2, 0.1, 1)
    scene.cloud()
    assert len(m.cloud()) > 50 and m.cloud_info['samples'] < scene.cloud_info['samples']             # every second row and column
    assert DS.CustomScene(tmp_path, 'cap', 'train', cloud={'source': 'file'}).cloud_options is None
    # pc_gt stays what it is: no .ply here
    assert scene.ply_file is None and tuple(scene.pc_gt.shape) == (1, 3)


def test_missing_depth_maps_and_sizes(tmp_path):
    DF.write_depth_capture(tmp_path, 'some', skip=(1, 4), unit_in_file=False)
    scene = DS.CustomScene(tmp_path, 'some', 'train', cloud='depth')
    assert scene._depth['frames'] == [0, 2, 3, 5] and scene._depth['unit'] == 1e-3 and len(scene._depth['files']) == 4
    assert tuple(scene._depth['cams'].shape) == (4, 16) and scene._depth['poses'].shape == (4, 12)
    scene.cloud()
    assert scene.cloud_info['frames'] == 4
    DF.write_depth_capture(tmp_path, 'none', skip=range(6))
    with pytest.raises(ValueError, match="cloud='depth', but no frame has a depth_file_path"):
        DS.CustomScene(tmp_path, 'none', 'train', cloud='depth')
    assert DS.CustomScene(tmp_path, 'none', 'train').cloud_options is None                                # 'file' does not look at depth at all
    # one map of another size
    from PIL import Image
    DF.write_depth_capture(tmp_path, 'odd')
    Image.fromarray(np.zeros((40, 64), np.uint16)).save(tmp_path / 'custom' / 'odd' / 'depth' / 'frame_00003.png')
    with pytest.raises(ValueError, match='the depth maps must share one size'):
        DS.CustomScene(tmp_path, 'odd', 'train', cloud='depth')
    # an 8-bit RGB file is no depth map
    DF.write_depth_capture(tmp_path, 'rgb')
    Image.fromarray(np.zeros((48, 64, 3), np.uint8)).save(tmp_path / 'custom' / 'rgb' / 'depth' / 'frame_00002.png')
    with pytest.raises(ValueError, match='single-channel 16-bit PNG'):
        DS.CustomScene(tmp_path, 'rgb', 'train', cloud='depth').cloud()


def test_per_frame_cameras_and_undistort_false_use_the_true_lens(tmp_path):
    DF.write_depth_capture(tmp_path, 'lens', dist=DF.MILD)
    a = DS.CustomScene(tmp_path, 'lens', 'train', cloud='depth')
    b = DS.CustomScene(tmp_path, 'lens', 'train', cloud='depth', undistort=False)
    c = DS.CustomScene(tmp_path, 'lens', 'train', cloud='depth', cameras='per_frame')
    for other in (b, c):
        assert torch.equal(a._depth['cams'], other._depth['cams']) and torch.equal(a._depth['target'], other._depth['target'])
        assert np.array_equal(a._depth['poses'], other._depth['poses'])
    assert np.array_equal(a._depth['cams'].numpy()[0, 5:11], np.float32(DF.MILD)) and a.zoom > 1.0         # the target is at zoom 1 all the same
    assert torch.equal(a.cloud(), c.cloud())


def test_cloud_file_keeps_todays_behaviour(tmp_path):
    import custom_fixture as CF
    CF.write_capture(tmp_path, 'bare')
    scene = DS.CustomScene(tmp_path, 'bare', 'train')
    with pytest.raises(ValueError, match="'bare': no point cloud \\(ply_file_path of transforms.json, or points.ply next to it\\): the world frame is "
                                         'fitted to the cloud, there is no fit without one'):
        scene.world_frame()
    with pytest.raises(ValueError, match="'bare': no point cloud \\(ply_file_path of transforms.json, or points.ply next to it\\): the blocks are "
                                         'fitted to the cloud, there is no fit without one'):
        scene.block_init(None)
    with pytest.raises(ValueError, match='no point cloud'):
        scene.cloud()
    CF.write_capture(tmp_path, 'ply', with_points=True)
    scene = DS.CustomScene(tmp_path, 'ply', 'train', cloud='file')
    assert scene.cloud() is scene.pc_gt and tuple(scene.cloud().shape) == (30, 3) and scene.cloud_info is None
    # a capture with both: 'file' reads the .ply, 'depth' the maps, and pc_gt is the .ply either way
    DF.write_depth_capture(tmp_path, 'both', with_points=True)
    f, d = DS.CustomScene(tmp_path, 'both', 'train'), DS.CustomScene(tmp_path, 'both', 'train', cloud='depth')
    assert torch.equal(f.pc_gt, d.pc_gt) and len(f.cloud()) == 30 and len(d.cloud()) > 300


def _cfg(n_blocks, frame, **training):
    return {'model': {'name': 'dbw', 'mesh': dict(n_blocks=n_blocks, txt_size=8, **frame),
                      'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                      'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True, 'opacity_noise': False},
                      'loss': {'rgb_weight': 1, 'perceptual_weight': 0, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}},
            'training': dict(training)}


def test_the_shipped_config():
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(DS.__file__)), '..', 'configs', 'custom_depth_cloud.yml')
    cfg = DS.load_config(path)
    assert cfg['dataset']['name'] == 'custom' and DS.cloud_options(cfg['dataset']['cloud']) == dict(DS.CLOUD_DEFAULTS)
    assert train.wants_world_frame(cfg) and train.blocks_init_options(cfg) == {}
    # the mapping its comment shows is the same request
    assert DS.cloud_options({'source': 'depth', 'unit': 0.001, 'range': [0.1, 10.0], 'grid': 128, 'bound': 2.0, 'stride': 1, 'edge': 0.05,
                             'min_count': 2}) == dict(DS.CLOUD_DEFAULTS, unit=0.001)


def test_the_config_path_on_the_cpu(tmp_path, capsys):
    DF.write_depth_capture(tmp_path, 'cap')
    cfg = {'dataset': {'name': 'custom', 'tag': 'cap', 'cloud': 'depth'}, 'training': {'batch_size': 2}}
    scene, _, _ = DS.create_train_val_test(cfg, tmp_path)
    run_dir = tmp_path / 'run'
    run_dir.mkdir()
    pts = train.resolve_depth_cloud(scene, 'cpu', str(run_dir))
    out = capsys.readouterr().out
    info = scene.cloud_info
    assert f"depth_cloud: {len(pts)} points from {info['samples']} samples of 6 frames" in out
    back = np.asarray(eval3d.read_ply_points(run_dir / 'depth_cloud.ply'), np.float32)
    assert back.tobytes() == pts.numpy().tobytes()
    assert train.resolve_depth_cloud(DS.CustomScene(tmp_path, 'cap', 'train'), 'cpu', str(run_dir)) is None            # cloud: file
    # R_world: auto and blocks_init: points find the cloud
    mesh = {'R_world': 'auto', 'T_world': 'auto', 'S_world': 'auto'}
    full = _cfg(4, mesh, blocks_init={'min_points': 20})
    frame = train.resolve_world_frame(full, scene, 'cpu', str(run_dir))
    assert frame is not None and (run_dir / 'world_frame.yml').exists()
    torch.manual_seed(5)
    model = dbw_amd.create_model(full, scene.img_size)
    init = train.resolve_blocks_init(full, scene, model, 'cpu', str(run_dir))
    out = capsys.readouterr().out
    assert 'R_world: auto -> WorldFrame(' in out and 'blocks_init: points -> ' in out
    assert 1 <= len(init) <= 4 and torch.equal(model.T.detach()[:len(init)], init.T) and (run_dir / 'blocks_init.yml').exists()
    assert init.n_points_used <= len(pts)
