"""GPU tests of the depth cloud (csrc/depth_cloud.hip, dbw_lens_depth_cloud of include/dbw_lens.h).  `-m gpu`.

The kernels and the host build (tests/host_depth_math.cpp through tests/depth_ref.py) compile one header with one rounding per operation,
and a cell adds up integers only: points, counts and info are compared for EQUALITY of bytes, at every shape of depth_ref.CASES -- N across
the 16 frames of a launch, frames of 1x1 up to 37x67, the three camera kinds, G of 1, 2, 8 and 64, both strides, the edge rule off and on,
both min_counts -- and at the corners: no sample at all, every sample in one cell, samples on the faces of the box, a depth tensor at an odd
element offset, a stream of its own, the same call twice, a workspace full of 0xFF.  Then one capture end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import depth_fixture as DF                                      # noqa: E402
import depth_ref as DR                                          # noqa: E402
import rectify_ref as RF                                        # noqa: E402
from dbw_amd import _lib, ops                                  # noqa: E402
from dbw_amd import dataset as DS                               # noqa: E402

DEV = 'cuda'


def _bits(depth):
    return torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(DEV)


def _device(depth, cams, target, poses, lo, hi, G, **kw):
    pts, counts, info = ops.depth_cloud(depth if torch.is_tensor(depth) else _bits(depth), cams, target, poses, lo, hi, grid=G, return_info=True, **kw)
    torch.cuda.synchronize()
    return pts.cpu().numpy(), counts.cpu().numpy(), info


def _same(got, want, tag=''):
    assert got[0].shape == want[0].shape and got[0].dtype == np.float32 and got[1].dtype == np.int32, tag
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and list(got[2]) == want[2].tolist(), (tag, got[2], want[2])


@pytest.mark.parametrize('c', DR.CASES, ids=DR.case_id)
def test_the_kernel_gives_the_bytes_of_the_host_build(c):
    depth, cams, target, poses = DR.case(c['N'], c['H'], c['W'], c['kind'])
    want = DR.cloud_host(depth, cams, target, poses, DR.box(-2.0, 2.0, c['G']), c['G'], 1, 65535, c['stride'], c['permille'], c['min_count'])
    got = _device(depth, cams, target, poses, -2.0, 2.0, c['G'], stride=c['stride'], edge=c['permille'] / 1000, min_count=c['min_count'])
    _same(got, want, DR.case_id(c))


def _identity(N, H, W):
    """N frames through the pinhole whose lens map is the identity (focal length 4, the principal point on the pixel grid): every pixel reads
    itself.  Poses of 2^-10 world units a depth step, inside the cube [-64, 64]^3."""
    cams = RF.table([(4.0, 4.0, W / 2, H / 2)] * N, [(0.0,) * 6] * N, [RF.RADTAN] * N)
    poses = np.tile(np.float32([2.0 ** -10, 0, 0, 0, 2.0 ** -10, 0, 0, 0, 2.0 ** -10, 0, 0, 0]), (N, 1))
    return cams, RF.target((4.0, 4.0, W / 2, H / 2)), poses


def test_no_sample_at_all():
    N, H, W = 3, 24, 32
    cams, target, poses = _identity(N, H, W)
    got = _device(np.zeros((N, H, W), np.uint16), cams, target, poses, -64.0, 64.0, 8)
    assert got[0].shape == (0, 3) and got[1].shape == (0,) and got[2] == [0, 0, 0]
    # measurements, but none in range / none in the box
    d = np.full((N, H, W), 500, np.uint16)
    assert _device(d, cams, target, poses, -64.0, 64.0, 8, d_range=(501, 600))[2] == [0, 0, 0]
    assert _device(d, cams, target, poses, 10.0, 20.0, 8)[2] == [0, 0, N * H * W]
    # cells below min_count give no row
    assert _device(d, cams, target, poses, -64.0, 64.0, 1, min_count=N * H * W + 1)[2] == [0, N * H * W, 0]


def test_every_sample_in_one_cell():
    """Full contention: N * H * W adds to one count and three sums."""
    N, H, W = 33, 37, 67
    cams, target, poses = _identity(N, H, W)
    depth = (1000 + (np.arange(N * H * W) % 977)).astype(np.uint16).reshape(N, H, W)
    want = DR.cloud_host(depth, cams, target, poses, DR.box(-64.0, 64.0, 1), 1)
    got = _device(depth, cams, target, poses, -64.0, 64.0, 1)
    _same(got, want)
    assert got[1].tolist() == [N * H * W] and got[2] == [1, N * H * W, 0]
    # ... and in one cell of many
    want = DR.cloud_host(depth, cams, target, poses, DR.box(-16.0, 2032.0, 64), 64)         # a cell is 32 wide: |x| < 15.93, |y| < 8.7, 0.97 < z < 1.94
    got = _device(depth, cams, target, poses, -16.0, 2032.0, 64)
    _same(got, want)
    assert got[1].tolist() == [N * H * W]


def test_samples_on_the_faces_of_the_box():
    """G = 2 over [-64, 64]: a step is 1/16.  Four 1x1 frames whose one sample has p = (0, 0, a * 1024 + t) with a = 2^-10: on the low face
    (q = 0), one step below it, on the last step (q = 2047) and on the high face (q = 2048: outside)."""
    cams, target, poses = _identity(4, 1, 1)
    poses[:, 11] = np.float32([-65.0, -65.0625, 62.9375, 63.0])
    depth = np.full((4, 1, 1), 1024, np.uint16)
    bx = DR.box(-64.0, 64.0, 2)
    cell, q = DR.samples_host(depth, cams, target, poses, bx, 2)
    assert cell.reshape(-1).tolist() == [2 + 4, -2, 2 + 4 + 1, -2] and q[0, 0, 0].tolist() == [1024, 1024, 0] and q[2, 0, 0].tolist() == [1024, 1024, 2047]
    want = DR.cloud_host(depth, cams, target, poses, bx, 2)
    got = _device(depth, cams, target, poses, -64.0, 64.0, 2)
    _same(got, want)
    assert got[2] == [2, 2, 2] and got[1].tolist() == [1, 1]
    assert got[0][:, 2].tolist() == [-64.0 + 0.5 / 16, -64.0 + 2047.5 / 16]


def test_alignment_stream_repeat_and_a_dirty_workspace():
    c = dict(N=17, H=37, W=67, kind='fisheye', G=8, stride=1, permille=50, min_count=1)
    depth, cams, target, poses = DR.case(c['N'], c['H'], c['W'], c['kind'], seed=5)
    want = DR.cloud_host(depth, cams, target, poses, DR.box(-2.0, 2.0, 8), 8, 1, 65535, 1, 50, 1)
    kw = dict(stride=1, edge=0.05, min_count=1)
    # the depth maps at an odd element offset of their buffer: 2-byte alignment only
    buf = torch.zeros(depth.size + 1, dtype=torch.int16, device=DEV)
    buf[1:] = _bits(depth).reshape(-1)
    odd = buf[1:].view(depth.shape)
    assert odd.data_ptr() % 4 == 2
    _same(_device(odd, cams, target, poses, -2.0, 2.0, 8, **kw), want, 'odd offset')
    # a numpy array is uploaded
    _same(_device_np(depth, cams, target, poses, kw), want, 'numpy')
    # a stream of its own
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        pts, counts, info = ops.depth_cloud(_bits(depth), cams, target, poses, -2.0, 2.0, grid=8, return_info=True, **kw)
    s.synchronize()
    _same((pts.cpu().numpy(), counts.cpu().numpy(), info), want, 'stream')
    # twice into one dirty workspace
    ws = torch.full((_lib.family('lens').dbw_lens_depth_cloud_workspace_bytes(8),), 0xFF, dtype=torch.uint8, device=DEV)
    first = _device(depth, cams, target, poses, -2.0, 2.0, 8, workspace=ws, **kw)
    assert bool((ws != 0xFF).any())
    second = _device(depth, cams, target, poses, -2.0, 2.0, 8, workspace=ws, **kw)
    _same(first, want, 'dirty workspace')
    _same(second, want, 'second call')
    ws.fill_(0xFF)
    _same(_device(depth, cams, target, poses, -2.0, 2.0, 8, workspace=ws, **kw), want, 'dirty again')
    if hasattr(torch, 'uint16'):
        try:
            u16 = _bits(depth).view(torch.uint16)
        except (RuntimeError, TypeError):
            u16 = None
        if u16 is not None:
            _same(_device(u16, cams, target, poses, -2.0, 2.0, 8, **kw), want, 'uint16')


def _device_np(depth, cams, target, poses, kw):
    pts, counts, info = ops.depth_cloud(depth, cams, target, poses, -2.0, 2.0, grid=8, device=DEV, return_info=True, **kw)
    return pts.cpu().numpy(), counts.cpu().numpy(), info


def test_python_refusals():
    depth, cams, target, poses = DR.case(3, 5, 7, 'pinhole')
    with pytest.raises(RuntimeError, match='runs on the GPU'):
        ops.depth_cloud(torch.from_numpy(depth.view(np.int16)), cams, target, poses, -2, 2)
    with pytest.raises(TypeError, match='torch.int16'):
        ops.depth_cloud(torch.zeros(3, 5, 7, device=DEV), cams, target, poses, -2, 2)
    with pytest.raises(ValueError, match='workspace'):
        ops.depth_cloud(_bits(depth), cams, target, poses, -2, 2, grid=8, workspace=torch.zeros(16, dtype=torch.uint8, device=DEV))


@pytest.fixture(scope='module')
def capture_root(tmp_path_factory):
    root = tmp_path_factory.mktemp('depth')
    DF.write_depth_capture(root, 'cap', dist=DF.MILD)
    return root


def test_the_scene_builds_the_same_cloud_and_world_frame_on_the_device(capture_root):
    scene = DS.CustomScene(capture_root, 'cap', 'train', cloud='depth')
    host, dev = scene.cloud(), scene.cloud(DEV)
    assert dev.is_cuda and torch.equal(dev.cpu(), host) and scene.cloud(DEV) is dev
    fr, cpu = scene.world_frame(DEV), scene.world_frame(None)
    # tests/test_gpu_worldfit.py: the device's frame against the CPU path's
    assert np.abs(np.array(cpu.T_world) - np.array(fr.T_world)).max() < 1e-9 and abs(cpu.S_world - fr.S_world) < 1e-9


def test_one_epoch_of_the_command_line(capture_root, tmp_path):
    import yaml
    cfg = {'dataset': {'name': 'custom', 'tag': 'cap', 'cloud': 'depth'},
           'model': {'name': 'dbw', 'mesh': {'n_blocks': 3, 'R_world': 'auto', 'T_world': 'auto', 'S_world': 'auto', 'txt_size': 16},
                     'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                     'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True,
                                    'opacity_noise': False},
                     'loss': {'rgb_weight': 1, 'perceptual_weight': 0.1, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}},
           'training': {'batch_size': 2, 'n_epoches': 3, 'seed': 3, 'blocks_init': {'min_points': 20}, 'optimizer': {'name': 'adam', 'lr': 1e-3},
                        'scheduler': {'name': 'multi_step'}}}
    path = tmp_path / 'cap.yml'
    with open(path, 'w') as f:
        yaml.safe_dump(cfg, f)
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(ops.__file__)))
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run(['timeout', '-k', '10', '300', sys.executable, '-m', 'dbw_amd.train', '--config', str(path), '--tag', 'run', '--data-root',
                        str(capture_root), '--runs-root', str(tmp_path / 'runs'), '--no-perceptual', '--no-record', '--epochs', '1', '--device', DEV],
                       capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert 'depth_cloud: ' in r.stdout and ' samples of 6 frames' in r.stdout and 'blocks_init: points -> ' in r.stdout and 'R_world: auto -> ' in r.stdout
    run_dir = tmp_path / 'runs' / 'custom' / 'run'
    assert (run_dir / 'depth_cloud.ply').exists() and (run_dir / 'blocks_init.yml').exists() and (run_dir / 'world_frame.yml').exists()
