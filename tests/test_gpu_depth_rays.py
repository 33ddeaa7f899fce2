"""GPU: the depth rays (csrc/depth_cloud.hip depth_rays_kernel, dbw_lens_depth_rays of include/dbw_lens.h) against the host build of the
same header (tests/host_depth_rays.cpp) byte for byte: frames from 1x1, 17 and 33 frames across the 16 of a launch, both strides, the three
camera kinds, the edge rule off and on -- and the scene's rays built on the device against those built in numpy."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import depth_fixture as DF                                      # noqa: E402
import depth_ref as DR                                          # noqa: E402
import freespace_ref as FR                                      # noqa: E402
from dbw_amd import ops                                         # noqa: E402
from dbw_amd import dataset as DS                               # noqa: E402

DEV = 'cuda'
SHAPES = [(1, 1), (2, 2), (5, 7), (24, 32), (37, 67)]
CASES = [dict(N=N, H=H, W=W, kind=DR.KINDS[(k + a) % 3], stride=(1, 3)[(k + a // 2) % 2], permille=(0, 50)[(k + a) % 2])
         for a, N in enumerate((1, 3, 17, 33)) for k, (H, W) in enumerate(SHAPES)]
CASES += [dict(N=3, H=24, W=32, kind=kind, stride=stride, permille=permille)
          for kind, stride, permille in (('pinhole', 1, 50), ('radtan', 3, 0), ('fisheye', 1, 50), ('fisheye', 3, 0), ('radtan', 1, 50), ('pinhole', 3, 0))]


def _id(c):
    return '{N}x{H}x{W}-{kind}-s{stride}-e{permille}'.format(**c)


def _bits(depth):
    return torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(DEV)


@pytest.mark.parametrize('c', CASES, ids=_id)
def test_the_kernel_gives_the_bytes_of_the_host_build(c):
    depth, cams, target, poses = DR.case(c['N'], c['H'], c['W'], c['kind'])
    want = FR.host_depth_rays(depth, cams, target, poses, 1, 65535, c['stride'], c['permille'])
    got = ops.depth_rays(_bits(depth), cams, target, poses, stride=c['stride'], edge=c['permille'] / 1000)
    Hs, Ws = -(-c['H'] // c['stride']), -(-c['W'] // c['stride'])
    assert got.shape == (c['N'], Hs, Ws, 4) and got.dtype == torch.int32
    g = got.cpu().numpy().view(np.uint32)
    assert g.tobytes() == want.tobytes(), _id(c)
    frame = g[..., 3].view(np.int32)
    n = np.broadcast_to(np.arange(c['N'])[:, None, None], frame.shape)
    assert ((frame == n) | (frame == -1)).all() and not g[frame == -1][:, :3].any()
    if c['H'] >= 24:
        assert 0.2 < (frame >= 0).mean() <= 1.0
    ends, fr = ops.depth_rays_compact(got)
    assert ends.dtype == torch.float32 and fr.dtype == torch.int32 and ends.shape == (int((frame >= 0).sum()), 3)
    assert torch.equal(fr.cpu(), torch.from_numpy(frame[frame >= 0])) and bool(torch.isfinite(ends).all())


def test_range_edge_rule_a_numpy_upload_and_the_refusals():
    depth, cams, target, poses = DR.case(17, 37, 67, 'radtan', seed=5)
    for d_range, permille in (((1, 65535), 0), ((1, 65535), 50), ((2000, 3000), 0), ((2000, 3000), 200)):
        want = FR.host_depth_rays(depth, cams, target, poses, d_range[0], d_range[1], 1, permille)
        got = ops.depth_rays(depth, cams, target, poses, d_range=d_range, edge=permille / 1000, device=DEV).cpu().numpy().view(np.uint32)
        assert got.tobytes() == want.tobytes(), (d_range, permille)
    loose = FR.host_depth_rays(depth, cams, target, poses)[..., 3].view(np.int32)
    strict = FR.host_depth_rays(depth, cams, target, poses, permille=50)[..., 3].view(np.int32)
    assert (strict >= 0).sum() < (loose >= 0).sum() and ((loose >= 0) | (strict < 0)).all()          # the edge rule only drops
    with pytest.raises(RuntimeError, match='runs on the GPU'):
        ops.depth_rays(torch.from_numpy(depth.view(np.int16)), cams, target, poses)
    with pytest.raises(TypeError, match='torch.int16'):
        ops.depth_rays(torch.zeros(17, 37, 67, device=DEV), cams, target, poses)
    with pytest.raises(ValueError, match='d_range'):
        ops.depth_rays(_bits(depth), cams, target, poses, d_range=(0, 10))


def test_the_scene_builds_the_same_rays_on_the_device(tmp_path):
    DF.write_depth_capture(tmp_path, 'cap', dist=DF.MILD)
    scene = DS.CustomScene(tmp_path, 'cap', 'train', cloud='depth')
    host, dev = scene.rays(), scene.rays(DEV)
    assert all(d.is_cuda for d in dev) and scene.rays(DEV)[0] is dev[0]
    for h, d in zip(host, dev):
        assert h.dtype == d.dtype and torch.equal(d.cpu(), h)
    assert scene.rays_info == {'rays': host[0].shape[0], 'samples': 6 * 48 * 64, 'frames': 6} and host[0].shape[0] > 0.5 * 6 * 48 * 64
