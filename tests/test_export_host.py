"""CPU tests of the export's host side: argument validation of include/dbw_export.h before any launch (the boundary against its
ctypes binding and the library: tests/test_abi_families.py), and the file writers of dbw_amd/export.py (PNG, GIF, PLY, textured OBJ with its atlas)."""
import ctypes
import os

import numpy as np
import pytest
import torch
from PIL import Image

import oracle as O
from dbw_amd import _lib, eval3d, export
from dbw_amd.structures import PackedScene


def _frame_args(**over):
    """Arguments of dbw_frames_u8 with the mandatory pointers non-null (never dereferenced: each call below must fail validation, on the host)."""
    p = ctypes.c_void_p(256)
    a = dict(src=p, N=2, C=4, H=8, W=8, flags=0, bkg3=None, bkg_img=None, mask=None, edge3=None, edge_img=None, out=p, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return list(a.values())


def test_frames_u8_validates_before_any_launch():
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    three = (ctypes.c_float * 3)(0.1, 0.2, 0.3)
    for name in ('src', 'out'):
        assert lib.dbw_frames_u8(*_frame_args(**{name: None})) == -1 and b'null pointer' in lib.dbw_last_error(), name
    for over in (dict(H=0), dict(W=0), dict(W=-3), dict(N=-1), dict(H=1 << 16, W=1 << 16)):
        assert lib.dbw_frames_u8(*_frame_args(**over)) == -1 and b'bad size' in lib.dbw_last_error(), over
    for C in (0, 1, 2, 5, -3):
        assert lib.dbw_frames_u8(*_frame_args(C=C)) == -1 and b'C must be 3 or 4' in lib.dbw_last_error(), C
    # a composite needs the alpha plane
    assert lib.dbw_frames_u8(*_frame_args(C=3, bkg3=three)) == -1 and b'C must be 4' in lib.dbw_last_error()
    assert lib.dbw_frames_u8(*_frame_args(C=3, bkg_img=p)) == -1 and b'C must be 4' in lib.dbw_last_error()
    assert lib.dbw_frames_u8(*_frame_args(bkg3=three, bkg_img=p)) == -1 and b'exclusive' in lib.dbw_last_error()
    # a mask takes exactly one colour, a colour takes a mask
    for over in (dict(mask=p), dict(mask=p, edge3=three, edge_img=p), dict(edge3=three), dict(edge_img=p)):
        assert lib.dbw_frames_u8(*_frame_args(**over)) == -1 and b'exactly one' in lib.dbw_last_error(), over
    assert lib.dbw_frames_u8(*_frame_args(flags=8)) == -1 and b'unknown flag' in lib.dbw_last_error()
    for over in (dict(C=4), dict(C=3, mask=p, edge3=three)):                    # the (N,H,W,3) layout: plain frames only
        assert lib.dbw_frames_u8(*_frame_args(flags=_lib.FRAME_HWC, **over)) in (-1, -2), over
    assert lib.dbw_frames_u8(*_frame_args(flags=_lib.FRAME_HWC, C=3, mask=p, edge3=three)) == -2 and b'no mask' in lib.dbw_last_error()
    assert lib.dbw_frames_u8(*_frame_args(N=0)) == 0                            # nothing to do is not an error, and launches nothing
    with pytest.raises(RuntimeError, match='C must be 3 or 4'):
        _lib.call('dbw_frames_u8', *_frame_args(C=2))


# ---- writers -----------------------------------------------------------------------------------------------------------------------------
def test_png_round_trip_is_exact(tmp_path):
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (18, 27, 3), generator=g, dtype=torch.uint8)
    for src in (img, img.numpy()):
        path = export.save_png(src, tmp_path / 'a.png')
        assert np.array_equal(np.asarray(Image.open(path)), img.numpy())
    f = torch.rand(3, 18, 27, generator=g) * 1.4 - 0.2                          # a float image on the host: the reference's rule
    export.save_png(f, tmp_path / 'b.png')
    assert np.array_equal(np.asarray(Image.open(tmp_path / 'b.png')), (f.clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).numpy())
    with pytest.raises(ValueError):
        export.save_png(torch.zeros(18, 27, 4, dtype=torch.uint8), tmp_path / 'c.png')


def test_video_falls_back_to_a_gif_with_the_frames_and_their_duration(tmp_path):
    g = torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (7, 12, 16, 3), generator=g, dtype=torch.uint8)
    out = export.save_gif(frames, tmp_path / 'traj.gif', fps=20)
    assert out == str(tmp_path / 'traj.gif')
    im = Image.open(out)
    assert im.n_frames == 7 and im.size == (16, 12) and im.info['duration'] == 50 and im.info.get('loop') == 0
    try:
        import imageio  # noqa: F401
        has_imageio = True
    except ImportError:
        has_imageio = False
    out = export.save_video(frames.numpy(), tmp_path / 'b.mp4')
    assert out == str(tmp_path / ('b.mp4' if has_imageio else 'b.gif')) and os.path.exists(out)
    if not has_imageio:
        assert not os.path.exists(tmp_path / 'b.mp4')
        b = Image.open(out)
        assert b.n_frames == 7 and b.info['duration'] == 40                          # 24 fps: 41.67 ms, and a GIF counts hundredths of a second
    # 16 x 12 random pixels hold fewer than 256 colours: the adaptive palette keeps every frame exact
    im.seek(3)
    assert np.array_equal(np.asarray(im.convert('RGB')), frames[3].numpy())


def test_ply_round_trip(tmp_path):
    g = torch.Generator().manual_seed(2)
    pts = torch.randn(3000, 3, generator=g) * 40
    path = export.save_ply(tmp_path / 'gt.ply', pts)
    back = eval3d.read_ply_points(path)
    assert back.shape == (3000, 3) and back.dtype == np.float64 and np.array_equal(back, pts.double().numpy())
    assert eval3d.read_ply_points(export.save_ply(tmp_path / 'e.ply', np.zeros((0, 3)))).shape == (0, 3)


def _two_map_scene(seed=3):
    """A hand-built scene: an icosphere on a 12 x 10 map with circular padding (3, 2), a subdivided plane on a 9 x 20 map without."""
    g = torch.Generator().manual_seed(seed)
    v0, f0 = O.get_icosphere(1)
    v1, f1 = O.get_plane()
    v1, f1 = O.subdivide(v1, f1)
    maps = [torch.rand(12, 10, 3, generator=g), torch.rand(9, 20, 3, generator=g)]
    pads = [(3, 2), (0, 0)]
    uv0, uv1 = torch.rand(len(f0), 3, 2, generator=g), torch.rand(len(f1), 3, 2, generator=g)
    uv0[0], uv1[0] = torch.tensor([[0., 0.], [1., 1.], [1., 0.]]), torch.tensor([[0., 1.], [1., 1.], [0.5, 0.]])      # the corners
    desc, _ = PackedScene.describe_maps([m.shape[:2] for m in maps], pads, 'cpu')
    scene = PackedScene(torch.cat([v0, v1 + 2.5]).float(), torch.cat([f0, f1 + len(v0)]).to(torch.int32), torch.cat([uv0, uv1]).float(),
                        torch.cat([torch.zeros(len(f0)), torch.ones(len(f1))]).to(torch.int32), desc, torch.cat([m.reshape(-1) for m in maps]))
    return scene, maps, pads


def _parse_obj(path):
    v, vt, f, other = [], [], [], []
    for line in open(path):
        tok = line.split()
        if tok[0] == 'v':
            v.append([float(x) for x in tok[1:]])
        elif tok[0] == 'vt':
            vt.append([float(x) for x in tok[1:]])
        elif tok[0] == 'f':
            f.append([[int(i) for i in t.split('/')] for t in tok[1:]])
        else:
            other.append(tok)
    return np.array(v), np.array(vt), np.array(f), other


def test_obj_files_parse_back(tmp_path):
    scene, maps, pads = _two_map_scene()
    path = export.save_scene_as_obj(scene, tmp_path / 'mesh.obj')
    assert sorted(os.listdir(tmp_path)) == ['mesh.mtl', 'mesh.obj', 'mesh.png']
    v, vt, f, other = _parse_obj(path)
    F_ = scene.faces.shape[0]
    assert v.shape == (scene.verts.shape[0], 3) and vt.shape == (3 * F_, 2) and f.shape == (F_, 3, 2)
    assert np.allclose(v, scene.verts.numpy(), rtol=0, atol=1e-6)
    assert np.array_equal(f[:, :, 0] - 1, scene.faces.numpy()) and np.array_equal(f[:, :, 1] - 1, np.arange(3 * F_).reshape(F_, 3))
    assert vt.min() >= 0 and vt.max() <= 1
    assert ['mtllib', 'mesh.mtl'] in other and ['usemtl', 'mesh'] in other
    assert other.index(['mtllib', 'mesh.mtl']) == 0 and [t[0] for t in other].index('usemtl') > 0
    mtl = open(tmp_path / 'mesh.mtl').read().split('\n')
    assert mtl[0] == 'newmtl mesh' and 'map_Kd mesh.png' in mtl
    atlas = np.asarray(Image.open(tmp_path / 'mesh.png'))
    assert atlas.dtype == np.uint8 and atlas.ndim == 3 and atlas.shape[2] == 3 and max(atlas.shape) <= 512
    # every map sits in the atlas with its padding columns materialised, texel for texel (8-bit truncation)
    a, _ = export.build_atlas(scene)
    assert np.array_equal(atlas, (a.clamp(0, 1) * 255).to(torch.uint8).numpy())
    padded0 = torch.cat([maps[0][:, -3:], maps[0], maps[0][:, :2]], 1)
    (r0, c0), (r1, c1) = export._shelf_layout([(12, 15), (9, 20)])[0]
    assert torch.equal(a[r0:r0 + 12, c0:c0 + 15], padded0) and torch.equal(a[r1:r1 + 9, c1:c1 + 20], maps[1]) and (r0, c0) != (r1, c1)
    # a Meshes-free round trip through the loader
    back = export.load_obj_as_scene(path)
    assert back.map_desc.shape[0] == 1 and back.faces.shape == scene.faces.shape and torch.equal(back.faces, scene.faces)
    assert tuple(back.map_desc[0, 1:5].tolist()) == (atlas.shape[0], atlas.shape[1], 0, 0)


def test_sampling_the_atlas_reads_the_same_texels(tmp_path):
    """The atlas decoded from the PNG, sampled at the remapped UVs, against the original maps sampled through the oracle's sampler at
    4000 random (face, barycentric) points: |diff| <= 1/255 + 1e-4 -- truncation loses less than 1/255 per texel, the bilinear weights
    are convex, and 1e-4 covers the fp32 UV remap over <= 512 texels."""
    scene, maps, pads = _two_map_scene(seed=4)
    back = export.load_obj_as_scene(export.save_scene_as_obj(scene, tmp_path / 's.obj'))
    g = torch.Generator().manual_seed(5)
    n, F_ = 4000, scene.faces.shape[0]
    face = torch.randint(0, F_, (n,), generator=g)
    n0 = int((scene.face_map == 0).sum())
    face[:6] = torch.tensor([0, 0, 0, n0, n0, n0])                                       # the faces whose corners are the maps' corners
    bary = torch.rand(n, 3, generator=g)
    bary = bary / bary.sum(-1, keepdim=True)
    bary[:6] = torch.eye(3).repeat(2, 1)
    p2f, bw = face.view(1, n, 1, 1), bary.view(1, n, 1, 1, 3)
    padded = [torch.cat([m[:, m.shape[1] - pl:], m, m[:, :pr]], 1) for m, (pl, pr) in zip(maps, pads)]      # what the kernels sample
    want = O.sample_textures(p2f, bw, scene.face_uvs, scene.face_map.long(), padded, F_)
    atlas = back.maps.view(int(back.map_desc[0, 1]), int(back.map_desc[0, 2]), 3)
    got = O.sample_textures(p2f, bw, back.face_uvs, back.face_map.long(), [atlas], F_)
    d = float((got - want).abs().max())
    print(f'atlas sampling vs the original maps: max abs diff {d:.3e}')
    assert set(scene.face_map[face].tolist()) == {0, 1}
    assert d <= 1 / 255 + 1e-4
