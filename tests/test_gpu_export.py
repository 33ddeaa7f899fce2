"""GPU tests of the qualitative evaluation and export: the frame conversion kernel (dbw_frames_u8) against the host build of the header it
compiles, the 8-bit view pipeline (render_views_u8 / render_rotated_views_u8) against the fp32 one followed by the reference's
quantisation, the files qualitative_eval writes, the OBJ round trip and Trainer.evaluate.  `-m gpu`.

Bounds: bytes made from the same floats are compared EXACTLY.  Where the 8-bit path resolves its 4x4 super-samples in the lit kernel and
the fp32 path with avg_pool2d (an unlit renderer), a byte b made from the float x' must satisfy q(x - tol) <= b <= q(x + tol) for the
other path's float x, tol = RESOLVE_ATOL of tests/test_gpu_lit.py (derived there): q is monotone and |x' - x| <= tol."""
import os
import types

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

import oracle as O                                              # noqa: E402  (checker only)
import dbw_amd                                                  # noqa: E402
import frame_ref as FR                                          # noqa: E402
from dbw_amd import eval3d, export, ops                         # noqa: E402
from dbw_amd import renderer as RN                              # noqa: E402
from test_gpu_lit import RESOLVE_ATOL, _setup                   # noqa: E402

DEV = 'cuda:0'
ATLAS_ATOL = 1 / 255 + 1e-4         # truncation loses less than 1/255 per texel, bilinear weights are convex; 1e-4: the fp32 UV remap


def _rand(shape, g, lo=-0.2, hi=1.2):
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _within(b, x, tol):
    """q(x - tol) <= b <= q(x + tol), b (..,H,W,3) uint8, x (..,3,H,W) fp32 (CPU)."""
    lo, hi = FR.quantise(x - tol).movedim(-3, -1), FR.quantise(x + tol).movedim(-3, -1)
    return bool(((lo <= b) & (b <= hi)).all())


def _png(path):
    return torch.from_numpy(np.array(Image.open(path).convert('RGB')))


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', [(40, 56), (18, 27)])
def test_frames_u8_equals_the_host_header_exactly(H, W):
    g = torch.Generator().manual_seed(H + W)
    N = 3
    src = _rand((N, 4, H, W), g)
    k255 = torch.randint(0, 256, (N, 4, H, W), generator=g).float() / 255
    pick = torch.rand(N, 4, H, W, generator=g) < 0.3
    src = torch.where(pick, k255, src)                                          # exact k/255 among values inside and outside [0, 1]
    src[:, 3] = torch.where(pick[:, 3], k255[:, 3], torch.rand(N, H, W, generator=g))
    src[0, 0, 0, :3] = torch.tensor([float('nan'), float('inf'), -0.0])
    bkg_img, bkg3 = torch.rand(3, H, W, generator=g), [0.25, 1.0, 0.6]
    mask = (torch.randint(0, 17, (N, 1, H, W), generator=g).float() / 16) * (torch.rand(N, 1, H, W, generator=g) < 0.3)
    col3, col_img = [0.3, 0.3, 0.3], torch.rand(N, 3, H, W, generator=g)
    rgb = src[:, :3].contiguous()
    d = lambda t: t.to(DEV) if torch.is_tensor(t) else t
    cases = [dict(src=src), dict(src=rgb), dict(src=rgb.permute(0, 2, 3, 1).contiguous(), hwc=True), dict(src=src, clamp_input=True)]
    for bkg in (bkg3, bkg_img):
        cases += [dict(src=src, bkg=bkg), dict(src=src, bkg=bkg, clamp_input=True)]
        for col in (col3, col_img):
            cases += [dict(src=src, bkg=bkg, mask=mask, edge_color=col), dict(src=src, bkg=bkg, mask=mask, edge_color=col, edge_first=True)]
    for col in (col3, col_img):
        cases += [dict(src=rgb, mask=mask, edge_color=col), dict(src=src, mask=mask, edge_color=col)]
    for kw in cases:
        got = ops.frames_u8(**{k: d(v) for k, v in kw.items()})
        assert got.shape == (N, H, W, 3) and got.dtype == torch.uint8 and got.is_cuda
        assert torch.equal(got.cpu(), FR.frames_u8_host(**kw)), {k: (tuple(v.shape) if torch.is_tensor(v) else v) for k, v in kw.items()}
    # a source off the 16-byte alignment goes pixel by pixel: same bytes; `out=` is filled in place
    flat = torch.zeros(src.numel() + 1, device=DEV)
    flat[1:] = src.reshape(-1).to(DEV)
    out = torch.zeros(N, H, W, 3, dtype=torch.uint8, device=DEV)
    assert ops.frames_u8(flat[1:].view(N, 4, H, W), bkg=d(bkg_img), out=out) is out
    assert torch.equal(out.cpu(), FR.frames_u8_host(src, bkg=bkg_img))
    assert torch.equal(ops.frames_u8(src[:0].to(DEV)).cpu(), torch.zeros(0, H, W, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='C must be 4'):
        ops.frames_u8(d(rgb), bkg=bkg3)


def test_frames_u8_reproduces_the_reference_bytes(golden_dir):
    z = np.load(os.path.join(golden_dir, 'frames_u8.npz'))
    for tag in sorted(k[:-3] for k in z.files if k.endswith('_in')):
        x = torch.from_numpy(z[f'{tag}_in'])
        assert torch.equal(ops.frames_u8(x[None].to(DEV))[0].cpu(), torch.from_numpy(z[f'{tag}_u8'])), tag


# ---- the view pipeline ---------------------------------------------------------------------------------------------------------------------
def _scenes(views=5, H=40, W=56, kill=True):
    model, blocks, inp, cams = _setup(H, W, views=views, kill=kill)
    with torch.no_grad(), model._host_packed_rebuild():
        full = model.build_scene(filter_transparent=True)
    return model, blocks, full, inp


@pytest.mark.parametrize('H,W', [(40, 56), (18, 27)])
def test_render_views_u8_with_a_lit_renderer_equals_the_quantised_fp32_views(H, W):
    model, blocks, full, inp = _scenes(H=H, W=W)
    R, T, rl = inp['R'], inp['T'], model.renderer_light
    g = torch.Generator().manual_seed(7)
    bkg, bkg_small = torch.rand(3, H, W, generator=g), torch.rand(3, H // 2, W // 2, generator=g)
    per_face = model.get_scene_face_colors(filter_transparent=True, w_env=False)
    q = lambda x: FR.quantise(x).permute(0, 2, 3, 1)
    for kw in (dict(), dict(bkg=bkg), dict(bkg=bkg_small), dict(with_edges=True), dict(with_edges=True, edge_colors=(0.3, 0.3, 0.3), linewidth=0.7),
               dict(with_edges=True, edge_colors=per_face), dict(with_edges=True, edge_colors=per_face, bkg=bkg)):
        got = RN.render_views_u8(blocks, R, T, renderer=rl, **kw)
        assert got.shape == (len(R), H, W, 3) and got.dtype == torch.uint8 and not got.is_cuda and got.is_pinned()
        assert torch.equal(got, q(RN.render_views(blocks, R, T, renderer=rl, **kw))), sorted(kw)
    # eye_light swaps the model's unlit renderer for a Phong one on both paths
    got = RN.render_views_u8(full, R, T, renderer=model.renderer, eye_light=True, bkg=bkg)
    assert torch.equal(got, q(RN.render_views(full, R, T, renderer=model.renderer, eye_light=True, bkg=bkg)))
    assert 0.02 < float((got != q(RN.render_views(full, R, T, renderer=model.renderer, bkg=bkg))).float().mean())      # (the light is seen)
    # the rotated views: the same kernel, the clamp in front of the composite included
    for kw in (dict(), dict(bkg=bkg)):
        got = RN.render_rotated_views_u8(blocks, renderer=rl, n_views=4, **kw)
        assert torch.equal(got, q(RN.render_rotated_views(blocks, renderer=rl, n_views=4, **kw))), sorted(kw)


def test_render_views_u8_with_the_unlit_renderer_is_within_the_resolve_bound():
    model, blocks, full, inp = _scenes()
    R, T = inp['R'], inp['T']
    bkg = torch.rand(3, 40, 56, generator=torch.Generator().manual_seed(8))
    for scene, kw in ((full, dict()), (blocks, dict(bkg=bkg)), (full, dict(with_edges=True))):
        got = RN.render_views_u8(scene, R, T, renderer=model.renderer, **kw)
        x = RN.render_views(scene, R, T, renderer=model.renderer, **kw)
        n_diff = int((got != FR.quantise(x).permute(0, 2, 3, 1)).sum())
        print(f'unlit renderer {sorted(kw)}: {n_diff} of {got.numel()} bytes differ from the quantised avg_pool2d path')
        assert _within(got, x, RESOLVE_ATOL)
    got = RN.render_rotated_views_u8(full, renderer=model.renderer, n_views=4)
    assert _within(got, RN.render_rotated_views(full, renderer=model.renderer, n_views=4), RESOLVE_ATOL)


def test_render_views_u8_does_not_depend_on_chunking_and_fills_out_in_place():
    model, blocks, full, inp = _scenes(views=5)
    R, T = inp['R'], inp['T']
    for scene, r, kw in ((full, model.renderer, dict()), (blocks, model.renderer_light, dict(with_edges=True, bkg=torch.rand(3, 40, 56)))):
        ref = RN.render_views_u8(scene, R, T, renderer=r, chunk=len(R), **kw)
        for chunk in (1, 2, None):
            assert torch.equal(RN.render_views_u8(scene, R, T, renderer=r, chunk=chunk, **kw), ref), chunk
        assert len(torch.unique(ref.view(len(R), -1), dim=0)) == len(R)                 # five different views
    out = torch.zeros(5, 40, 56, 3, dtype=torch.uint8).pin_memory()
    assert RN.render_views_u8(full, R, T, renderer=model.renderer, out=out, chunk=2) is out
    assert torch.equal(out, RN.render_views_u8(full, R, T, renderer=model.renderer))
    assert torch.equal(RN.render_rotated_views_u8(full, renderer=model.renderer, n_views=5, chunk=2), RN.render_rotated_views_u8(full, renderer=model.renderer, n_views=5))
    with pytest.raises(ValueError, match='uint8 host tensor'):
        RN.render_views_u8(full, R, T, renderer=model.renderer, out=torch.zeros(5, 40, 56, 3))
    # the chunk size follows the workspace budget
    assert RN._views_per_chunk(full, (40, 56), 240) >= 10
    budget, RN.FRAME_WORKSPACE_BYTES = RN.FRAME_WORKSPACE_BYTES, 1
    try:
        assert RN._views_per_chunk(full, (40, 56), 240) == 1
    finally:
        RN.FRAME_WORKSPACE_BYTES = budget


# ---- the model's scenes and files ------------------------------------------------------------------------------------------------------------
def test_build_scene_without_the_dome_and_with_the_reduced_ground():
    model, blocks, full, inp = _scenes()
    with torch.no_grad(), model._host_packed_rebuild():
        again = model.build_scene(filter_transparent=True, w_bkg=True, reduce_ground=False)
        clean = model.build_scene(filter_transparent=True, w_bkg=False, reduce_ground=True)
        no_dome = model.build_scene(filter_transparent=True, w_bkg=False)
        reduced = model.build_scene(filter_transparent=True, reduce_ground=True)
        env_v = model._build_env_variant(True, False)
        env = model.build_env_scene()
    for a, b in ((again, full), (env_v, env)):
        for name in ('verts', 'faces', 'face_uvs', 'face_map', 'map_desc', 'maps'):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
    nvb, nfb, nfg = model._bkg_verts.shape[0], model._n_bkg_faces, model._n_ground_faces
    nvg = model._ground_base.shape[0]
    assert clean.verts.shape[0] == full.verts.shape[0] - nvb and clean.faces.shape[0] == full.faces.shape[0] - nfb
    assert clean.map_desc.shape[0] == full.map_desc.shape[0] - 1 and int(clean.faces.max()) == clean.verts.shape[0] - 1
    assert torch.equal(clean.face_uvs, full.face_uvs[nfb:]) and torch.equal(clean.faces, full.faces[nfb:] - nvb)        # the UVs are unchanged
    assert torch.equal(no_dome.verts, full.verts[nvb:]) and torch.equal(clean.verts[nvg:], full.verts[nvb + nvg:])      # the blocks stay
    # the ground plane (y = 0 in its own frame) shrinks by 3 / z_far about the image of its origin, in every direction of the plane
    origin = ops.posed_mesh(model.R_6d_ground, model.T_ground, torch.zeros(1, 3, device=DEV), *model._world_consts())
    torch.testing.assert_close(clean.verts[:nvg] - origin.detach(), (full.verts[nvb:nvb + nvg] - origin.detach()) * (3 / model.z_far), rtol=0, atol=1e-5)
    assert torch.equal(reduced.verts[nvb:nvb + nvg], clean.verts[:nvg]) and torch.equal(reduced.verts[:nvb], full.verts[:nvb])
    assert reduced.faces.shape == full.faces.shape and nfg > 0


def test_obj_export_renders_like_the_scene(tmp_path):
    model, blocks, full, inp = _scenes()
    with torch.no_grad():                               # contrast on the dome and the ground too (their maps start as a flat grey)
        g = torch.Generator().manual_seed(12)
        model.texture_bkg.add_(torch.randn(model.texture_bkg.shape, generator=g).to(DEV) * 2)
        model.texture_ground.add_(torch.randn(model.texture_ground.shape, generator=g).to(DEV) * 2)
        with model._host_packed_rebuild():
            full = model.build_scene(filter_transparent=True)
    back = export.load_obj_as_scene(export.save_scene_as_obj(full, tmp_path / 'mesh_full.obj'), device=DEV)
    assert back.map_desc.shape[0] == 1 and full.map_desc.shape[0] > 2
    assert torch.equal(back.faces, full.faces) and torch.equal(back.verts, full.verts)
    blank = export.load_obj_as_scene(tmp_path / 'mesh_full.obj', device=DEV)
    blank.maps = torch.full_like(blank.maps, 0.5)
    with torch.no_grad():
        a = model.renderer.render_packed(full, inp['R'], inp['T'], viz_purpose=True)
        b = model.renderer.render_packed(back, inp['R'], inp['T'], viz_purpose=True)
        c = model.renderer.render_packed(blank, inp['R'], inp['T'], viz_purpose=True)
    d = float((a - b).abs().max())
    print(f'OBJ re-import, hard 4x render: max abs diff {d:.3e} (bound {ATLAS_ATOL:.3e}); with a grey atlas {float((a - c).abs().max()):.3e}')
    assert d <= ATLAS_ATOL
    assert float((a - c).abs().max()) > 0.1             # (the check sees the textures: a grey atlas is far away)


class _Loader(list):
    """Two batches of (inp, labels) with the attributes qualitative_eval reads from a DataLoader."""
    batch_size = 2


def _loader(inp, pc_gt=True):
    ld = _Loader([({k: v[i:i + 2] for k, v in inp.items()}, None) for i in (0, 2)])
    ld.dataset = types.SimpleNamespace(pc_gt=torch.randn(5000, 3, generator=torch.Generator().manual_seed(9))) if pc_gt else types.SimpleNamespace()
    return ld


def _video_ext():
    try:
        import imageio  # noqa: F401
        return 'mp4'
    except ImportError:
        return 'gif'


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_qualitative_eval_writes_the_file_set(tmp_path):
    model, blocks, full, inp = _scenes(views=4, kill=True)
    H, W = model.img_size
    loader = _loader(inp)
    model.train()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    params = {k: v.detach().clone() for k, v in model.named_parameters()}
    model.qualitative_eval(loader, DEV, path=tmp_path, NV=6)
    assert model.training
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert all(torch.equal(p.detach(), params[k]) and p.grad is None for k, p in model.named_parameters())
    ext = _video_ext()
    meshes = ['mesh.mtl', 'mesh.obj', 'mesh.png', 'mesh_full.mtl', 'mesh_full.obj', 'mesh_full.png', f'rotated_mesh.{ext}']
    textures = [os.path.join('textures', n) for n in ['bkg.png', 'ground.png'] + [f'block_{k:02d}.png' for k in range(5)]]
    per_input = [f'{i}_{n}' for i in range(4) for n in ('inp.png', 'rec.png', 'rec_col.png', 'rec_col_inp.png', 'rec_syn_nobkg.png',
                                                         'rec_syn_nobkg_edged.png', f'rec_traj.{ext}', f'rec_traj_syn.{ext}')]
    assert _files(tmp_path) == sorted(meshes + textures + per_input + ['gt.ply'])
    # the stills
    assert torch.equal(_png(tmp_path / '0_inp.png'), FR.quantise(inp['imgs'][0].cpu()).permute(1, 2, 0))
    assert torch.equal(_png(tmp_path / '3_inp.png'), FR.quantise(inp['imgs'][3].cpu()).permute(1, 2, 0))
    model.eval()
    with torch.no_grad():
        rec = model.renderer.render_packed(full, inp['R'][:1], inp['T'][:1], viz_purpose=True)[:, :3].cpu()
        syn = model.predict_synthetic({k: v[:1] for k, v in inp.items()}, lit=True).cpu()
    assert _within(_png(tmp_path / '0_rec.png')[None], rec, RESOLVE_ATOL)
    assert torch.equal(_png(tmp_path / '0_rec_syn_nobkg.png')[None], FR.quantise(syn).permute(0, 2, 3, 1))               # (the lit kernel on both sides)
    for a, b in (('0_rec.png', '0_rec_col.png'), ('0_inp.png', '0_rec_col_inp.png'), ('0_rec_syn_nobkg.png', '0_rec_syn_nobkg_edged.png')):
        frac = float((_png(tmp_path / a) != _png(tmp_path / b)).any(-1).float().mean())
        assert 0 < frac < 1, (a, b, frac)                                              # the wireframe is drawn, over a part of the picture
    # the ground-truth points: 3000 of them, the draw of seed 123
    pts = eval3d.read_ply_points(tmp_path / 'gt.ply')
    pick = torch.randperm(5000, generator=torch.Generator().manual_seed(123))[:3000]
    assert pts.shape == (3000, 3) and np.array_equal(pts, loader.dataset.pc_gt[pick].double().numpy())
    # the videos
    for name in ('rotated_mesh', '0_rec_traj', '2_rec_traj_syn'):
        if ext == 'gif':
            im = Image.open(tmp_path / f'{name}.gif')
            assert im.n_frames == 6 and im.size == (W, H), name
    # the textures: the prepared maps, quantised; and the sigmoid of the parameters within the texture preparation's own tolerance
    for name, param in (('bkg', model.texture_bkg), ('ground', model.texture_ground), ('block_03', model.textures[3:4])):
        png = _png(tmp_path / 'textures' / f'{name}.png')
        maps = ops.texture_prep(param.detach().contiguous())[0][0].cpu()
        assert torch.equal(png, FR.quantise(maps))
        sig = torch.sigmoid(param.detach().cpu())[0]
        tol = 1e-6 * float(sig.abs().max())            # tests/test_gpu_model.py::test_texture_prep_and_decimation: rel_err(maps, sigmoid) < 1e-6 of the largest value
        assert bool(((FR.quantise(sig - tol) <= png) & (png <= FR.quantise(sig + tol))).all()), name
    # the meshes: everything, and the clean one (no dome, reduced ground); a block filtered at 0.5 is in neither
    n_v = lambda p: sum(1 for line in open(p) if line.startswith('v '))
    assert n_v(tmp_path / 'mesh_full.obj') == full.verts.shape[0] and n_v(tmp_path / 'mesh.obj') == full.verts.shape[0] - model._bkg_verts.shape[0]
    assert full.verts.shape[0] == model._bkg_verts.shape[0] + model._ground_base.shape[0] + 3 * model._block_nv
    # no dataset.pc_gt: no gt.ply, everything else
    other = tmp_path / 'no_gt'
    model.qualitative_eval(_loader(inp, pc_gt=False), DEV, path=other, NV=6)
    assert _files(other) == sorted(meshes + textures + per_input) and not model.training


def test_qualitative_eval_stops_after_the_meshes_when_every_block_is_transparent(tmp_path):
    model, blocks, full, inp = _scenes(views=4)
    with torch.no_grad():
        model.alpha_logit.fill_(-1.0)
    model.eval()
    model.qualitative_eval(_loader(inp), DEV, path=tmp_path, NV=6)
    ext = _video_ext()
    assert _files(tmp_path) == sorted(['mesh.mtl', 'mesh.obj', 'mesh.png', 'mesh_full.mtl', 'mesh_full.obj', 'mesh_full.png', f'rotated_mesh.{ext}']
                                      + [os.path.join('textures', n) for n in ['bkg.png', 'ground.png'] + [f'block_{k:02d}.png' for k in range(5)]])
    assert not model.training


def test_trainer_evaluate_writes_the_scores(tmp_path):
    from dbw_amd.trainer import Trainer
    model, blocks, full, inp = _scenes(views=4, kill=True)
    cfg = {'training': {'batch_size': 2, 'n_epoches': 1, 'seed': 3, 'optimizer': {'name': 'adam', 'lr': 1e-3}, 'scheduler': {'name': 'multi_step'}}}
    model.train()
    tr = Trainer(cfg, model, inp)
    loader = _loader(inp)
    scores = tr.evaluate(loader, tmp_path / 'run')
    want = model.quantitative_eval(loader, DEV, hard_inference=True)
    assert list(scores) == list(want) and scores['n_blocks'] == 3
    lines = open(tmp_path / 'run' / 'final_scores.tsv').read().split('\n')
    assert len(lines) == 3 and lines[2] == '' and lines[0].split('\t') == list(want)
    vals = lines[1].split('\t')
    assert len(vals) == len(want) and all('{:.5f}'.format(float(v)) == s for v, s in zip(want.values(), vals))
    assert os.path.exists(tmp_path / 'run' / 'quali_eval' / '0_rec.png') and os.path.exists(tmp_path / 'run' / 'quali_eval' / 'mesh.obj')
    assert not os.path.exists(tmp_path / 'run' / 'dtu_scores.tsv')
