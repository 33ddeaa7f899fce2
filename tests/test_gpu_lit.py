"""GPU tests of the lit visualisation renders (include/dbw_viz.h, csrc/render_lit.hip, Renderer(shading_type='flat' | 'phong'),
DifferentiableBlocksWorld.renderer_light / predict_synthetic(lit=True), render_views / render_rotated_views).  `-m gpu`.

The yardstick is tests/lit_ref.py -- a torch restatement of the lighting rules -- applied to the ORACLE's fragments and blended by the
oracle's layered_rgb_blend.  It is evaluated AT the vertices the device rendered (the packed scene's fp32 vertices copied to the CPU, as
OracleDBW._verts_through does for the training tests), so both rasterisers see the same numbers, no fragment flips, and the bar is the
project's own for images: max-norm relative error < 1e-4 (REL of tests/test_gpu_model.py) with no pixel left out."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import lit_ref as LR                                            # noqa: E402
import oracle as O                                              # noqa: E402  (checker only)
import dbw_amd                                                  # noqa: E402
from dbw_amd import mesh as M                                   # noqa: E402
from dbw_amd import ops                                         # noqa: E402
from dbw_amd import renderer as RN                              # noqa: E402
from dbw_amd.renderer import Renderer                           # noqa: E402
from dbw_amd.structures import PackedScene                      # noqa: E402

DEV = 'cuda:0'
REL = 1e-4
DIRECTION, KA, KD = [1, 0.25, -1], [0.7, 0.7, 0.7], [0.4, 0.4, 0.4]          # dbw.py:139-140
LIGHT = {'name': 'directional', 'direction': [DIRECTION], 'ambient_color': [KA], 'diffuse_color': [KD], 'specular_color': [[0., 0., 0.]]}
RESOLVE_ATOL = 4e-6         # 16 addends of at most 1.1, at most 15 roundings of at most 2^-24 * 17.6 on either side, divided by 16


def rel_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


def _cfg(n_blocks, ts, fpp=6):
    return {'model': {'name': 'dbw',
                      'mesh': {'n_blocks': n_blocks, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': ts},
                      'renderer': {'faces_per_pixel': fpp, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                      'rend_optim': {'coarse_learning': 1500, 'decimate_txt': 750, 'decimate_factor': 8, 'kill_blocks': True,
                                     'decouple_rendering': True, 'opacity_noise': True},
                      'loss': {'rgb_weight': 1, 'perceptual_weight': 0, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}}}


def _setup(H=40, W=56, nb=5, ts=16, views=3, kill=False):
    """A model with textured, non-trivial blocks (small and large superquadric exponents: slivers included), its cameras, and the
    host-packed scene of the blocks the hard renders keep."""
    torch.manual_seed(227391)
    model = dbw_amd.create_model(_cfg(nb, ts), (H, W))
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        model.sq_eps.add_(torch.randn(model.sq_eps.shape, generator=g) * 2.0)
        model.textures.add_(torch.randn(model.textures.shape, generator=g))
        model.alpha_logit.fill_(2.0)
        if kill:
            model.alpha_logit[1] = -8.0          # sigmoid < 0.01: killed
            model.alpha_logit[3] = -1.0          # kept by training renders, filtered by the hard ones
    model = model.to(DEV).eval()
    R, T, Km = O.synthetic_cameras(views, R_world=O.world_rotation(115, 0, 0))
    inp = {k: v.to(DEV) for k, v in dict(imgs=torch.rand(views, 3, H, W), R=R, T=T, K=Km).items()}
    model._ensure_cameras(inp)
    with torch.no_grad(), model._host_packed_rebuild():
        scene = model.build_blocks_scene(filter_transparent=True)
    return model, scene, inp, (R, T, Km)


def _lit_renderer(model, shading, lights=LIGHT, **over):
    kw = {**model.renderer.init_kwargs, 'lights': lights, 'shading_type': shading, 'background_color': (1, 1, 1), **over}
    r = Renderer(model.img_size, **kw).to(DEV)
    r.update_cameras(device=DEV, K=model.renderer.cameras.K)
    return r


@pytest.mark.parametrize('shading', ['flat', 'phong'])
def test_hard_antialiased_lit_render_matches_the_yardstick(shading):
    """viz_purpose=True: hard, one face per pixel, 4x4 super-samples resolved in the kernel, white background, the reference's light."""
    H, W = 40, 56
    model, scene, inp, (R, T, Km) = _setup(H, W)
    r = _lit_renderer(model, shading, faces_per_pixel=1, sigma=0, detach_bary=False)
    with torch.no_grad():
        img = r.render_packed(scene, inp['R'], inp['T'], viz_purpose=True)
    ref = F.avg_pool2d(LR.render_lit(O, LR.oracle_scene(scene), R, T, Km[0], (4 * H, 4 * W), 0.0, 1, [DIRECTION], KA, KD, shading == 'phong'), 4, 4)
    assert img.shape == (3, 4, H, W)
    err = rel_err(img, ref)
    print(f'{shading}: hard 4x lit render, rel err {err:.3e}; max value {float(img[:, :3].max()):.4f}')
    assert err < REL
    assert 0.01 < float(img[:, 3].mean()) < 0.99                                              # blocks and background are both in the picture
    # the light is seen: the same scene without it differs
    unlit = model.renderer.render_packed(scene, inp['R'], inp['T'], viz_purpose=True)
    assert float((unlit[:, 3] - img[:, 3]).abs().max()) < RESOLVE_ATOL and float((unlit[:, :3] - img[:, :3]).abs().max()) > 0.05


@pytest.mark.parametrize('shading', ['flat', 'phong'])
def test_soft_lit_pass_matches_the_yardstick(shading):
    """The renderer's own faces_per_pixel (6) and sigma (1e-4) at the image size, per-block opacities: the 8x8-tile kernels, ssaa 1."""
    H, W = 40, 56
    model, scene, inp, (R, T, Km) = _setup(H, W)
    r = _lit_renderer(model, shading)
    assert r.faces_per_pixel == 6 and r.sigma == 1e-4
    nb_kept = scene.map_desc.shape[0]
    alpha = torch.linspace(0.35, 0.95, nb_kept).repeat_interleave(model.BNF)
    with torch.no_grad():
        img = r.render_packed(scene, inp['R'], inp['T'], faces_alpha=alpha.to(DEV))
        img_fwd = r(scene, inp['R'], inp['T'], faces_alpha=alpha.to(DEV))
    ref = LR.render_lit(O, LR.oracle_scene(scene), R, T, Km[0], (H, W), 1e-4, 6, [DIRECTION], KA, KD, shading == 'phong', faces_alpha=alpha.repeat(len(R)))
    err = rel_err(img, ref)
    print(f'{shading}: soft lit pass (K 6, sigma 1e-4), rel err {err:.3e}')
    assert err < REL and torch.equal(img, img_fwd)
    # every supported list length has its instantiation: K = 1 (16x16 tiles, ssaa 1) and K = 12 against the yardstick as well
    for K in (1, 12):
        rk = _lit_renderer(model, shading, faces_per_pixel=K)
        with torch.no_grad():
            out = rk.render_packed(scene, inp['R'], inp['T'], faces_alpha=alpha.to(DEV))
        refk = LR.render_lit(O, LR.oracle_scene(scene), R, T, Km[0], (H, W), 1e-4, K, [DIRECTION], KA, KD, shading == 'phong', faces_alpha=alpha.repeat(len(R)))
        errk = rel_err(out, refk)
        print(f'{shading}: K {K}, rel err {errk:.3e}')
        assert errk < REL


def _lit_call(scene, model, R, T, H, W, ssaa, phong, K=1, sigma=0.0):
    cfg = ops.RenderCfg(H, W, K, sigma, 0.001, True, False, scene.faces.shape[0], 1e-8)
    Kmat = model.renderer.cameras.K[0].to(DEV).contiguous()
    return ops.render_scene_lit(scene.verts, scene.maps, None, scene.faces, R, T, Kmat, scene.face_uvs, scene.face_map, scene.map_desc,
                                ops.make_bg((1, 1, 1)), cfg, torch.tensor([DIRECTION], dtype=torch.float32), KA, KD, phong=phong, ssaa=ssaa)


@pytest.mark.parametrize('H,W', [(40, 56), (18, 27)])
def test_in_kernel_resolve_equals_the_full_resolution_render_pooled(H, W):
    """ssaa = 4 against the same entry point with ssaa = 1 at 4H x 4W followed by avg_pool2d; 18 x 27 renders at 72 x 108: no multiple of
    the 16 x 16 tile in either direction."""
    model, scene, inp, _ = _setup(H, W)
    for phong in (False, True):
        with torch.no_grad():
            a = _lit_call(scene, model, inp['R'], inp['T'], H, W, 4, phong)
            b = F.avg_pool2d(_lit_call(scene, model, inp['R'], inp['T'], 4 * H, 4 * W, 1, phong), 4, 4)
        d = float((a - b).abs().max())
        print(f'{H}x{W} phong={phong}: in-kernel resolve vs avg_pool2d, max abs diff {d:.3e}')
        assert a.shape == b.shape == (3, 4, H, W) and d <= RESOLVE_ATOL
        assert 0.01 < float(a[:, 3].mean()) < 0.99 and bool(((a[:, 3] > 0) & (a[:, 3] < 1)).any())      # anti-aliased edges exist
    with pytest.raises(NotImplementedError, match='faces_per_pixel must be 1'):
        _lit_call(scene, model, inp['R'], inp['T'], H, W, 4, False, K=6, sigma=1e-4)


def test_the_light_follows_the_camera():
    """View b alone gives the same picture as view b inside a batch, bit for bit; the renderer's lights are not touched by a call;
    update_lights / reset_default_lights change and restore the picture."""
    model, scene, inp, _ = _setup()
    for shading in ('flat', 'phong'):
        r = _lit_renderer(model, shading, faces_per_pixel=1, sigma=0)
        before = [t.clone() for t in (r.lights.direction, r.lights.ambient_color, r.lights.diffuse_color, r.lights.specular_color)]
        with torch.no_grad():
            batch = r.render_packed(scene, inp['R'], inp['T'], viz_purpose=True)
            for b in range(len(inp['R'])):
                one = r.render_packed(scene, inp['R'][b:b + 1], inp['T'][b:b + 1], viz_purpose=True)
                assert torch.equal(one[0], batch[b]), (shading, b)
            soft_b = r.render_packed(scene, inp['R'], inp['T'])
            assert torch.equal(r.render_packed(scene, inp['R'][1:2], inp['T'][1:2])[0], soft_b[1])
        for t0, t1 in zip(before, (r.lights.direction, r.lights.ambient_color, r.lights.diffuse_color, r.lights.specular_color)):
            assert torch.equal(t0, t1)
        # the views do see the light from different sides: in world space it moves with the camera
        dw = ops.light_dir_world(r.lights.direction, inp['R'])
        assert float((dw[0] - dw[1]).abs().max()) > 0.1
        with torch.no_grad():
            r.update_lights(direction=[[0, 0, -1]], ka=[[0.6, 0.6, 0.6]])
            moved = r.render_packed(scene, inp['R'], inp['T'], viz_purpose=True)
            r.reset_default_lights()
            back = r.render_packed(scene, inp['R'], inp['T'], viz_purpose=True)
        assert float((moved - batch).abs().max()) > 0.01 and torch.equal(back, batch)
        R, T, Km = [t.cpu() for t in (inp['R'], inp['T'], inp['K'])]
        ref = F.avg_pool2d(LR.render_lit(O, LR.oracle_scene(scene), R, T, Km[0], (160, 224), 0.0, 1, [[0, 0, -1]], [0.6] * 3, KD, shading == 'phong'), 4, 4)
        assert rel_err(moved, ref) < REL


def test_ambient_only_lit_render_equals_the_raw_viz_render():
    """kd = 0, ka = 1: the gain is exactly 1, so the new kernel must reproduce the tested unlit visualisation render (which resolves its
    super-samples with avg_pool2d: the order of the 16 additions differs)."""
    model, scene, inp, _ = _setup()
    amb = dict(LIGHT, ambient_color=[[1., 1., 1.]], diffuse_color=[[0., 0., 0.]])
    with torch.no_grad():
        raw = _lit_renderer(model, 'raw', lights={'name': 'ambient'}).render_packed(scene, inp['R'], inp['T'], viz_purpose=True)
        for shading in ('flat', 'phong'):
            lit = _lit_renderer(model, shading, lights=amb).render_packed(scene, inp['R'], inp['T'], viz_purpose=True)
            d = float((lit - raw).abs().max())
            print(f'{shading}: ambient-only lit vs raw viz render, max abs diff {d:.3e}')
            assert d <= RESOLVE_ATOL
        # ... and an AmbientLights renderer with a lit shading type is that picture too
        lit = _lit_renderer(model, 'flat', lights={'name': 'ambient'}).render_packed(scene, inp['R'], inp['T'], viz_purpose=True)
        assert float((lit - raw).abs().max()) <= RESOLVE_ATOL
        # the soft pass: the same list, the same blend -- against the raw renderer's training forward
        soft_raw = _lit_renderer(model, 'raw', lights={'name': 'ambient'}, detach_bary=False).render_packed(scene, inp['R'], inp['T'])
        soft_lit = _lit_renderer(model, 'flat', lights=amb).render_packed(scene, inp['R'], inp['T'])
        assert rel_err(soft_lit, soft_raw) < REL


def test_vertex_normals_are_deterministic_and_match_the_restatement():
    _, scene, _, _ = _setup()
    a = ops.vertex_normals(scene.verts, scene.faces)
    b = ops.vertex_normals(scene.verts, scene.faces)
    assert torch.equal(a, b) and a.shape == scene.verts.shape
    ref = LR.vertex_normals(scene.verts.cpu(), scene.faces.cpu().long())
    d = float((a.cpu() - ref).abs().max())
    print(f'vertex normals vs restatement, max abs diff {d:.3e}')
    assert d <= 1e-6
    assert float((a.norm(dim=-1) - 1).abs().max()) < 1e-5


@pytest.mark.parametrize('sync_free', [False, True])
def test_predict_synthetic_lit_and_unlit(sync_free):
    """Model level, a killed block in the middle and another one filtered by the hard renders: lit=True against the yardstick on the
    scene the method renders (kept blocks at the device's vertices, one 1x1 map per block in its get_fancy_cmap colour, white background,
    the light of dbw.py:139-140); lit=False is the picture of the parent commit, to the bit."""
    H, W, nb = 40, 56, 5
    model, scene, inp, (R, T, Km) = _setup(H, W, nb, kill=True)
    model.sync_free = sync_free
    lit = model.predict_synthetic(inp, None, lit=True)
    unlit = model.predict_synthetic(inp, None, lit=False)
    assert model.sync_free == sync_free and not model.training
    assert torch.equal(unlit, model.predict_synthetic(inp, None))
    keep = (model.get_opacities() > 0.5).nonzero().flatten().cpu()
    assert keep.tolist() == [0, 2, 4] and scene.map_desc.shape[0] == 3
    colors = torch.from_numpy(M.get_fancy_cmap()(torch.linspace(0, 1, nb + 1)[1:][keep].numpy())).float()
    osc = dict(verts=scene.verts.cpu(), faces=scene.faces.cpu().long(), face_uvs=scene.face_uvs.cpu(), face_map=scene.face_map.cpu().long(),
               maps=[c.view(1, 1, 3) for c in colors])
    ref = F.avg_pool2d(LR.render_lit(O, osc, R, T, Km[0], (4 * H, 4 * W), 0.0, 1, [DIRECTION], KA, KD, False), 4, 4)[:, :3]
    err = rel_err(lit, ref)
    print(f'sync_free={sync_free}: predict_synthetic(lit=True), rel err {err:.3e}, max {float(lit.max()):.4f}')
    assert lit.shape == (3, 3, H, W) and err < REL
    # lit=False: what the method did before -- the raw visualisation render of the same flat-coloured scene on white
    desc = PackedScene.describe_maps([(1, 1)] * 3, [(0, 0)] * 3, DEV)[0]
    flat = PackedScene(scene.verts, scene.faces, scene.face_uvs, scene.face_map, desc, colors.to(DEV).reshape(-1).contiguous())
    bg_renderer = Renderer(model.img_size, **{**model.renderer.init_kwargs, 'background_color': (1, 1, 1)})
    bg_renderer.update_cameras(device=DEV, K=model.renderer.cameras.K)
    with torch.no_grad():
        want = bg_renderer.render_packed(flat, inp['R'], inp['T'], viz_purpose=True)[:, :3]
    assert torch.equal(unlit, want) and float(unlit.max()) <= 1 + 1e-5
    # a shaded block is no single colour any more; an unshaded one is
    assert float((lit - unlit).abs().max()) > 0.05


def test_render_views_batches_edges_and_eye_light():
    H, W = 40, 56
    model, scene, inp, _ = _setup(H, W)
    R, T, _ = O.synthetic_cameras(23, R_world=O.world_rotation(115, 0, 0))
    R, T = R.to(DEV), T.to(DEV)
    r = model.renderer_light
    out = RN.render_views(scene, R, T, renderer=r, with_alpha=True)                   # 23 views: batches of 10, 10 and 3
    assert out.shape == (23, 4, H, W) and out.device.type == 'cpu'
    with torch.no_grad():
        for b in (0, 9, 10, 19, 20, 22):
            assert torch.equal(out[b], r(scene, R[b:b + 1], T[b:b + 1], viz_purpose=True)[0].cpu()), b
    # over a background picture
    bkg = torch.rand(3, H, W)
    rec = RN.render_views(scene, R, T, renderer=r, bkg=bkg)
    assert torch.equal(rec, out[:, :3] * out[:, 3:] + (1 - out[:, 3:]) * bkg)
    assert torch.equal(RN.render_views(scene, R, T, renderer=r), out[:, :3])
    # with_edges = draw_edges on the plain result, batch by batch
    colors = torch.rand(scene.faces.shape[0], 3, device=DEV)
    edged = RN.render_views(scene, R, T, renderer=r, with_edges=True, linewidth=2, edge_colors=colors, with_alpha=True)
    for lo in (0, 10, 20):
        n = min(10, 23 - lo)
        want = r.draw_edges(out[lo:lo + n, :3].to(DEV), scene, R=R[lo:lo + n], T=T[lo:lo + n], linewidth=2, colors=colors.repeat(n, 1))
        assert torch.equal(edged[lo:lo + n, :3], want.cpu()) and torch.equal(edged[lo:lo + n, 3], out[lo:lo + n, 3])
    assert float((edged[:, :3] - out[:, :3]).abs().max()) > 0.05
    red = RN.render_views(scene, R[:3], T[:3], renderer=r, with_edges=True)           # default colour: red
    assert float((red - out[:3, :3]).abs().max()) > 0.05
    # eye_light on an ambient renderer = a Phong renderer built by hand (renderer.py:343-351); a directional renderer is kept as it is
    eye = RN.render_views(scene, R, T, renderer=model.renderer, eye_light=True, with_alpha=True)
    hand = _lit_renderer(model, 'phong', faces_per_pixel=1, background_color=model.renderer.background_color)
    assert torch.equal(eye, RN.render_views(scene, R, T, renderer=hand, with_alpha=True))
    assert torch.equal(RN.render_views(scene, R, T, renderer=r, eye_light=True, with_alpha=True), out)
    assert float((eye[:, :3] - RN.render_views(scene, R, T, renderer=model.renderer, with_alpha=True)[:, :3]).abs().max()) > 0.05
    # render_rotated_views: look_at cameras around the scene, clamped to [0, 1]; eye_light there is the light of renderer.py:306-307
    rot = RN.render_rotated_views(scene, renderer=r, n_views=12, elev=30, dist=2.8)
    assert rot.shape == (12, 3, H, W) and float(rot.min()) >= 0 and float(rot.max()) <= 1
    R0 = RN.look_at_view_transform(1, 30, torch.linspace(-180, 180, 12)[:10], device=DEV)[0]
    with torch.no_grad():
        first = r(scene, R0, torch.tensor([[0., 0., 2.8]], device=DEV).expand(10, -1).contiguous(), viz_purpose=True).clamp(0, 1).cpu()
    assert torch.equal(rot[:10], first[:, :3])
    rot_eye = RN.render_rotated_views(scene, renderer=model.renderer, n_views=4, dist=2.8, eye_light=True)
    hand2 = _lit_renderer(model, 'phong', lights=dict(LIGHT, direction=[[0, 0, -1]], ambient_color=[[0.6, 0.6, 0.6]]), faces_per_pixel=1,
                          background_color=model.renderer.background_color)
    assert torch.equal(rot_eye, RN.render_rotated_views(scene, renderer=hand2, n_views=4, dist=2.8))
    with pytest.raises(NotImplementedError):
        RN.render_rotated_views(scene, renderer=model.renderer, R=torch.eye(3), eye_light=True)
