"""CPU tests of the lit visualisation renders' host side: argument validation of include/dbw_viz.h before any launch (the boundary
against its ctypes binding and the library: tests/test_abi_families.py), the Renderer's light / shading keywords and refusals, and the view-trajectory helpers."""
import ctypes

import pytest
import torch

import oracle as O
import dbw_amd
from dbw_amd import _lib, ops
from dbw_amd import renderer as RN
from dbw_amd.renderer import Renderer

LIGHT = {'name': 'directional', 'direction': [[1, 0.25, -1]], 'ambient_color': [[0.7, 0.7, 0.7]], 'diffuse_color': [[0.4, 0.4, 0.4]],
         'specular_color': [[0., 0., 0.]]}


def _lit_args(**over):
    """Arguments of dbw_render_lit_fwd with every pointer non-null (never dereferenced: each call below must fail validation, on the host)."""
    p = ctypes.c_void_p(256)
    a = dict(face_verts_c=p, first_idx=p, num_faces=p, neighbor=p, c2o=p, clip_code=p, clip_w=p, Fc_stride=8, face_uvs=p, face_map=p, map_desc=p,
             maps=p, faces_alpha=None, alpha_len=0, verts_world=p, faces=p, vert_normals=None, light_dir_world=p, ambient3=p, diffuse3=p, N=1,
             F_total=8, H=4, W=4, K=1, F=4, sigma=0.0, blur_radius=0.0, perspective_correct=1, background3=None, ssaa=4, image=p, workspace=p,
             workspace_bytes=1 << 30, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return list(a.values())


def test_viz_entry_points_validate_before_any_launch():
    lib = _lib.load()
    assert lib.dbw_vertex_normals(None, None, None, None, 4, 4, None, None) == -1 and b'null pointer' in lib.dbw_last_error()
    p = ctypes.c_void_p(256)
    assert lib.dbw_vertex_normals(p, p, p, p, 0, 4, p, None) == -1 and b'bad size' in lib.dbw_last_error()
    for name in ('face_verts_c', 'first_idx', 'num_faces', 'verts_world', 'faces', 'light_dir_world', 'ambient3', 'diffuse3', 'image', 'workspace'):
        assert lib.dbw_render_lit_fwd(*_lit_args(**{name: None})) == -1, name
        assert b'null pointer' in lib.dbw_last_error(), name
    for ssaa in (0, 2, 3, 8, -4):
        assert lib.dbw_render_lit_fwd(*_lit_args(ssaa=ssaa)) == -1 and b'ssaa must be 1 or 4' in lib.dbw_last_error()
        assert lib.dbw_render_lit_workspace_bytes(8, 1, 4, 4, 4, ssaa) == 0
    assert lib.dbw_render_lit_fwd(*_lit_args(ssaa=4, K=6)) == -2 and b'faces_per_pixel must be 1' in lib.dbw_last_error()      # DBW_ERR_UNSUPPORTED
    assert lib.dbw_render_lit_fwd(*_lit_args(ssaa=1, K=26)) == -2
    assert lib.dbw_render_lit_fwd(*_lit_args(H=0)) == -1 and b'bad size' in lib.dbw_last_error()
    assert lib.dbw_render_lit_fwd(*_lit_args(workspace_bytes=64)) == -1 and b'workspace too small' in lib.dbw_last_error()
    assert lib.dbw_render_lit_fwd(*_lit_args(c2o=None)) == -1 and b'all or none' in lib.dbw_last_error()
    # the workspace covers the rasteriser's at the RENDER size
    assert lib.dbw_render_lit_workspace_bytes(100, 2, 50, 40, 56, 4) > lib.dbw_rasterize_workspace_bytes_binned(100, 2, 160, 224)
    assert lib.dbw_render_lit_workspace_bytes(100, 2, 50, 40, 56, 1) > lib.dbw_rasterize_workspace_bytes_binned(100, 2, 40, 56)
    with pytest.raises(RuntimeError, match='ssaa must be 1 or 4'):
        _lib.call('dbw_render_lit_fwd', *_lit_args(ssaa=2))


def test_renderer_accepts_the_reference_light_keywords():
    kw = {'cameras': {'name': 'perspective'}, 'faces_per_pixel': 1, 'sigma': 0, 'detach_bary': False, 'z_clip': 0.001, 'lights': LIGHT,
          'shading_type': 'flat', 'background_color': (1, 1, 1)}                       # dbw.py:135-142
    r = Renderer((40, 56), **kw)
    assert r.lit and r.shading_type == 'flat' and r.background_color == (1, 1, 1) and r.faces_per_pixel == 1
    assert isinstance(r.lights, RN.DirectionalLights)
    assert r.lights.direction.tolist() == [[1, 0.25, -1]] and torch.allclose(r.lights.ambient_color, torch.full((1, 3), 0.7))
    assert torch.allclose(r.lights.diffuse_color, torch.full((1, 3), 0.4)) and not r.lights.specular_color.any()
    assert r.init_kwargs == kw
    r2 = Renderer((40, 56), **r.init_kwargs)                                          # round trip (render_views rebuilds renderers this way)
    assert r2.init_kwargs == kw and r2.shading_type == 'flat' and torch.equal(r2.lights.direction, r.lights.direction)
    # update_lights / reset_default_lights (renderer.py:118-132)
    r.update_lights(direction=[[0, 0, -1]], ka=[[0.6, 0.6, 0.6]], kd=[[0.1, 0.2, 0.3]], ks=[[0, 0, 0]])
    assert r.lights.direction.tolist() == [[0, 0, -1]] and torch.allclose(r.lights.diffuse_color, torch.tensor([[0.1, 0.2, 0.3]]))
    r.reset_default_lights()
    assert r.lights.direction.tolist() == [[1, 0.25, -1]] and torch.allclose(r.lights.ambient_color, torch.full((1, 3), 0.7))
    assert torch.allclose(r.lights.diffuse_color, torch.full((1, 3), 0.4))
    # PyTorch3D's defaults where a key is absent
    d = RN.DirectionalLights(specular_color=[[0, 0, 0]])
    assert d.direction.tolist() == [[0, 1, 0]] and torch.allclose(d.ambient_color, torch.full((1, 3), 0.5)) and torch.allclose(d.diffuse_color, torch.full((1, 3), 0.3))
    a = Renderer((8, 8), shading_type='phong')                                        # ambient light (white), Phong: lit, the gain is 1
    assert a.lit and isinstance(a.lights, RN.AmbientLights) and torch.equal(a.lights.ambient_color, torch.ones(1, 3)) and not a.lights.diffuse_color.any()
    raw = Renderer((8, 8))
    assert not raw.lit and raw.shading_type == 'raw' and isinstance(raw.lights, RN.AmbientLights)


def test_renderer_refusals_name_their_reasons():
    with pytest.raises(NotImplementedError, match='specular'):
        Renderer((8, 8), lights=dict(LIGHT, specular_color=[[0.2, 0.2, 0.2]]), shading_type='flat')
    with pytest.raises(NotImplementedError, match='default is 0.2'):                  # a directional light without an explicit specular_color
        Renderer((8, 8), lights={'name': 'directional'}, shading_type='flat')
    with pytest.raises(NotImplementedError, match='point'):
        Renderer((8, 8), lights={'name': 'point'}, shading_type='flat')
    with pytest.raises(NotImplementedError, match='per-vertex textures'):
        Renderer((8, 8), lights=LIGHT, shading_type='gouraud')
    with pytest.raises(NotImplementedError, match="'raw' ignores the light"):
        Renderer((8, 8), lights=LIGHT)
    r = Renderer((8, 8), lights=LIGHT, shading_type='phong')
    with pytest.raises(NotImplementedError, match='specular'):
        r.update_lights(ks=[[0.1, 0.1, 0.1]])
    assert not r.lights.specular_color.any()
    # a lit renderer needs the same cameras as the others
    with pytest.raises(NotImplementedError, match='perspective cameras'):
        r.render_packed(None, torch.eye(3)[None], torch.zeros(1, 3))
    # the lit pass is forward only
    v = torch.zeros(3, 3, requires_grad=True)
    cfg = ops.RenderCfg(8, 8, 1, 0.0, 0.001, True, False, 1)
    with pytest.raises(NotImplementedError, match='forward only'):
        ops.render_scene_lit(v, torch.zeros(3), None, torch.zeros(1, 3, dtype=torch.int32), torch.eye(3)[None], torch.zeros(1, 3), torch.eye(4),
                             None, None, None, None, cfg, torch.tensor([[0., 0, -1]]), [1, 1, 1], [0, 0, 0])
    with pytest.raises(NotImplementedError, match='faces_per_pixel must be 1'):
        ops.render_scene_lit(v.detach(), torch.zeros(3), None, torch.zeros(1, 3, dtype=torch.int32), torch.eye(3)[None], torch.zeros(1, 3), torch.eye(4),
                             None, None, None, None, ops.RenderCfg(8, 8, 6, 1e-4, 0.001, True, False, 1), torch.tensor([[0., 0, -1]]), [1, 1, 1],
                             [0, 0, 0], ssaa=4)
    # the trajectory helpers refuse to invent cameras
    with pytest.raises(NotImplementedError, match='perspective cameras'):
        RN.render_views(None, torch.eye(3)[None], torch.zeros(1, 3), renderer=None)
    with pytest.raises(NotImplementedError, match='perspective cameras'):
        RN.render_rotated_views(None, renderer=None)


def test_model_builds_renderer_light_like_the_reference():
    cfg = {'model': {'name': 'dbw', 'mesh': {'n_blocks': 3, 'txt_size': 8},
                     'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001}}}
    m = dbw_amd.create_model(cfg, (16, 24))
    rl = m.renderer_light
    kw = rl.init_kwargs
    assert kw['lights'] == LIGHT and kw['shading_type'] == 'flat' and tuple(kw['background_color']) == (1, 1, 1)      # dbw.py:139-142
    assert kw['faces_per_pixel'] == 1 and kw['sigma'] == 0 and kw['detach_bary'] is False and rl.img_size == (16, 24)
    assert not m.renderer.lit and not m.renderer_fine.lit and not m.renderer_env.lit and rl.lit
    Km = O.synthetic_cameras(1)[2]
    m._ensure_cameras(dict(imgs=torch.zeros(1, 3, 16, 24), K=Km))
    assert torch.equal(rl.cameras.K, m.renderer.cameras.K) and rl.cameras.K is not None
    assert list(m.state_dict()) == list(dbw_amd.create_model(cfg, (16, 24)).state_dict())
    assert not any('renderer_light' in k for k in m.state_dict())


def test_look_at_view_transform_and_circle_trajectory():
    g = torch.Generator().manual_seed(0)
    dist, elev, azim = torch.rand(40, generator=g) * 3 + 0.5, torch.rand(40, generator=g) * 160 - 80, torch.rand(40, generator=g) * 720 - 360
    R, T = RN.look_at_view_transform(dist, elev, azim)
    e, a = torch.deg2rad(elev), torch.deg2rad(azim)
    C = torch.stack([dist * torch.cos(e) * torch.sin(a), dist * torch.sin(e), dist * torch.cos(e) * torch.cos(a)], -1)
    Ro, To = O.look_at_cameras(C)
    assert torch.allclose(R, Ro, atol=1e-6) and torch.allclose(T, To, atol=1e-6)
    assert torch.allclose(-(T[:, None] @ R.transpose(1, 2))[:, 0], C, atol=1e-5)       # camera centre = -T R^T
    R1, T1 = RN.look_at_view_transform(2.0, 30.0, torch.tensor([0., 90.]))                # scalars broadcast
    assert R1.shape == (2, 3, 3) and T1.shape == (2, 3) and torch.allclose(T1, torch.tensor([[0., 0., 2.]]).expand(2, 3), atol=1e-6)
    for n in (50, 7):
        R, T = RN.get_circle_traj(dist=2.5, a_scale=15, e_scale=15, N_views=n)
        assert R.shape == (n, 3, 3) and T.shape == (n, 3)
        assert torch.allclose(torch.det(R), torch.ones(n), atol=1e-5) and torch.allclose(R @ R.transpose(1, 2), torch.eye(3).expand(n, 3, 3), atol=1e-5)
        assert torch.allclose(T.norm(dim=-1), torch.full((n,), 2.5), atol=1e-5)
    azim = torch.cos(torch.linspace(0, 2, 8)[:-1] * torch.pi) * 15 - 180                  # renderer.py:411-414
    elev = torch.sin(torch.linspace(0, 2, 8)[:-1] * torch.pi) * 15
    Rr, Tr = RN.look_at_view_transform(2.5, elev, azim)
    assert torch.allclose(R, Rr, atol=1e-6) and torch.allclose(T, Tr, atol=1e-6)
