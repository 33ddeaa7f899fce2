"""Renderer -- same constructor keywords, attributes and `forward` contract as the reference's
src/model/renderer.py:24-60,84-98 (`Renderer(img_size, **cfg.model.renderer)`; `forward(meshes, R, T,
viz_purpose=False, faces_alpha=...) -> (B,4,H,W)` BCHW, premultiplied RGB + alpha), with everything below it
(PyTorch3D MeshRenderer / MeshRasterizer / TexturesUV sampling / LayeredShader + layered_rgb_blend) replaced by the
HIP path in libdbw_hip.so.  Only the configuration the hot path uses is implemented:
perspective cameras with an explicit NDC K matrix, ambient white light, the 'raw' layered shader (clip_inside True or False) -- and,
for the pictures a user looks at (the reference's `renderer_light`, dbw.py:139-143, and the eye_light variants of render_views /
render_rotated_views), a directional light with 'flat' or 'phong' shading through the forward-only lit kernel (include/dbw_viz.h).
Anything else raises NotImplementedError instead of silently rendering something different."""
import math
from copy import deepcopy

import torch
from torch import nn
from torch.nn import functional as F

from . import ops
from .structures import Meshes, PackedScene

EPS = 1e-8          # renderer.py:20
DIRECTION_LIGHT = [1, 0.25, -1]          # renderer.py:21


class PerspectiveCameras:
    """Holder of the shared intrinsics.  K is None until update_cameras(K=...) (dbw.py:204-208)."""

    def __init__(self, K=None, device=None, **kwargs):
        self.K = None if K is None else torch.as_tensor(K, dtype=torch.float32).reshape(-1, 4, 4)[:1]
        if device is not None and self.K is not None:
            self.K = self.K.to(device)
        self.kwargs = kwargs

    def to(self, device):
        if self.K is not None:
            self.K = self.K.to(device)
        return self


def _color3(v, name):
    """One RGB triple as a (1,3) fp32 CPU tensor (the reference writes its lights as [[r, g, b]])."""
    t = torch.as_tensor(v, dtype=torch.float32).reshape(-1, 3)
    if t.shape[0] != 1:
        raise NotImplementedError(f'{name}: one value shared by the views, got {tuple(t.shape)}')
    return t.clone()


class AmbientLights:
    """PyTorch3D's AmbientLights: ambient_color (default white), no diffuse, no specular term."""

    def __init__(self, ambient_color=((1.0, 1.0, 1.0),)):
        self.ambient_color = _color3(ambient_color, 'ambient_color')
        self.diffuse_color = torch.zeros(1, 3)
        self.specular_color = torch.zeros(1, 3)
        self.direction = torch.tensor([[0., 1., 0.]])

    def to(self, device):
        return self


SPECULAR_REASON = ('a non-zero specular_color is not rendered: PyTorch3D takes the camera centre of the specular term from a cameras object '
                   'that does not carry the view\'s R, T, which cannot be verified without the library; every light the reference builds has '
                   'specular_color 0 (note that PyTorch3D\'s own default is 0.2: pass specular_color=[[0, 0, 0]] explicitly)')


class DirectionalLights:
    """PyTorch3D's DirectionalLights (defaults: direction (0, 1, 0), ambient 0.5, diffuse 0.3, specular 0.2), host-side values: the
    direction points FROM the surface TO the light, in camera space (Renderer fixes the light to the camera, renderer.py:87-89).  The
    `_direction` ... copies are the constructor's values (renderer.py:74-78: reset_default_lights)."""

    def __init__(self, direction=((0, 1, 0),), ambient_color=((0.5, 0.5, 0.5),), diffuse_color=((0.3, 0.3, 0.3),),
                 specular_color=((0.2, 0.2, 0.2),)):
        self.direction = torch.as_tensor(direction, dtype=torch.float32).reshape(-1, 3).clone()
        self.ambient_color = _color3(ambient_color, 'ambient_color')
        self.diffuse_color = _color3(diffuse_color, 'diffuse_color')
        self.specular_color = _color3(specular_color, 'specular_color')
        if bool((self.specular_color != 0).any()):
            raise NotImplementedError(SPECULAR_REASON)
        self._direction, self._ambient_color = self.direction, self.ambient_color
        self._diffuse_color, self._specular_color = self.diffuse_color, self.specular_color

    def to(self, device):
        return self


class Renderer(nn.Module):
    def __init__(self, img_size, **kwargs):
        super().__init__()
        self.img_size = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)
        self._init_kwargs = deepcopy(kwargs)
        self.init_cameras(**kwargs.pop('cameras', {}))
        self.init_lights(**kwargs.pop('lights', {}))
        self.sigma = kwargs.pop('sigma', 1e-4)
        self.background_color = tuple(kwargs.pop('background_color', (0, 0, 0)))
        self.faces_per_pixel = kwargs.pop('faces_per_pixel', 25)
        p_correct = kwargs.pop('perspective_correct', None)
        self.z_clip = kwargs.pop('z_clip', None)
        kwargs.pop('debug', False)
        if not kwargs.pop('layered_shader', True):
            raise NotImplementedError('only the layered shader is on the hot path (renderer.py:39-43)')
        self.clip_inside = bool(kwargs.pop('clip_inside', True))          # False: sigmoid(-d / sigma) instead of exp(-max(d, 0) / sigma), renderer.py:257-258
        self.shading_type = kwargs.pop('shading_type', 'raw')
        if self.shading_type == 'gouraud':
            raise NotImplementedError("shading_type='gouraud' needs per-vertex textures, which the UV-textured scenes of this path do not have")
        if self.shading_type not in ('raw', 'flat', 'phong'):
            raise NotImplementedError(f"shading_type='{self.shading_type}': one of 'raw', 'flat', 'phong'")
        if self.shading_type == 'raw' and isinstance(self.lights, DirectionalLights):
            raise NotImplementedError("shading_type='raw' ignores the light: a directional light needs 'flat' or 'phong' (nothing in the "
                                      'reference combines the two)')
        self.detach_bary = kwargs.pop('detach_bary', False)
        assert len(kwargs) == 0, kwargs
        # perspective_correct=None is inferred True for perspective cameras
        self.perspective_correct = True if p_correct is None else bool(p_correct)
        self._bg = ops.make_bg(self.background_color)

    # -- renderer.py:62-73
    def init_cameras(self, **kwargs):
        kwargs = deepcopy(kwargs)
        self.cam_name = kwargs.pop('name', 'fov')
        self.cam_kwargs = kwargs
        self.cameras = PerspectiveCameras(**kwargs)

    def init_lights(self, **kwargs):
        kwargs = deepcopy(kwargs)
        name = kwargs.pop('name', 'ambient')
        if name == 'point':
            raise NotImplementedError("lights 'point' are not implemented (nothing in the reference builds one): 'ambient' or 'directional'")
        if name not in ('ambient', 'directional'):
            raise KeyError(name)
        self.lights = {'ambient': AmbientLights, 'directional': DirectionalLights}[name](**kwargs)

    # -- renderer.py:118-132
    def update_lights(self, direction=None, ka=None, kd=None, ks=None):
        if direction is not None:
            self.lights.direction = torch.as_tensor(direction, dtype=torch.float32).reshape(-1, 3).clone()
        if ka is not None:
            self.lights.ambient_color = _color3(ka, 'ka')
        if kd is not None:
            self.lights.diffuse_color = _color3(kd, 'kd')
        if ks is not None:
            ks = _color3(ks, 'ks')
            if bool((ks != 0).any()):
                raise NotImplementedError(SPECULAR_REASON)
            self.lights.specular_color = ks

    def reset_default_lights(self):
        self.lights.direction = self.lights._direction
        self.lights.ambient_color = self.lights._ambient_color
        self.lights.diffuse_color = self.lights._diffuse_color
        self.lights.specular_color = self.lights._specular_color

    @property
    def lit(self):
        """True: render_packed / forward go through the forward-only lit kernel (flat / Phong shading)."""
        return self.shading_type != 'raw'

    @property
    def init_kwargs(self):
        return deepcopy(self._init_kwargs)

    def to(self, device):
        super().to(device)
        self.cameras.to(device)
        return self

    # -- renderer.py:106-116
    def get_copy_cameras(self, **kwargs):
        merged = deepcopy(self.cam_kwargs)
        merged.update(kwargs)
        return PerspectiveCameras(**merged)

    def update_cameras(self, **kwargs):
        self.cameras = self.get_copy_cameras(**kwargs)

    def _cfg(self, n_faces, viz=False, lds_aggregate=False, texbins=None, const_faces=0):
        H, W = self.img_size
        if viz:   # exact anti-aliased rendering for visualisation (renderer.py:56-60): 4x res, sigma 0, 1 face per pixel
            return ops.RenderCfg(H * 4, W * 4, 1, 0.0, self.z_clip, self.perspective_correct, False, n_faces, EPS)
        cfg = ops.RenderCfg(H, W, self.faces_per_pixel, self.sigma, self.z_clip, self.perspective_correct, self.detach_bary,
                            n_faces, EPS, lds_aggregate, texbins, const_faces, clip_inside=self.clip_inside)
        if texbins is not None:         # the texture bins' record sub-ranges follow the demand of this renderer's previous backward (ops.BinDemand)
            if getattr(self, '_bin_demand', None) is None:
                self._bin_demand = ops.BinDemand()
            cfg.bin_demand = self._bin_demand
        return cfg

    def render_packed(self, scene, R, T, faces_alpha=None, viz_purpose=False, lds_aggregate=False, Kmat=None):
        """scene: PackedScene shared by the len(R) views.  lds_aggregate: hint for the backward pass (pays when neighbouring
        pixels hit the same texels: magnified or decimated maps); results are identical either way.  Kmat: a live (4,4) matrix in place of
        cameras.K[0] (intrinsics refinement, DESIGN.md 6t: it may require a gradient)."""
        if self.cam_name != 'perspective' or self.cameras.K is None:
            raise NotImplementedError('the HIP path needs perspective cameras with an explicit NDC K: call '
                                      'update_cameras(K=...) first (dbw.py:204-208)')
        Kmat = (self.cameras.K[0] if Kmat is None else Kmat.reshape(4, 4).float()).to(R.device).contiguous()
        R, T = R.float().contiguous(), T.float().contiguous()
        if self.lit:
            return self._render_lit(scene, R, T, Kmat, faces_alpha, viz_purpose)
        cfg = self._cfg(scene.faces.shape[0], viz_purpose, lds_aggregate, getattr(scene, 'texbins', None), getattr(scene, 'const_faces', 0))
        if viz_purpose:
            with torch.no_grad():
                img = ops.render_scene(scene.verts, scene.maps, None, scene.faces, R, T, Kmat, scene.face_uvs, scene.face_map,
                                       scene.map_desc, self._bg, cfg)
                return F.avg_pool2d(img, kernel_size=4, stride=4)
        return ops.render_scene(scene.verts, scene.maps, faces_alpha, scene.faces, R, T, Kmat, scene.face_uvs, scene.face_map,
                                scene.map_desc, self._bg, cfg)

    @torch.no_grad()
    def parse_packed(self, scene, face_label, R, T):
        """Scene parsing maps of `scene` for the len(R) views at this renderer's image size, cameras and z_clip: -> (label, depth, cover,
        counts) of ops.parse_scene.  face_label: one label in [0, 64) per face of the scene.  Hard rasterisation whatever the renderer's
        sigma and faces_per_pixel are; lights and shading play no part."""
        if self.cam_name != 'perspective' or self.cameras.K is None:
            raise NotImplementedError('the HIP path needs perspective cameras with an explicit NDC K: call '
                                      'update_cameras(K=...) first (dbw.py:204-208)')
        Kmat = self.cameras.K[0].to(R.device).contiguous()
        H, W = self.img_size
        cfg = ops.RenderCfg(H, W, 1, 0.0, self.z_clip, self.perspective_correct, False, scene.faces.shape[0], EPS)
        return ops.parse_scene(scene.verts, scene.faces, face_label, R.float().contiguous(), T.float().contiguous(), Kmat, cfg)

    def _render_lit(self, scene, R, T, Kmat, faces_alpha, viz_purpose):
        """Flat / Phong shading under this renderer's light, which follows the camera (renderer.py:87-89; `self.lights` itself is not
        touched).  viz_purpose: hard, one face per pixel, 4x4 super-samples resolved inside the kernel; else this renderer's own
        faces_per_pixel and sigma at the image size.  Forward only."""
        H, W = self.img_size
        n_faces = scene.faces.shape[0]
        if viz_purpose:
            cfg, ssaa, faces_alpha = ops.RenderCfg(H, W, 1, 0.0, self.z_clip, self.perspective_correct, False, n_faces, EPS), 4, None
        else:
            cfg, ssaa = ops.RenderCfg(H, W, self.faces_per_pixel, self.sigma, self.z_clip, self.perspective_correct, self.detach_bary, n_faces,
                                      EPS, clip_inside=self.clip_inside), 1
        li = self.lights
        if li.direction.shape[0] not in (1, R.shape[0]):
            raise ValueError(f'{li.direction.shape[0]} light directions for {R.shape[0]} views')
        adjacency = None
        if self.shading_type == 'phong':          # the vertex -> (face, corner) table: once per topology
            adjacency = getattr(scene, '_lit_adjacency', None)
            if adjacency is None:
                adjacency = ops.vertex_adjacency(scene.faces, scene.verts.shape[0])
                try:
                    scene._lit_adjacency = adjacency
                except AttributeError:
                    pass
        return ops.render_scene_lit(scene.verts, scene.maps, faces_alpha, scene.faces, R, T, Kmat, scene.face_uvs, scene.face_map,
                                    scene.map_desc, self._bg, cfg, li.direction, li.ambient_color.reshape(3).tolist(),
                                    li.diffuse_color.reshape(3).tolist(), phong=self.shading_type == 'phong', ssaa=ssaa, adjacency=adjacency)

    # -- renderer.py:134-175: wireframe overlays (visualisation) on the same rasteriser kernels
    def _as_scene(self, meshes):
        return PackedScene.from_meshes(meshes) if isinstance(meshes, Meshes) else meshes

    @torch.no_grad()
    def render_edges(self, meshes, R, T, image_size=None, linewidth=1, return_pix2face=False, faces_per_pixel=1):
        """(B,1,H,W) mask of the pixels that lie inside a face and closer than `linewidth` pixels to one of its edges
        (renderer.py:134-147): a hard rasterisation whose signed squared NDC distances are thresholded at
        (linewidth * 2 / min(image_size))^2; with return_pix2face also the (B,H,W) int64 packed face id of the nearest face."""
        if self.cam_name != 'perspective' or self.cameras.K is None:
            raise NotImplementedError('the HIP path needs perspective cameras with an explicit NDC K (dbw.py:204-208)')
        scene = self._as_scene(meshes)
        H, W = image_size or self.img_size
        cfg = ops.RenderCfg(H, W, int(faces_per_pixel), 0.0, self.z_clip, self.perspective_correct, False, scene.faces.shape[0], EPS)
        Kmat = self.cameras.K[0].to(R.device).contiguous()
        cl, p2f, _, _, dists = ops.render_fragments(scene.verts.detach(), scene.faces, R.float().contiguous(), T.float().contiguous(), Kmat, cfg)
        mask = (-dists < (linewidth * 2 / min(H, W)) ** 2).float()[:, None]       # B1HWK; empty slots hold -1: never an edge
        mask = mask.max(-1)[0]
        if not return_pix2face:
            return mask
        first = p2f[..., 0]
        B, F_ = R.shape[0], scene.faces.shape[0]
        orig = cl['c2o'].view(-1).long()[first.clamp(min=0).long()] + torch.arange(B, device=first.device).view(B, 1, 1) * F_
        return mask, torch.where(first >= 0, orig, torch.full_like(orig, -1))

    @torch.no_grad()
    def draw_edges(self, img, meshes, R=None, T=None, colors=None, linewidth=1, antialias=True):
        """img (B,3,H,W) with the wireframe of `meshes` painted on it (renderer.py:149-175); colors: one RGB triple, or one per
        packed face (B*F,3).  antialias: the mask is rasterised at 4x the resolution and average-pooled."""
        scene = self._as_scene(meshes)
        B = img.shape[0]
        dev = img.device
        if R is None:
            R = torch.eye(3, device=dev)[None].expand(B, -1, -1)
        if T is None:
            T = torch.zeros(1, 3, device=dev).expand(B, -1)
        colors = torch.as_tensor((1., 0., 0.) if colors is None else colors, dtype=torch.float32, device=dev)
        size = tuple(img.shape[-2:])
        mask, face_img = self.edge_layers(scene, R, T, size, colors, linewidth, antialias)
        if face_img is None:
            face_img = colors[None, :, None, None].expand(B, -1, *((size[0] * 4, size[1] * 4) if antialias else size))
            if antialias:
                face_img = F.avg_pool2d(face_img, kernel_size=4, stride=4)
        return img * (1 - mask) + mask * face_img

    @torch.no_grad()
    def edge_layers(self, scene, R, T, size, colors, linewidth=1, antialias=True):
        """The two layers draw_edges blends over an image of `size`: the mask (B,1,H,W) and, for one colour per packed face (colors
        (B*F,3)), the colour image (B,3,H,W) -- None for a single colour.  antialias: both are rasterised at 4x and average-pooled."""
        if antialias:
            size, linewidth = (size[0] * 4, size[1] * 4), linewidth * 4
        mask, pix2face = self.render_edges(scene, R, T, image_size=size, linewidth=linewidth, return_pix2face=True)
        face_img = colors[pix2face].permute(0, 3, 1, 2) if colors.dim() == 2 else None      # (empty pixels: last row, masked)
        if antialias:
            mask = F.avg_pool2d(mask, kernel_size=4, stride=4)
            face_img = None if face_img is None else F.avg_pool2d(face_img, kernel_size=4, stride=4)
        return mask, face_img

    def render_viz(self, scene, R, T):
        """(B,4,H,W): the exact 4x anti-aliased hard render of render_packed(viz_purpose=True), through the lit kernel for every renderer
        -- it resolves its 4x4 super-samples in registers, no 4H x 4W image exists.  An unlit ('raw') renderer is an ambient gain of 1
        and no diffuse term there (tests/test_gpu_lit.py bounds the difference to the pooled raw render: RESOLVE_ATOL)."""
        if self.lit:
            return self.render_packed(scene, R, T, viz_purpose=True)
        if self.cam_name != 'perspective' or self.cameras.K is None:
            raise NotImplementedError('the HIP path needs perspective cameras with an explicit NDC K: call '
                                      'update_cameras(K=...) first (dbw.py:204-208)')
        H, W = self.img_size
        cfg = ops.RenderCfg(H, W, 1, 0.0, self.z_clip, self.perspective_correct, False, scene.faces.shape[0], EPS)
        Kmat = self.cameras.K[0].to(R.device).contiguous()
        return ops.render_scene_lit(scene.verts, scene.maps, None, scene.faces, R.float().contiguous(), T.float().contiguous(), Kmat, scene.face_uvs,
                                    scene.face_map, scene.map_desc, self._bg, cfg, torch.tensor([[0., 0., -1.]]), [1., 1., 1.], [0., 0., 0.],
                                    phong=False, ssaa=4)

    def forward(self, meshes, R, T, viz_purpose=False, **kwargs):
        faces_alpha = kwargs.pop('faces_alpha', None)
        assert len(kwargs) == 0, kwargs
        if isinstance(meshes, Meshes):
            if len(meshes) != len(R) and len(meshes) != 1:
                raise ValueError(f'{len(meshes)} meshes for {len(R)} cameras')
            scene = PackedScene.from_meshes(meshes)
        else:
            scene = meshes
        return self.render_packed(scene, R, T, faces_alpha, viz_purpose)


# -- renderer.py:290-380,411-414: view trajectories (tensors in, tensors out; writing videos / GIFs is left to the caller) --------------------
def look_at_view_transform(dist=1.0, elev=0.0, azim=0.0, device='cpu'):
    """PyTorch3D's look_at_view_transform for cameras that look at the origin with +Y up: dist, elev, azim (degrees; scalars or (N,)
    tensors, broadcast) -> R (N,3,3), T (N,3).  Camera centre C = dist * (cos e sin a, sin e, cos e cos a); R's columns are the camera
    axes (z = towards the origin, x = up x z, y = z x x, each normalised), T = -C @ R."""
    dist, elev, azim = torch.broadcast_tensors(*[torch.as_tensor(v, dtype=torch.float32, device=device).reshape(-1) for v in (dist, elev, azim)])
    e, a = elev * (math.pi / 180.0), azim * (math.pi / 180.0)
    C = torch.stack([dist * torch.cos(e) * torch.sin(a), dist * torch.sin(e), dist * torch.cos(e) * torch.cos(a)], dim=-1)
    up = torch.tensor([0., 1., 0.], device=C.device).expand_as(C)
    z = F.normalize(-C, dim=-1, eps=1e-5)
    x = F.normalize(torch.cross(up, z, dim=-1), dim=-1, eps=1e-5)
    y = F.normalize(torch.cross(z, x, dim=-1), dim=-1, eps=1e-5)
    degenerate = (x.abs() < 5e-3).all(dim=-1, keepdim=True)          # looking along the up axis: x from y and z instead
    x = torch.where(degenerate, F.normalize(torch.cross(y, z, dim=-1), dim=-1, eps=1e-5), x)
    R = torch.stack([x, y, z], dim=-1)
    T = -(C[:, None] @ R)[:, 0]
    return R, T


def get_circle_traj(dist=1, a_scale=15, e_scale=15, N_views=50):
    azim = torch.cos(torch.linspace(0, 2, N_views + 1) * math.pi)[:-1] * a_scale - 180
    elev = torch.sin(torch.linspace(0, 2, N_views + 1) * math.pi)[:-1] * e_scale
    return look_at_view_transform(dist, azim=azim, elev=elev)


def _eye_light_renderer(renderer, direction, ambient):
    """eye_light of render_views / render_rotated_views (renderer.py:301-310,343-351): an ambient renderer is swapped for a Phong one,
    one face per pixel, under a directional light; a renderer that has a directional light already is kept."""
    if not isinstance(renderer.lights, AmbientLights):
        return renderer
    kwargs = renderer.init_kwargs
    kwargs['lights'] = {'name': 'directional', 'direction': [direction], 'ambient_color': [[ambient] * 3], 'diffuse_color': [[0.4, 0.4, 0.4]],
                        'specular_color': [[0., 0., 0.]]}
    kwargs['shading_type'] = 'phong'
    kwargs['faces_per_pixel'] = 1
    out = Renderer(renderer.img_size, **kwargs)
    out.cameras = renderer.cameras
    return out


def _need_renderer(renderer):
    if renderer is None:
        raise NotImplementedError('renderer=None (the reference then builds FoV cameras): the HIP path needs perspective cameras with an '
                                  'explicit NDC K, pass a Renderer whose update_cameras(K=...) was called')


def _composite_bkg(views, bkg, img_size):
    rec, alpha = torch.cat(views, dim=0).split([3, 1], dim=1)
    if bkg is not None:
        bkg = bkg.cpu()
        if tuple(bkg.shape[-2:]) != tuple(img_size):
            bkg = F.interpolate(bkg[None], size=tuple(img_size), mode='bilinear', align_corners=False)[0]
        rec = rec * alpha + (1 - alpha) * bkg
    return rec


@torch.no_grad()
def render_views(mesh, R, T, renderer=None, bkg=None, with_edges=False, linewidth=1, edge_colors=None, eye_light=False, with_alpha=False):
    """The views (R[i], T[i]) of `mesh` (Meshes or PackedScene), exact 4x anti-aliased renders in batches of 10 (renderer.py:333-380) ->
    (N,3,H,W) on the CPU, composited over `bkg` (3,H,W) where given, or (N,4,H,W) with_alpha.  with_edges: the wireframe painted on every
    view (edge_colors: one RGB triple or one row per face of the scene)."""
    _need_renderer(renderer)
    if eye_light:
        renderer = _eye_light_renderer(renderer, DIRECTION_LIGHT, 0.7)
    scene = renderer._as_scene(mesh)
    n_views = len(R)
    views, B = [], 10
    for k in range((n_views - 1) // B + 1):
        R_view, T_view = R[k * B: (k + 1) * B], T[k * B: (k + 1) * B]
        B_eff = len(R_view)
        res = renderer(scene, R_view, T_view, viz_purpose=True)
        if with_edges:
            res, alpha = res.split([3, 1], dim=1)
            colors = edge_colors
            if isinstance(colors, torch.Tensor) and colors.dim() == 2:
                colors = colors.to(res.device).repeat(B_eff, 1)
            res = renderer.draw_edges(res, scene, R=R_view, T=T_view, linewidth=linewidth, colors=colors)
            res = torch.cat([res, alpha], dim=1)
        views.append(res.cpu())
    if with_alpha:
        return torch.cat(views, dim=0)
    return _composite_bkg(views, bkg, renderer.img_size)


@torch.no_grad()
def render_rotated_views(mesh, renderer=None, n_views=50, elev=30, dist=2.5, R=None, T=None, bkg=None, eye_light=False):
    """`mesh` seen from n_views azimuths around it (renderer.py:290-330): look_at cameras at unit distance composed with (R, T) where
    given (elev / dist then count for nothing), else elevated by `elev` and pushed back by `dist` -> (n_views,3,H,W) on the CPU, clamped
    to [0, 1]."""
    _need_renderer(renderer)
    if eye_light:
        if R is not None:
            raise NotImplementedError
        renderer = _eye_light_renderer(renderer, [0, 0, -1], 0.6)
    scene = renderer._as_scene(mesh)
    dev = scene.verts.device
    elev, dist = 0 if R is not None else elev, 0 if T is not None else dist
    R = torch.eye(3, device=dev) if R is None else R.to(dev)
    T = torch.zeros(3, device=dev) if T is None else T.to(dev)
    azim = torch.linspace(-180, 180, n_views)
    views, B = [], 10
    for k in range((n_views - 1) // B + 1):
        R_view = look_at_view_transform(dist=1, elev=elev, azim=azim[k * B: (k + 1) * B], device=dev)[0]
        T_view = torch.tensor([[0., 0., float(dist)]], device=dev).expand(len(R_view), -1)
        views.append(renderer(scene, (R_view @ R).contiguous(), (T_view + T).contiguous(), viz_purpose=True).clamp(0, 1).cpu())
    return _composite_bkg(views, bkg, renderer.img_size)


# -- the same trajectories as 8-bit frames: what an image or a video file holds (include/dbw_export.h) ----------------------------------------
FRAME_WORKSPACE_BYTES = 256 << 20          # device memory one chunk of views may take (render workspace + fp32 image + edge layers)


def _views_per_chunk(scene, img_size, n_views, with_edges=False):
    """Views rendered per launch: as many as fit FRAME_WORKSPACE_BYTES, from the lit kernel's own workspace size (the clipper emits at
    most two faces per face) and the planes a view keeps on the device."""
    H, W = img_size
    F_ = int(scene.faces.shape[0])
    per_view = int(ops._viz_lib().dbw_render_lit_workspace_bytes(2 * F_, 1, F_, H, W, 4)) + H * W * (16 + 2 * 3)
    if with_edges:           # the 4x edge rasterisation: fragments and the two pooled layers
        per_view += 16 * H * W * 4 * 8 + H * W * 16
    return max(1, min(n_views, FRAME_WORKSPACE_BYTES // max(per_view, 1)))


def _host_frames(n, H, W, out):
    if out is None:
        return torch.empty(n, H, W, 3, dtype=torch.uint8, pin_memory=True)
    if out.is_cuda or out.dtype != torch.uint8 or not out.is_contiguous() or tuple(out.shape) != (n, H, W, 3):
        raise ValueError(f'out: a contiguous ({n},{H},{W},3) uint8 host tensor (pinned, for the copy to overlap the next render)')
    return out


def _stream_frames(chunks, n, H, W, device, out=None):
    """chunks yields (count, fill): fill(dst) enqueues the render and the conversion of `count` frames into the (count,H,W,3) uint8 device
    tensor dst on the current stream.  Each chunk is copied to the host on a second stream, ordered by events: chunk k copies while
    chunk k + 1 renders; two device buffers alternate.  -> the (n,H,W,3) uint8 host tensor, complete on return."""
    out = _host_frames(n, H, W, out)
    cur, copy = torch.cuda.current_stream(device), torch.cuda.Stream(device)
    bufs, copied, pos = [None, None], [None, None], 0
    for k, (count, fill) in enumerate(chunks):
        slot = k & 1
        if bufs[slot] is None or bufs[slot].shape[0] < count:
            bufs[slot] = torch.empty(count, H, W, 3, dtype=torch.uint8, device=device)
        if copied[slot] is not None:
            cur.wait_event(copied[slot])               # the copy of chunk k - 2 has left this buffer
        fill(bufs[slot][:count])
        done = torch.cuda.Event()
        done.record(cur)
        with torch.cuda.stream(copy):
            copy.wait_event(done)
            out[pos:pos + count].copy_(bufs[slot][:count], non_blocking=True)
            copied[slot] = torch.cuda.Event()
            copied[slot].record(copy)
        pos += count
    copy.synchronize()
    assert pos == n
    return out


def _bkg_on_device(bkg, img_size, device):
    """The background of _composite_bkg (resized on the host exactly as there), on the device."""
    if bkg is None:
        return None
    bkg = bkg.cpu().float()
    if tuple(bkg.shape[-2:]) != tuple(img_size):
        bkg = F.interpolate(bkg[None], size=tuple(img_size), mode='bilinear', align_corners=False)[0]
    return bkg.contiguous().to(device)


def _pooled_color(colors):
    """One colour after draw_edges' 4x4 average pooling of its constant image (sixteen equal addends need not sum to 16 c in fp32)."""
    return F.avg_pool2d(colors.reshape(1, 3, 1, 1).expand(1, 3, 4, 4), kernel_size=4, stride=4).reshape(3).tolist()


@torch.no_grad()
def render_views_u8(mesh, R, T, renderer=None, bkg=None, with_edges=False, linewidth=1, edge_colors=None, eye_light=False, out=None, chunk=None):
    """render_views as 8-bit frames: the views (R[i], T[i]) of `mesh`, exact 4x anti-aliased renders -> (N,H,W,3) uint8 on the HOST (pinned;
    or `out`, filled in place), quantised as the reference's convert_to_img does (clamp to [0, 1], times 255, truncate).  Same arguments
    as render_views; composite, edge blend, quantisation and interleave run on the device (dbw_frames_u8), so 3 bytes per pixel cross to the
    host instead of 16, and the copy of a chunk overlaps the render of the next.  Every renderer goes through the lit kernel
    (Renderer.render_viz).  chunk: views per launch (default: what fits FRAME_WORKSPACE_BYTES); the frames do not depend on it."""
    _need_renderer(renderer)
    if eye_light:
        renderer = _eye_light_renderer(renderer, DIRECTION_LIGHT, 0.7)
    scene = renderer._as_scene(mesh)
    dev = scene.verts.device
    H, W = renderer.img_size
    n_views = len(R)
    B = int(chunk) if chunk else _views_per_chunk(scene, (H, W), n_views, with_edges)
    bkg_dev = _bkg_on_device(bkg, (H, W), dev)
    colors = color3 = None
    if with_edges:
        colors = torch.as_tensor((1., 0., 0.) if edge_colors is None else edge_colors, dtype=torch.float32, device=dev)
        if colors.dim() != 2:
            color3 = _pooled_color(colors)

    def chunks():
        for k in range((n_views - 1) // B + 1):
            R_view, T_view = R[k * B: (k + 1) * B], T[k * B: (k + 1) * B]

            def fill(dst, R_view=R_view, T_view=T_view):
                res = renderer.render_viz(scene, R_view, T_view)
                mask = col = None
                if with_edges:
                    per_face = colors.repeat(len(R_view), 1) if color3 is None else colors
                    mask, col = renderer.edge_layers(scene, R_view, T_view, (H, W), per_face, linewidth=linewidth)
                    col = color3 if col is None else col
                ops.frames_u8(res, bkg=bkg_dev, mask=mask, edge_color=col, edge_first=True, out=dst)
            yield len(R_view), fill
    return _stream_frames(chunks(), n_views, H, W, dev, out)


@torch.no_grad()
def render_rotated_views_u8(mesh, renderer=None, n_views=50, elev=30, dist=2.5, R=None, T=None, bkg=None, eye_light=False, out=None, chunk=None):
    """render_rotated_views as 8-bit frames (see render_views_u8): `mesh` from n_views azimuths -> (n_views,H,W,3) uint8 on the host."""
    _need_renderer(renderer)
    if eye_light:
        if R is not None:
            raise NotImplementedError
        renderer = _eye_light_renderer(renderer, [0, 0, -1], 0.6)
    scene = renderer._as_scene(mesh)
    dev = scene.verts.device
    H, W = renderer.img_size
    elev, dist = 0 if R is not None else elev, 0 if T is not None else dist
    R = torch.eye(3, device=dev) if R is None else R.to(dev)
    T = torch.zeros(3, device=dev) if T is None else T.to(dev)
    azim = torch.linspace(-180, 180, n_views)
    B = int(chunk) if chunk else _views_per_chunk(scene, (H, W), n_views)
    bkg_dev = _bkg_on_device(bkg, (H, W), dev)

    def chunks():
        for k in range((n_views - 1) // B + 1):
            az = azim[k * B: (k + 1) * B]

            def fill(dst, az=az):
                R_view = look_at_view_transform(dist=1, elev=elev, azim=az, device=dev)[0]
                T_view = torch.tensor([[0., 0., float(dist)]], device=dev).expand(len(R_view), -1)
                res = renderer.render_viz(scene, (R_view @ R).contiguous(), (T_view + T).contiguous())
                ops.frames_u8(res, bkg=bkg_dev, clamp_input=bkg_dev is not None, out=dst)      # (render_rotated_views clamps before it composites)
            yield len(az), fill
    return _stream_frames(chunks(), n_views, H, W, dev, out)
