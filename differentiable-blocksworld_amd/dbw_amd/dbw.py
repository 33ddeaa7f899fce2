"""DifferentiableBlocksWorld -- host-side mirror of the reference model (src/model/dbw.py:38-462): same constructor
keywords (cfg.model.{mesh,renderer,rend_optim,loss}), same 10 parameters and buffer names/shapes (checkpoints
interchange), same `forward(inp, labels) -> {'rgb','parsimony','tv','overlap','total'}` contract that
src/trainer.py:137-147 drives, with every per-iteration computation executed by libdbw_hip.so:

  build_blocks / build_ground / build_bkg  -> dbw_sq_blocks_*, dbw_posed_mesh_*, dbw_texture_prep_*
  Renderer (x3: coarse, fine, env)         -> dbw_project_clip_*, dbw_rasterize_*, dbw_shade_blend_*
  decoupled composite + MSE                -> dbw_composite_mse
  TV / overlap regularisers                -> dbw_tv_l2sq, dbw_overlap_loss
Only O(K)-scalar glue (opacity sigmoid/noise, parsimony over K numbers, loss weighting) stays in torch.

The perceptual term needs the third-party `lpips` package + VGG weights (absent here): it is a pluggable callable
(`perceptual_fn`), excluded from the HIP path as SURVEY.md 8(a) A10 prescribes.  `perceptual_name: ssim` installs the reference's other
registered criterion instead, SSIMLoss, as a built-in term (metrics.SSIMTerm, csrc/ssim_term.hip)."""
import warnings
from copy import deepcopy

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import mesh as M
from . import ops, phase
from .renderer import DIRECTION_LIGHT, Renderer
from .structures import PackedScene

DECIMATE_FACTOR = 8            # dbw.py:32
OVERLAP_N_POINTS = 1000        # dbw.py:33
OVERLAP_N_BLOCKS = 1.95        # dbw.py:34
OVERLAP_TEMPERATURE = 0.005    # dbw.py:35


_FUSED_SLOT = {'rgb': 0, 'parsimony': 1, 'tv': 2, 'overlap': 3}      # ops.fused_losses output layout


def safe_pow(t, exponent, eps=1e-6):      # utils/pytorch.py:35-36
    return t.clamp(eps).pow(exponent)


# loss.py:11-24: the registry's criteria on an image pair, called as criterion(imgs, rec) with their default (mean) reduction
_CRITERIA = {'mse': F.mse_loss, 'l2': F.mse_loss, 'l1': F.l1_loss, 'huber': F.smooth_l1_loss}
# loss.py:43-47 (tv_norm_funcs): norm of a difference tensor over its channel axis
_TV_NORMS = {'l1': lambda t: t.abs().sum(-1), 'l2': lambda t: safe_pow(t.pow(2).sum(-1), 0.5), 'l2sq': lambda t: t.pow(2).sum(-1)}


SURFACE_KEYS = ('points', 'tau', 'back', 'ground', 'start_epoch', 'max_cloud')
SURFACE_DEFAULTS = {'points': 16384, 'tau': 0.1, 'back': 0.5, 'ground': True, 'start_epoch': 1, 'max_cloud': 262144}
SURFACE_THIN_SEED = 20240917        # the permutation that thins a cloud above max_cloud


def parse_surface_config(entry):
    """model.loss.surface -> {points, tau, back, ground, start_epoch, max_cloud} with the defaults filled in; unknown keys are refused.
    points: cloud points drawn per step (0: all of them, in order); tau: the truncation distance; back: the weight of the direction from
    the block vertices to the cloud; ground: whether the ground's faces are part of the surface; start_epoch: the first epoch with the term;
    max_cloud: a larger cloud is thinned to this many points when it is set.  The defaults are design choices in the normalised frame, where
    the cameras sit in [-1, 1]^3 -- a tenth of the rig's half-extent as the reach of a point, 16384 points as a step's sample, the back
    direction at half weight because a block's unobserved sides have no points to answer to -- and NOT measured values."""
    from collections.abc import Mapping
    if entry is None:
        entry = {}
    if not isinstance(entry, Mapping):
        raise ValueError(f"model.loss.surface: a mapping of {', '.join(SURFACE_KEYS)}, got {entry!r}")
    bad = [k for k in entry if k not in SURFACE_KEYS]
    if bad:
        raise ValueError(f"model.loss.surface.{bad[0]}: not one of {', '.join(SURFACE_KEYS)}")
    o = dict(SURFACE_DEFAULTS, **entry)
    o.update(points=int(o['points']), tau=float(o['tau']), back=float(o['back']), ground=bool(o['ground']), start_epoch=int(o['start_epoch']),
             max_cloud=int(o['max_cloud']))
    if o['points'] < 0 or o['points'] > (1 << 24):
        raise ValueError(f"model.loss.surface.points: in [0, 2^24], got {o['points']}")
    if not (0 < o['tau'] < float('inf')):
        raise ValueError(f"model.loss.surface.tau: positive, got {o['tau']}")
    if not (0 <= o['back'] < float('inf')):
        raise ValueError(f"model.loss.surface.back: non-negative, got {o['back']}")
    if not (1 <= o['max_cloud'] <= (1 << 24)):
        raise ValueError(f"model.loss.surface.max_cloud: in [1, 2^24], got {o['max_cloud']}")
    return o


FREESPACE_KEYS = ('rays', 'tau', 'margin', 'ground', 'start_epoch', 'max_rays')
FREESPACE_DEFAULTS = {'rays': 16384, 'tau': 0.1, 'margin': 0.02, 'ground': True, 'start_epoch': 1, 'max_rays': 1048576}
FREESPACE_THIN_SEED = 20241020      # the permutation that thins the rays above max_rays


def parse_freespace_config(entry):
    """model.loss.freespace -> {rays, tau, margin, ground, start_epoch, max_rays} with the defaults filled in; unknown keys are refused.
    rays: depth rays drawn per step (0: all of them, in order); tau: where the penalty of a hit in front of the measured surface turns from
    quadratic to linear; margin: how far in front of the measured surface a hit goes unpunished (depth noise); ground: whether the ground's
    faces can stop a ray; start_epoch: the first epoch with the term; max_rays: more rays are thinned to this many when they are set.  The
    defaults are design choices in the normalised frame, where the cameras sit in [-1, 1]^3 -- a tenth of the rig's half-extent as the
    quadratic reach, a fifth of that as the depth maps' slack, 16384 rays as a step's sample, as the surface term draws points -- and NOT
    measured values."""
    from collections.abc import Mapping
    if entry is None:
        entry = {}
    if not isinstance(entry, Mapping):
        raise ValueError(f"model.loss.freespace: a mapping of {', '.join(FREESPACE_KEYS)}, got {entry!r}")
    bad = [k for k in entry if k not in FREESPACE_KEYS]
    if bad:
        raise ValueError(f"model.loss.freespace.{bad[0]}: not one of {', '.join(FREESPACE_KEYS)}")
    o = dict(FREESPACE_DEFAULTS, **entry)
    o.update(rays=int(o['rays']), tau=float(o['tau']), margin=float(o['margin']), ground=bool(o['ground']), start_epoch=int(o['start_epoch']),
             max_rays=int(o['max_rays']))
    if o['rays'] < 0 or o['rays'] > (1 << 24):
        raise ValueError(f"model.loss.freespace.rays: in [0, 2^24], got {o['rays']}")
    if not (0 < o['tau'] < float('inf')):
        raise ValueError(f"model.loss.freespace.tau: positive, got {o['tau']}")
    if not (0 <= o['margin'] < float('inf')):
        raise ValueError(f"model.loss.freespace.margin: non-negative, got {o['margin']}")
    if not (1 <= o['max_rays'] <= (1 << 24)):
        raise ValueError(f"model.loss.freespace.max_rays: in [1, 2^24], got {o['max_rays']}")
    return o


class DifferentiableBlocksWorld(nn.Module):
    name = 'dbw'

    def __init__(self, img_size, **kwargs):
        super().__init__()
        self._init_kwargs = deepcopy(kwargs)
        self._init_kwargs['img_size'] = img_size
        self.img_size = tuple(img_size) if not isinstance(img_size, int) else (img_size, img_size)
        self._init_blocks(**kwargs.get('mesh', {}))
        self._init_renderer(self.img_size, **kwargs.get('renderer', {}))
        self._init_rend_optim(**kwargs.get('rend_optim', {}))
        self.perceptual_fn = None
        self._init_loss(**kwargs.get('loss', {}))
        self.cur_epoch = 0
        self.world_size, self.rank = 1, 0     # view-sharded data parallel (parallel.py)
        self._noise_override = None
        self._overlap_u_override = None
        # sync_free=True: dead blocks (kill_blocks / filter_transparent) keep their slot and are collapsed to a point by the
        # kernel instead of being packed away on the host -> no device->host sync per iteration (dbw.py:322 `.item()`), same
        # images/losses/gradients, and the whole iteration becomes hipGraph-capturable.
        self.sync_free = False
        self.overlap_passes = False   # render the env pass on a side stream, concurrently with the fg pass (layered path only)
        self.fused_loss_epilogue = True   # training forward: composite + MSE as the epilogue of the fg pass (ops.render_decoupled_mse)

    @property
    def init_kwargs(self):
        return deepcopy(self._init_kwargs)

    # ------------------------------------------------------------------------------------------------ block poses given from outside
    @torch.no_grad()
    def init_blocks(self, T, R_6d, S, index=None):
        """Sets the poses of the blocks `index` (default: the first len(T)) to T (n,3), R_6d (n,6), S (n,3).  In-place copies into the rows of
        self.T, self.R_6d and self.S, on purpose: parallel.FlatParams re-homes p.data as views of its flat buffer, and a copy into the view
        survives that whether it comes before or after.  Nothing else is touched: opacities, shapes and textures keep their init."""
        n = T.shape[0]
        index = torch.arange(n) if index is None else torch.as_tensor(index)
        index = index.to(device=self.T.device, dtype=torch.int64).reshape(-1)
        if not (tuple(T.shape) == (n, 3) and tuple(R_6d.shape) == (n, 6) and tuple(S.shape) == (n, 3) and index.shape[0] == n):
            raise ValueError(f'init_blocks: T (n,3), R_6d (n,6), S (n,3) and index (n,) expected, got {tuple(T.shape)}, {tuple(R_6d.shape)}, '
                             f'{tuple(S.shape)}, {tuple(index.shape)}')
        if n and not (0 <= int(index.min()) and int(index.max()) < self.n_blocks):
            raise ValueError(f'init_blocks: block index outside [0, {self.n_blocks})')
        for p, v in ((self.T, T), (self.R_6d, R_6d), (self.S, S)):
            p.data.index_copy_(0, index, v.detach().to(device=p.device, dtype=p.dtype))

    def init_blocks_from_points(self, points, **kw):
        """Starts the blocks where the cloud `points` (N,3, in the frame of the cameras) has its clusters: worldfit.blocks_from_points with
        this model's world frame, block count, T_range, ratio_block_scene and scale_min, applied through init_blocks -> the BlockInit.  The
        clustering runs where the points are (a cuda device: the HIP kernel)."""
        from .worldfit import blocks_from_points
        init = blocks_from_points(points, self.S_world, self.R_world[0], self.T_world[0], self.n_blocks, T_range=self.T_range,
                                  ratio_block_scene=self.ratio_block_scene, scale_min=self.scale_min, **kw)
        self.init_blocks(init.T, init.R_6d, init.S, init.index)
        return init

    # ------------------------------------------------------------------------------------------------ init (dbw.py:55-119)
    def _init_blocks(self, **kwargs):
        self.n_blocks = kwargs.pop('n_blocks', 1)
        self.S_world = kwargs.pop('S_world', 1)
        elev, azim, roll = kwargs.pop('R_world', [0, 0, 0])
        self.register_buffer('R_world', M.world_rotation(elev, azim, roll)[None])
        self.register_buffer('T_world', torch.Tensor(kwargs.pop('T_world', [0., 0., 0.]))[None])
        self.z_far = kwargs.pop('z_far', 10)
        self.ratio_block_scene = kwargs.pop('ratio_block_scene', 1 / 4)
        self.txt_size = kwargs.pop('txt_size', 256)
        self.txt_bkg_upscale = kwargs.pop('txt_bkg_upscale', 1)
        self.scale_min = kwargs.pop('scale_min', 0.2)
        opacity_init = kwargs.pop('opacity_init', 0.5)
        T_range = kwargs.pop('T_range', [1, 1, 1])
        self.T_range = tuple(float(t) for t in T_range)         # (init_blocks_from_points: what counts as inside the scene)
        T_init_mode = kwargs.pop('T_init_mode', 'gauss')
        assert len(kwargs) == 0, kwargs
        N, TS = self.n_blocks, self.txt_size

        # sky dome + ground plane (dbw.py:74-79)
        bkg_v, bkg_f = M.get_icosphere(level=2, flip_faces=True)
        bkg_v = bkg_v * self.z_far
        self.register_buffer('bkg_verts_uvs', M.point_to_uv_sphericalmap(bkg_v))
        g_v, g_f = M.get_plane()
        g_v = g_v * torch.Tensor([self.z_far, 1, self.z_far])[None]
        for _ in range(3):
            g_v, g_f = M.subdivide_mesh(g_v, g_f)
        self.register_buffer('ground_verts_uvs', (g_v[:, [0, 2]] / self.z_far + 1) / 2)

        # block primitive = icosphere-1 superquadric (dbw.py:82-96)
        b_v, b_f = M.get_icosphere(level=1)
        self.sq_eps = nn.Parameter(torch.zeros(N, 2))
        self.register_buffer('sq_eta', torch.asin(b_v[:, 1])[None].repeat(N, 1))
        self.register_buffer('sq_omega', torch.atan2(b_v[:, 0], b_v[:, 2])[None].repeat(N, 1))
        faces_uvs, verts_uvs = M.get_icosphere_uvs(level=1, fix_continuity=True, fix_poles=True)
        p_left = abs(int(np.floor(verts_uvs.min(0)[0][0].item() * TS)))
        p_right = int(np.ceil((verts_uvs.max(0)[0][0].item() - 1) * TS))
        verts_u = (verts_uvs[..., 0] * TS + p_left) / (TS + p_left + p_right)
        verts_uvs = torch.stack([verts_u, verts_uvs[..., 1]], dim=-1)
        self.txt_padding = p_left, p_right
        self.BNF = len(faces_uvs)
        self.register_buffer('block_faces_uvs', faces_uvs)
        self.register_buffer('block_verts_uvs', verts_uvs)

        # learnable pose parameters; RNG draw order = dbw.py:99-119 (same seed -> same init as the reference)
        self.R_6d_ground = nn.Parameter(torch.Tensor([[1., 0., 0., 0., 1., 0.]]))
        self.T_ground = nn.Parameter(torch.Tensor([[0., -0.9 * T_range[1], 0.]]))
        S_init = (torch.rand(N, 3) + 0.5 - self.scale_min).log()
        R_6d_init = M.matrix_to_rotation_6d(M.random_rotations(N))
        if T_init_mode == 'gauss':
            T_init = torch.randn(N, 3) / 2 * torch.Tensor(T_range)
        elif T_init_mode == 'uni':
            T_init = (2 * torch.rand(N, 3) - 1) * torch.Tensor(T_range)
        else:
            raise NotImplementedError
        self.S = nn.Parameter(S_init.clone())
        self.R_6d = nn.Parameter(R_6d_init.clone())
        self.T = nn.Parameter(T_init.clone())
        self.alpha_logit = nn.Parameter(torch.logit(torch.ones(N) * opacity_init) + 1e-3)
        u = self.txt_bkg_upscale
        self.texture_bkg = nn.Parameter(torch.randn(1, TS * u, TS * u, 3) / 10)
        self.texture_ground = nn.Parameter(torch.randn(1, TS * u, TS * u, 3) / 10)
        self.textures = nn.Parameter(torch.randn(N, TS, TS, 3) / 10)

        # ---- constant device tables for the kernels (non-persistent: not part of checkpoints) ----
        nvb = bkg_v.shape[0]
        reg = lambda n, t: self.register_buffer(n, t.contiguous(), persistent=False)
        reg('_bkg_verts', bkg_v)
        reg('_ground_base', g_v)
        reg('_env_faces', torch.cat([bkg_f, g_f + nvb], 0).to(torch.int32))
        reg('_env_face_uvs', torch.cat([self.bkg_verts_uvs[bkg_f], self.ground_verts_uvs[g_f]], 0).float())
        reg('_env_face_map', torch.cat([torch.zeros(len(bkg_f)), torch.ones(len(g_f))]).to(torch.int32))
        reg('_env_map_desc', PackedScene.describe_maps([(TS * u, TS * u)] * 2, [(0, 0)] * 2, 'cpu')[0])
        self._n_bkg_faces, self._n_ground_faces = len(bkg_f), len(g_f)
        # cos/sin tables of the constant angle buffers, evaluated once on the host (include/dbw_hip.h: `trig`)
        reg('_trig', torch.stack([torch.cos(self.sq_eta), torch.sin(self.sq_eta), torch.cos(self.sq_omega), torch.sin(self.sq_omega)], 0))
        nv = b_v.shape[0]
        self._block_nv = nv
        reg('_block_faces_all', torch.cat([b_f + k * nv for k in range(N)], 0).to(torch.int32))
        reg('_block_face_uvs_all', verts_uvs[faces_uvs].repeat(N, 1, 1).float())
        reg('_block_face_map_all', torch.arange(N).repeat_interleave(self.BNF).to(torch.int32))
        reg('_block_map_desc_all', PackedScene.describe_maps([(TS, TS)] * N, [self.txt_padding] * N, 'cpu')[0])
        bb, bi, self._bins_per_block = PackedScene.describe_bins([(TS, TS)], 'cpu')
        bb, bi, _ = PackedScene.describe_bins([(TS, TS)] * N, 'cpu')
        reg('_block_bin_base', bb)
        reg('_block_bin_info', bi)
        reg('_block_faces_one', b_f)

    def _init_rend_optim(self, **kwargs):          # dbw.py:121-129
        self.opacity_noise = kwargs.pop('opacity_noise', False)
        self.decouple_rendering = kwargs.pop('decouple_rendering', False)
        self.coarse_learning = kwargs.pop('coarse_learning', True)
        self.decimate_txt = kwargs.pop('decimate_txt', False)
        self.decim_factor = kwargs.pop('decimate_factor', DECIMATE_FACTOR)
        self.kill_blocks = kwargs.pop('kill_blocks', False)
        assert len(kwargs) == 0, kwargs
        d = int(self.decim_factor)
        if d < 1 or (d & (d - 1)) or self.txt_size % d:
            raise NotImplementedError(f'decimate_factor={d}: the sampler keeps decimated maps at cell resolution and needs a '
                                      'power of two that divides txt_size')
        # descriptors of the decimated maps: same (h, w), stored at (h >> shift, w >> shift)
        shift, TS, u, N = d.bit_length() - 1, self.txt_size, self.txt_bkg_upscale, self.n_blocks
        dev = self._env_map_desc.device
        self.register_buffer('_env_map_desc_dec', PackedScene.describe_maps([(TS * u, TS * u)] * 2, [(0, 0)] * 2, dev, shift)[0], persistent=False)
        self.register_buffer('_block_map_desc_dec', PackedScene.describe_maps([(TS, TS)] * N, [self.txt_padding] * N, dev, shift)[0],
                             persistent=False)

    def _init_renderer(self, img_size, **kwargs):  # dbw.py:131-143
        kwargs = deepcopy(kwargs)
        if kwargs.get('shading_type', 'raw') != 'raw' or kwargs.get('lights', {}).get('name', 'ambient') != 'ambient':
            raise NotImplementedError("the model's training renderers need a backward pass: shading_type='raw' under ambient light only (flat / "
                                      'Phong shading under a directional light is forward only: renderer_light)')
        self.renderer = Renderer(img_size, **kwargs)
        kwargs['sigma'] = 5e-6
        self.renderer_fine = Renderer(img_size, **kwargs)
        kwargs['faces_per_pixel'] = 1
        kwargs['sigma'] = 0
        kwargs['detach_bary'] = False
        self.renderer_env = Renderer(img_size, **kwargs)
        # what a user looks at (predict_synthetic, dbw.py:245): flat shading under a directional light fixed to the camera, white background
        kwargs['lights'] = {'name': 'directional', 'direction': [DIRECTION_LIGHT], 'ambient_color': [[0.7, 0.7, 0.7]],
                            'diffuse_color': [[0.4, 0.4, 0.4]], 'specular_color': [[0., 0., 0.]]}
        kwargs['shading_type'] = 'flat'
        kwargs['background_color'] = (1, 1, 1)
        self.renderer_light = Renderer(img_size, **kwargs)

    def _init_loss(self, **kwargs):                # dbw.py:145-163
        weights = {'rgb': kwargs.pop('rgb_weight', 1.0), 'perceptual': kwargs.pop('perceptual_weight', 0),
                   'parsimony': kwargs.pop('parsimony_weight', 0), 'scale': kwargs.pop('scale_weight', 0),
                   'tv': kwargs.pop('tv_weight', 0), 'overlap': kwargs.pop('overlap_weight', 0)}
        # the surface term, last: the names and the order of every config without it stay what they were
        weights['surface'] = kwargs.pop('surface_weight', 0)
        self.surface_cfg = parse_surface_config(kwargs.pop('surface', None))
        # the free-space term, after it for the same reason
        weights['freespace'] = kwargs.pop('freespace_weight', 0)
        self.freespace_cfg = parse_freespace_config(kwargs.pop('freespace', None))
        name = kwargs.pop('name', 'mse')
        # loss.py:22, dbw.py:155,163: 'lpips' (a third-party network: set_perceptual) or 'ssim', the built-in term (metrics.SSIMTerm)
        self.perceptual_name = kwargs.pop('perceptual_name', 'lpips')
        tv_type = kwargs.pop('tv_type', 'l2sq')
        assert len(kwargs) == 0, kwargs
        # loss.py:11-24,43-47: the image criteria of the registry that are criteria on an RGB image pair (mse / l2, l1, huber = SmoothL1)
        # and the three total-variation norms.  The defaults of every shipped config (mse, l2sq) run inside the HIP kernels (loss epilogue of
        # the fg pass, tv_l2sq_sets); the others through torch on the rendered image / the prepared maps -- autograd then reaches the HIP
        # backward the same way (general path of compute_losses; the one-call C step and the fused loss epilogue stand aside)
        if name not in _CRITERIA:
            raise NotImplementedError(f"loss '{name}': an image criterion out of {sorted(_CRITERIA)} (loss.py:11-24; bce / cosine / ssim / "
                                      'chamfer / tv / lpips are not reconstruction criteria on an RGB image pair)')
        if tv_type not in _TV_NORMS:
            raise NotImplementedError(f"tv_type '{tv_type}': one of {sorted(_TV_NORMS)} (loss.py:43-47)")
        self.criterion_name, self.tv_type = name, tv_type
        self.default_criteria = name in ('mse', 'l2') and tv_type == 'l2sq'
        self.loss_weights = {k: v for k, v in weights.items() if v > 0}
        self.loss_names = [f'loss_{n}' for n in list(self.loss_weights.keys()) + ['total']]
        if self.perceptual_name == 'ssim' and 'perceptual' in self.loss_weights:
            from .metrics import SSIMTerm
            self.perceptual_fn = SSIMTerm()

    @property
    def _keeps_scene_verts(self):
        """whether compute_losses has a term on the posed vertices (the surface term, the free-space term)"""
        return 'surface' in self.loss_weights or 'freespace' in self.loss_weights

    def set_perceptual(self, fn):
        """fn(imgs, rec) -> scalar, e.g. lpips.LPIPS(net='vgg') with normalize=True (loss.py:32-40).  Replaces the built-in term that
        perceptual_name: ssim installed."""
        self._modules.pop('perceptual_fn', None)        # (a module installed before: a plain callable may take its place)
        self.perceptual_fn = fn

    # ------------------------------------------------------------------------------------------------ bookkeeping
    def set_cur_epoch(self, epoch):
        self.cur_epoch = epoch

    def step(self):
        self.cur_epoch += 1

    def to(self, device):
        super().to(device)
        for r in (self.renderer, self.renderer_fine, self.renderer_env, self.renderer_light):
            r.to(device)
        return self

    def release_graph(self):
        """Drop the tensors cached by the last forward (they keep its autograd graph -- and the parameters' AccumulateGrad
        nodes, which are bound to the stream they were created on -- alive)."""
        for n in ('_alpha', '_alpha_full', '_blocks_maps', '_bkg_maps', '_ground_maps', '_keep_mask', '_surface_ground_v', '_surface_block_v'):
            if hasattr(self, n):
                setattr(self, n, None)

    def is_live(self, name):                        # dbw.py:457-462
        milestone = getattr(self, name)
        if isinstance(milestone, bool):
            return milestone
        return True if self.cur_epoch < milestone else False

    @property
    def bkg_n_faces(self):
        return self._n_bkg_faces

    @property
    def ground_n_faces(self):
        return self._n_ground_faces

    @property
    def env_n_faces(self):
        return self._n_bkg_faces + self._n_ground_faces

    @property
    def blocks_n_faces(self):
        return self.n_blocks * self.BNF

    def get_opacities(self):                        # dbw.py:410-414
        alpha = torch.sigmoid(self.alpha_logit)
        if self.kill_blocks:
            alpha = alpha * (alpha > 0.01)
        return alpha

    @torch.no_grad()
    def get_nb_opaque_blocks(self):
        return (self.get_opacities() > 0.5).sum().item()

    @torch.no_grad()
    def load_state_dict(self, state_dict, strict=False):   # tolerant by-name copy, spq_ -> sq_ (dbw.py:440-455)
        state = self.state_dict()
        missing = []
        for name, param in state_dict.items():
            name = name.replace('module.', '').replace('spq_', 'sq_')
            if name in state:
                state[name].copy_(param.data if isinstance(param, nn.Parameter) else param)
            else:
                missing.append(name)
        if missing:
            warnings.warn(f'load_state_dict: {missing} not found')

    # ------------------------------------------------------------------------------------------------ scene building
    def _world_consts(self):
        return float(self.S_world), self.R_world[0].contiguous(), self.T_world[0].contiguous()

    def sky_world_verts(self):
        """The sky dome's vertices in world coordinates.  Constant geometry (no parameter involved): cached until the world transform
        changes (load_state_dict copies into the R_world / T_world buffers in place -> their version counters move; S_world is a plain
        attribute) or the model moves.  The training steps copy it in front of the ground's vertices (a new tensor: a new sky)."""
        key = (float(self.S_world), self.R_world._version, self.T_world._version, self.R_world.data_ptr(), self._bkg_verts.device)
        if getattr(self, '_bkg_world_key', None) != key:
            S_w, R_w, T_w = self._world_consts()
            self._bkg_world = ((self._bkg_verts * S_w) @ R_w + T_w).detach()
            self._bkg_world_key = key
        return self._bkg_world

    def build_env_scene(self):
        """join(build_bkg(world_coord=True), build_ground(world_coord=True))  (dbw.py:214,267-295) as a PackedScene."""
        S_w, R_w, T_w = self._world_consts()
        ph = phase.phase_of(self, self.training)
        ground_v = ops.posed_mesh(self.R_6d_ground, self.T_ground, self._ground_base, S_w, R_w, T_w)
        if self._keeps_scene_verts:
            self._surface_ground_v = ground_v       # the surface and free-space terms read the render's own vertices (compute_losses)
        bkg_maps, self._bkg_maps = ops.texture_prep(self.texture_bkg, ph.decim_env)
        g_maps, self._ground_maps = ops.texture_prep(self.texture_ground, ph.decim_env)
        verts = torch.cat([self.sky_world_verts(), ground_v], 0)
        maps = torch.cat([bkg_maps.reshape(-1), g_maps.reshape(-1)])
        scene = PackedScene(verts, self._env_faces, self._env_face_uvs, self._env_face_map, phase.env_map_desc(self, ph), maps)
        scene.const_faces = self._n_bkg_faces       # the sky dome is a buffer (dbw.py:74-76): no gradient flows to its vertices
        return scene

    def get_blocks_verts(self):
        """Block-frame superquadric vertices * ratio (dbw.py:348-352), for callers that want them unposed."""
        dev = self.sq_eps.device
        ident6 = torch.tensor([[1., 0., 0., 0., 1., 0.]], device=dev).repeat(self.n_blocks, 1)
        zeros = torch.zeros(self.n_blocks, 3, device=dev)
        logS = torch.log(torch.full((self.n_blocks, 3), 1.0 - self.scale_min, device=dev))
        eye = torch.eye(3, device=dev)
        return ops.sq_blocks(self.sq_eps, logS, ident6, zeros, self._trig, None, self.n_blocks, self.ratio_block_scene,
                             self.scale_min, 1.0, eye, None)

    def build_blocks_scene(self, filter_transparent=False):
        """build_blocks(filter_transparent, as_scene=True) (dbw.py:297-346) as a PackedScene, or None if no block is left.
        Sets self._alpha (live blocks), self._alpha_full, self._blocks_maps like the reference."""
        ph = phase.phase_of(self, self.training, filter_transparent)
        noise = None
        if ph.noise_scale:
            noise = self._noise_override if self._noise_override is not None else self._shared_randn_like(self.alpha_logit)
        # sigmoid(alpha_logit + noise), the transparency mask on the noise-free opacity and alpha * mask: one launch
        self._alpha, self._alpha_full, mask_i32 = ops.block_alpha(self.alpha_logit, noise, ph.noise_scale, ph.mask_threshold)
        keep, nb = None, self.n_blocks
        if ph.masked:
            if self.sync_free:
                keep = mask_i32
            else:
                nb = int(mask_i32.sum().item())                      # same host sync as dbw.py:322
                if nb < self.n_blocks:
                    keep = mask_i32
                    self._alpha = self._alpha[mask_i32.bool()]
        maps_all, self._blocks_maps = ops.texture_prep(self.textures, ph.decim_blocks)
        self._keep_mask = keep
        if self._keeps_scene_verts:
            self._surface_block_v = None
        if nb == 0:
            return None
        S_w, R_w, T_w = self._world_consts()
        verts = ops.sq_blocks(self.sq_eps, self.S, self.R_6d, self.T, self._trig, keep, nb, self.ratio_block_scene,
                              self.scale_min, S_w, R_w, T_w, dense=not self.sync_free)
        if self._keeps_scene_verts:
            self._surface_block_v = verts
        maps = maps_all if (keep is None or self.sync_free) else maps_all[keep.bool()]
        F_ = nb * self.BNF
        # (a view of the full table: its row 0 announces all n_blocks rows, which stay readable behind the nb rows in use)
        desc = phase.block_map_desc(self, ph)[:nb]
        self._blocks_decimated = ph.blocks_decimated
        return PackedScene(verts.reshape(-1, 3), self._block_faces_all[:F_], self._block_face_uvs_all[:F_],
                           self._block_face_map_all[:F_], desc, maps.reshape(-1), phase.block_texbins(self, ph, nb))

    def blocks_mesh(self, filter_transparent=True):
        """-> (verts (V,3) fp32, faces (F,3) int64): the posed blocks in world coordinates, live ones only, joined into one mesh in block
        order -- what the reference's build_blocks(filter_transparent, as_scene=True).get_mesh_verts_faces(0) returns (dbw.py:297-346), the
        mesh the DTU evaluation scores (eval3d.evaluate_dtu).  An evaluation-time call: under sync_free the kept blocks are packed on the
        host all the same, and the per-step state of the last forward is left as it was."""
        with torch.no_grad(), self._host_packed_rebuild():
            scene = self.build_blocks_scene(filter_transparent=filter_transparent)
        dev = self.alpha_logit.device
        if scene is None:
            return torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev)
        return scene.verts.detach().clone(), scene.faces.to(torch.int64)

    def build_scene(self, filter_transparent=False, w_bkg=True, reduce_ground=False):
        """Background + ground + blocks as ONE scene (dbw.py:250-266), for the non-decoupled hard / SSAA evaluation render.  w_bkg=False
        leaves the sky dome out; reduce_ground scales the ground's x / z by 3 / z_far in front of its pose, UVs unchanged (dbw.py:282-285)
        -- the clean mesh the evaluation exports."""
        env = self.build_env_scene() if (w_bkg and not reduce_ground) else self._build_env_variant(w_bkg, reduce_ground)
        blocks = self.build_blocks_scene(filter_transparent=filter_transparent)
        return env if blocks is None else PackedScene.join([env, blocks])

    def _build_env_variant(self, w_bkg, reduce_ground):
        """build_env_scene without the sky dome and / or with the reduced ground: an export-time scene, built from the same tables."""
        S_w, R_w, T_w = self._world_consts()
        base = self._ground_base
        if reduce_ground:
            base = (base * torch.tensor([3 / self.z_far, 1, 3 / self.z_far], device=base.device)).contiguous()
        ground_v = ops.posed_mesh(self.R_6d_ground, self.T_ground, base, S_w, R_w, T_w)
        ph = phase.phase_of(self, self.training)
        g_maps, self._ground_maps = ops.texture_prep(self.texture_ground, ph.decim_env)
        desc = phase.env_map_desc(self, ph)
        nf, nv = self._n_bkg_faces, self._bkg_verts.shape[0]
        if w_bkg:
            bkg_maps, self._bkg_maps = ops.texture_prep(self.texture_bkg, ph.decim_env)
            scene = PackedScene(torch.cat([self.sky_world_verts(), ground_v], 0), self._env_faces, self._env_face_uvs,
                                self._env_face_map, desc, torch.cat([bkg_maps.reshape(-1), g_maps.reshape(-1)]))
            scene.const_faces = nf
            return scene
        desc = desc[1:].clone()
        desc[0, 0], desc[0, 6] = 0, 1
        return PackedScene(ground_v, (self._env_faces[nf:] - nv).contiguous(), self._env_face_uvs[nf:].contiguous(),
                           torch.zeros_like(self._env_face_map[nf:]), desc, g_maps.reshape(-1))

    def _shared_randn_like(self, t):
        """Opacity noise (and the overlap samples) must be identical on every data-parallel rank: they are
        drawn from the device's default generator, which ShardedTrainStep seeds identically on all ranks and which every
        rank advances in lockstep (the default generator is also the one hipGraph capture knows how to replay)."""
        return torch.randn(t.shape, device=t.device, dtype=t.dtype)

    # ------------------------------------------------------------------------------------------------ rendering
    def _ensure_cameras(self, inp):
        if 'K' in inp and self.renderer.cameras.K is None:          # intrinsics frozen from the first sample (dbw.py:204-208)
            for r in (self.renderer, self.renderer_fine, self.renderer_env, self.renderer_light):
                r.update_cameras(device=inp['imgs'].device, K=inp['K'][0:1])

    def render_joined(self, inp, filter_transparent=False):
        """-> (B,4,H,W): the NON-decoupled rendering (dbw.py:225-232, `decouple_rendering: False`; no shipped config uses it): sky dome,
        ground and blocks joined into one scene and rendered in ONE soft pass of the phase's renderer, the env faces fully opaque
        (alpha_env = 1) next to the blocks' learned opacities.  Same kernels as the fg pass of the decoupled path."""
        self._ensure_cameras(inp)
        fine = not self.is_live('coarse_learning')
        filter_tsp = filter_transparent or fine
        renderer = self.renderer_fine if fine else self.renderer
        scene = self.build_scene(filter_transparent=filter_tsp)
        alpha = None
        if not filter_tsp:
            n_blk = scene.faces.shape[0] - self.env_n_faces
            alpha = torch.cat([torch.ones(self.env_n_faces, device=scene.verts.device), self._alpha.repeat_interleave(self.BNF)[:n_blk]])
        return renderer.render_packed(scene, inp['R'], inp['T'], faces_alpha=alpha, Kmat=inp.get('K_live'))

    def render_layers(self, inp, filter_transparent=False):
        """-> fg (B,4,H,W), env (B,4,H,W): the two passes of the decoupled rendering (dbw.py:213-222)."""
        if not self.decouple_rendering:
            raise NotImplementedError('render_layers is the decoupled rendering; decouple_rendering=False renders one joined scene: render_joined')
        self._ensure_cameras(inp)
        R, T = inp['R'], inp['T']
        K_live = inp.get('K_live')                    # intrinsics refinement: a live K in place of the renderers' frozen one
        fine = not self.is_live('coarse_learning')
        filter_tsp = filter_transparent or fine
        renderer = self.renderer_fine if fine else self.renderer
        if self.overlap_passes:
            # the env pass (hard, 1 face/pixel) and the fg pass are independent until the composite: issue the env pass on a
            # side stream so its latency-bound kernels overlap the fg kernels (autograd replays the same streams in backward)
            cur = torch.cuda.current_stream()
            side = self._side_stream = getattr(self, '_side_stream', None) or torch.cuda.Stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                env = self.renderer_env.render_packed(self.build_env_scene(), R, T, lds_aggregate=True, Kmat=K_live)
            env.record_stream(cur)
        else:
            env = self.renderer_env.render_packed(self.build_env_scene(), R, T, lds_aggregate=True, Kmat=K_live)     # magnified textures
        blocks = self.build_blocks_scene(filter_transparent=filter_tsp)
        if blocks is not None:
            alpha = None if filter_tsp else self._alpha.repeat_interleave(self.BNF)   # shared by all views (== .repeat(B))
            fg = renderer.render_packed(blocks, R, T, faces_alpha=alpha, lds_aggregate=self._blocks_decimated, Kmat=K_live)
        else:
            fg = torch.zeros_like(env)
        if self.overlap_passes:
            torch.cuda.current_stream().wait_stream(self._side_stream)
        return fg, env

    def _host_packed_rebuild(self):
        """Context of a visualisation-only rebuild of the scene with the kept blocks packed on the host (sync_free off): the per-step state
        the last forward cached (`_alpha`, `_alpha_full`, the maps, the keep mask -- a later compute_losses reads them) is put back
        afterwards, and the opacity noise of the rebuild is the forward's or none: the shared default generator, which the data-parallel
        ranks advance in lock step, is not touched."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            names = ('_alpha', '_alpha_full', '_blocks_maps', '_bkg_maps', '_ground_maps', '_keep_mask', '_blocks_decimated', '_surface_ground_v',
                     '_surface_block_v')
            saved = {n: getattr(self, n) for n in names if hasattr(self, n)}
            sf, nz, on = self.sync_free, self._noise_override, self.opacity_noise
            self.sync_free = False
            if self._noise_override is None:
                self.opacity_noise = False
            try:
                yield
            finally:
                self.sync_free, self._noise_override, self.opacity_noise = sf, nz, on
                for n, v in saved.items():
                    setattr(self, n, v)
        return ctx()

    def predict(self, inp, labels=None, w_edges=False, filter_transparent=False):
        if self.decouple_rendering:
            fg, env = self.render_layers(inp, filter_transparent)
            rec = ops.composite(fg, env)                               # rec = rec_fg*mask + (1-mask)*rec_env (dbw.py:223)
        else:
            rec = self.render_joined(inp, filter_transparent)[:, :3]   # rec, mask = renderer(scene).split([3, 1]) (dbw.py:232)
        if w_edges:                                                    # dbw.py:234-238: wireframe of the joined scene, coloured per block
            fine = not self.is_live('coarse_learning')
            filter_tsp = filter_transparent or fine
            with torch.no_grad():
                # host-packed scene (only the kept blocks): the colour table below has one row per KEPT face, while the sync-free
                # scene of the training path keeps all n_blocks blocks (culled ones collapsed to a point) and its face ids run over all
                with self._host_packed_rebuild():
                    scene = self.build_scene(filter_transparent=filter_tsp)
                colors = self.get_scene_face_colors(filter_transparent=filter_tsp).repeat(len(inp['R']), 1)
                renderer = self.renderer_fine if fine else self.renderer
                rec = renderer.draw_edges(rec, scene, inp['R'], inp['T'], colors=colors)
        return rec

    @torch.no_grad()
    def predict_synthetic(self, inp, labels=None, lit=False):
        """Blocks alone in their synthetic colours (dbw.py:240-248), exact 4x anti-aliased hard render on a white background.  lit=True is
        the reference's picture: flat shading under `renderer_light`'s directional light, which gives the blocks their visible shape
        (values reach ambient + diffuse = 1.1: the reference clamps when it saves).  lit=False: every block in its one unshaded colour."""
        self._ensure_cameras(inp)
        if self.renderer_light.cameras.K is None and self.renderer.cameras.K is not None:      # (intrinsics set on the other renderers directly)
            self.renderer_light.update_cameras(device=inp['imgs'].device, K=self.renderer.cameras.K)
        was_training = self.training
        self.eval()
        flat = self.build_synthetic_blocks()
        self.train(was_training)
        if flat is None:
            return torch.ones_like(inp['imgs'])
        if lit:
            return self.renderer_light.render_packed(flat, inp['R'], inp['T'], viz_purpose=True)[:, :3]
        bg_renderer = Renderer(self.img_size, **{**self.renderer.init_kwargs, 'background_color': (1, 1, 1)})
        bg_renderer.update_cameras(device=flat.verts.device, K=self.renderer.cameras.K)
        return bg_renderer.render_packed(flat, inp['R'], inp['T'], viz_purpose=True)[:, :3]

    @torch.no_grad()
    def build_synthetic_blocks(self):
        """build_blocks(filter_transparent=True, synthetic_colors=True, as_scene=True) (dbw.py:297-346): the opaque blocks, each in its one
        colour of the fancy colour map (a 1x1 map per block), or None when no block is left.  Host-packed: kept blocks only."""
        with self._host_packed_rebuild():
            blocks = self.build_blocks_scene(filter_transparent=True)
        if blocks is None:
            return None
        keep = (self.get_opacities() > 0.5).nonzero().flatten()
        values = torch.linspace(0, 1, self.n_blocks + 1)[1:][keep.cpu()]
        colors = torch.from_numpy(M.get_fancy_cmap()(values.numpy())).float().to(blocks.verts.device)
        desc = PackedScene.describe_maps([(1, 1)] * len(colors), [(0, 0)] * len(colors), blocks.verts.device)[0]
        return PackedScene(blocks.verts, blocks.faces, blocks.face_uvs, blocks.face_map, desc, colors.reshape(-1).contiguous())

    @torch.no_grad()
    def get_scene_face_colors(self, filter_transparent=False, w_env=True):       # dbw.py:420-431
        val_blocks = torch.linspace(0, 1, self.n_blocks + 1)[1:]
        if filter_transparent:
            val_blocks = val_blocks[self.get_opacities().cpu() > 0.5]
        elif self.kill_blocks:
            val_blocks = val_blocks[self.get_opacities().cpu() > 0.01]
        NFE = self.env_n_faces if w_env else 0
        values = torch.cat([torch.zeros(NFE), val_blocks.repeat_interleave(self.BNF)])
        return torch.from_numpy(M.get_fancy_cmap()(values.numpy())).float().to(self.sq_eps.device)

    @torch.no_grad()
    def parse_views(self, inp, filter_transparent=True, w_bkg=True):
        """What the blocks world says is in the views of `inp` (its R, T; K on first use): -> parse.SceneParse with, per pixel, the label of
        the part that is seen (0 sky, 1 ground, 2 + k block k in its ORIGINAL index, 255 nothing), its depth, and the word of all labels that
        cover the pixel, seen or hidden -- the blocks' amodal masks -- plus per view and label the amodal and the visible area.  One hard
        pass over sky, ground and blocks joined (w_bkg=False: without the sky dome), renderer.parse_packed.  A block that filter_transparent
        or kill_blocks drops leaves its label unused.  An evaluation-time call like predict(w_edges=True): the scene is packed on the host
        under sync_free too, and the per-step state of the last forward is left as it was."""
        from .parse import LABEL_BLOCK0, LABEL_GROUND, LABEL_SKY, MAX_BLOCKS, SceneParse, default_palette
        if self.n_blocks > MAX_BLOCKS:
            raise NotImplementedError(f'{self.n_blocks} blocks: the coverage word has 64 bits, two of them for sky and ground')
        self._ensure_cameras(inp)
        with self._host_packed_rebuild():
            scene = self.build_scene(filter_transparent=filter_transparent, w_bkg=w_bkg)
        opac = self.get_opacities().cpu()
        kept = opac > 0.5 if filter_transparent else (opac > 0.01 if self.kill_blocks else torch.ones_like(opac, dtype=torch.bool))
        blocks = LABEL_BLOCK0 + kept.nonzero().flatten().to(torch.int32)
        face_label = torch.cat([torch.full((self.bkg_n_faces if w_bkg else 0,), LABEL_SKY, dtype=torch.int32),
                                torch.full((self.ground_n_faces,), LABEL_GROUND, dtype=torch.int32), blocks.repeat_interleave(self.BNF)])
        if face_label.numel() != scene.faces.shape[0]:
            raise RuntimeError(f'{face_label.numel()} labels for a scene of {scene.faces.shape[0]} faces: the kept blocks are not the packed ones')
        label, depth, cover, counts = self.renderer.parse_packed(scene, face_label, inp['R'], inp['T'])
        values = torch.linspace(0, 1, self.n_blocks + 1)[1:]
        palette = default_palette(torch.from_numpy(M.get_fancy_cmap()(values.numpy())).float()[:, :3])
        return SceneParse(label, depth, cover, counts, self.n_blocks, kept, palette)

    @torch.no_grad()
    def get_arranged_block_txt(self):                                            # dbw.py:433-438
        maps = torch.sigmoid(self.textures).permute(0, 3, 1, 2)
        ncol, nrow = 5, len(maps) // 5
        rows = [torch.cat([maps[k] for k in range(ncol * i, ncol * (i + 1))], dim=2) for i in range(nrow)]
        return torch.cat(rows, dim=1)[None]

    def forward(self, inp, labels=None):
        self._view_ids = inp.get('view_ids')          # (for a perceptual criterion with cached targets: _perceptual_term)
        try:
            return self._forward(inp)
        finally:
            self._view_ids = None

    def _forward(self, inp):
        if inp['imgs'].shape[0] == 0:
            # a data-parallel rank whose shard is exhausted (parallel.py / trainer.py: uneven shards): nothing to render, the step
            # only carries this rank's share of the view-independent regularisers
            self.build_env_scene()
            self.build_blocks_scene(filter_transparent=not self.is_live('coarse_learning'))
            return self.compute_losses(inp['imgs'], None, layers=None)
        if 'exposure' in inp:
            # per-view exposure compensation: the fused epilogue stands aside as it does for masks, the layers are rendered
            # and both image terms see rec = exp(g) * composite + b; validity masks combine with it
            refusal = self._exposure_refusal()
            if refusal is not None:
                raise NotImplementedError(f'a batch with exposure: {refusal}')
            if 'view_ids' not in inp:
                raise KeyError("a batch with 'exposure' carries 'view_ids', the rows of theta of its views")
            masks, count = inp.get('masks'), None
            if masks is not None:
                count = 3.0 * float(inp['mask_sum'] if 'mask_sum' in inp else masks.sum(dtype=torch.float64))      # (one host read without it)
            fg, env = self.render_layers(inp)
            return self.compute_losses(inp['imgs'], None, layers=(fg, env), masks=masks, mask_count=count,
                                       exposure=(inp['exposure'], inp['view_ids'], inp.get('view_ids_host')))
        if 'masks' in inp:
            # validity masks: the fused epilogue stands aside, the layers are rendered and both image terms take the masks
            refusal = self._mask_refusal()
            if refusal is not None:
                raise NotImplementedError(f'a batch with masks: {refusal}')
            masks = inp['masks']
            msum = inp['mask_sum'] if 'mask_sum' in inp else float(masks.sum(dtype=torch.float64))      # (one host read without it)
            fg, env = self.render_layers(inp)
            return self.compute_losses(inp['imgs'], None, layers=(fg, env), masks=masks, mask_count=3.0 * float(msum))
        if not self.decouple_rendering:                                # one joined scene, one soft pass; losses through the general path
            return self.compute_losses(inp['imgs'], self.render_joined(inp)[:, :3])
        fused = self._forward_fused(inp) if self.fused_loss_epilogue else None
        if fused is not None:
            return fused
        fg, env = self.render_layers(inp)
        return self.compute_losses(inp['imgs'], None, layers=(fg, env))

    def _mask_refusal(self):
        """-> why this model cannot take a batch with validity masks, or None."""
        if not self.decouple_rendering:
            return 'decouple_rendering is off: the masked reconstruction term is the decoupled composite'
        if 'rgb' not in self.loss_weights or not self.default_criteria:
            return f'criteria {self.criterion_name} / {self.tv_type}: the masked kernels have mse and l2sq, with an rgb term'
        if self.world_size > 1:
            return 'data-parallel training needs a global valid count, which is not implemented'
        return None

    def _exposure_refusal(self):
        """-> why this model cannot take a batch with per-view exposures, or None."""
        if not self.decouple_rendering:
            return 'decouple_rendering is off: the compensated reconstruction term is the decoupled composite'
        if 'rgb' not in self.loss_weights or not self.default_criteria:
            return f'criteria {self.criterion_name} / {self.tv_type}: the exposure kernel has mse and l2sq, with an rgb term'
        if self.world_size > 1:
            return 'data-parallel training: the exposure gradients are per view and the ranks do not exchange them'
        return None

    def _forward_fused(self, inp):
        """The training iteration with the reconstruction loss as the epilogue of the fg pass (ops.render_decoupled_mse): env pass,
        then fg pass + decoupled composite + MSE in one kernel -- no fg image, no composite kernel, no image-sized gradient round
        trips.  Returns None when the configuration needs the general path (non-decoupled, perceptual term, no block left, layered
        fallbacks switched off)."""
        if 'perceptual' in self.loss_weights:
            return None
        self._ensure_cameras(inp)
        fine = phase.phase_of(self, self.training).fine_renderer
        renderer = self.renderer_fine if fine else self.renderer
        if phase.fast_path_refusal(self, renderer) is not None:
            return None
        blocks = self.build_blocks_scene(filter_transparent=fine)
        if blocks is None or blocks.faces.shape[0] >= (1 << 20) or blocks.map_desc.shape[0] >= (1 << 11):
            return None
        env = self.build_env_scene()
        R, T = inp['R'].float().contiguous(), inp['T'].float().contiguous()
        K_live = inp.get('K_live')                    # intrinsics refinement
        Kmat = (renderer.cameras.K[0] if K_live is None else K_live.reshape(4, 4).float()).to(R.device).contiguous()
        alpha = None if fine else self._alpha.repeat_interleave(self.BNF)
        cfg_e = self.renderer_env._cfg(env.faces.shape[0], lds_aggregate=True, const_faces=env.const_faces)
        cfg_f = renderer._cfg(blocks.faces.shape[0], lds_aggregate=self._blocks_decimated, texbins=blocks.texbins)
        imgs = inp['imgs']
        count = imgs.numel() if getattr(self, '_global_count', None) is None else self._global_count
        rgb = ops.render_decoupled_mse(env, blocks, alpha, imgs, float(self.loss_weights['rgb']) / float(count), R, T, Kmat, cfg_e, cfg_f,
                                       self.renderer_env._bg, renderer._bg)
        return self.compute_losses(imgs, None, layers=None, rgb_value=rgb)

    # ------------------------------------------------------------------------------------------------ evaluation (dbw.py:464-493)
    @torch.no_grad()
    def quantitative_eval(self, loader, device, hard_inference=True):
        """PSNR / SSIM (/ LPIPS when a perceptual network was supplied with set_perceptual; never the built-in SSIM term) of the reconstruction over `loader`
        (batches of (inp, labels) like the reference's datasets).  hard_inference: exact anti-aliased render of the joined scene
        (4x resolution, sigma 0, one face per pixel, 4x4 average pooling; renderer.py:56-60,178-183), else the soft decoupled
        prediction.  -> OrderedDict like the reference's; LPIPS is NaN when no network is installed."""
        from collections import OrderedDict
        from .metrics import AverageMeter, SSIMTerm, mse2psnr, ssim
        was_training = self.training
        self.eval()
        opacities = self.get_opacities()
        n_blocks = int((opacities > 0.5).sum().item())
        meters = {k: AverageMeter() for k in ('L_tot', 'L_rec', 'PSNR', 'SSIM', 'LPIPS')}
        scene = self.build_scene(filter_transparent=True) if hard_inference else None
        for inp, labels in loader:
            inp = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in inp.items()}
            imgs, N = inp['imgs'], len(inp['imgs'])
            if hard_inference:
                self._ensure_cameras(inp)
                rec = self.renderer.render_packed(scene, inp['R'], inp['T'], viz_purpose=True)[:, :3]
            else:
                rec = self.predict(inp, labels, filter_transparent=True)
            losses = self.compute_losses(imgs, rec)
            meters['L_tot'].update(losses['total'], N=N)
            meters['L_rec'].update(sum(losses[k] for k in ('rgb', 'perceptual') if k in losses), N=N)
            meters['PSNR'].update(mse2psnr(F.mse_loss(imgs, rec)), N=N)
            meters['SSIM'].update(ssim(imgs, rec, padding=False).mean(), N=N)
            # (the built-in SSIM term is no LPIPS: the column stays NaN, the term is part of L_rec and L_tot)
            lpips_fn = None if isinstance(self.perceptual_fn, SSIMTerm) else self.perceptual_fn
            meters['LPIPS'].update(lpips_fn(imgs, rec) if lpips_fn is not None else float('nan'), N=N)
        self.train(was_training)
        return OrderedDict([('n_blocks', n_blocks)] + [(k, m.avg) for k, m in meters.items()]
                           + [(f'alpha{k}', a.item()) for k, a in enumerate(opacities)])

    # ------------------------------------------------------------------------------------------------ qualitative evaluation (dbw.py:495-554)
    @torch.no_grad()
    def qualitative_eval(self, loader, device, path=None, NV=240, parse=False):
        """The pictures, meshes and videos of a trained model, the file set of the reference (dbw.py:495-554), under `path`:
        textures/{bkg,ground,block_XX}.png; rotated_mesh.*; mesh_full.obj and mesh.obj (without the sky dome, reduced ground), each with its
        .mtl and .png; gt.ply (3000 points of loader.dataset.pc_gt under seed 123, where the dataset has one); and per input i (at most
        10): i_inp, i_rec, i_rec_col, i_rec_col_inp, i_rec_syn_nobkg, i_rec_syn_nobkg_edged .png and the two trajectories i_rec_traj.*,
        i_rec_traj_syn.* over R @ R_traj of get_circle_traj(N_views=NV).  Videos are mp4 where imageio imports, animated GIFs otherwise
        (export.save_video); rotated_mesh has NV views too (the reference's 240 is its NV).  Stops after the meshes when no block is
        opaque.  parse=True adds <path>/parse/: the scene parsing maps of those inputs (parse_views, export.write_parse).
        `loader`: any iterable of (inp, labels); its batch_size, or the size of the first batch, numbers the inputs.  Every frame is
        converted to 8 bits on the GPU (renderer.render_views_u8, ops.frames_u8).  The train / eval state is put back on exit.
        -> {'render': seconds in render + conversion + copy, 'encode': seconds in the file writers}."""
        import time
        from pathlib import Path
        from . import export
        from .renderer import get_circle_traj, render_rotated_views_u8, render_views_u8, _pooled_color
        path = Path(path or '.')
        path.mkdir(parents=True, exist_ok=True)
        spent = {'render': 0.0, 'encode': 0.0}

        def timed(kind, fn, *a, **k):
            t0 = time.perf_counter()
            out = fn(*a, **k)
            spent[kind] += time.perf_counter() - t0
            return out

        def still(name, src, **k):
            frame = timed('render', lambda: ops.frames_u8(src, **k)[0].cpu())
            timed('encode', export.save_png, frame, path / name)

        was_training = self.training
        self.eval()
        try:
            # Textures: the prepared maps (sigmoid of the parameters), (n,h,w,3)
            (path / 'textures').mkdir(exist_ok=True)
            for name, param in (('bkg', self.texture_bkg), ('ground', self.texture_ground), ('block_', self.textures)):
                frames = timed('render', lambda: ops.frames_u8(ops.texture_prep(param.detach())[0], hwc=True).cpu())
                for k, frame in enumerate(frames):
                    timed('encode', export.save_png, frame, path / 'textures' / (f'block_{str(k).zfill(2)}.png' if name == 'block_' else f'{name}.png'))

            # Basic 3D
            with self._host_packed_rebuild():       # host-packed: the colour table below has one row per KEPT face
                meshes = self.build_scene(filter_transparent=True)
                clean_mesh = self.build_scene(filter_transparent=True, w_bkg=False, reduce_ground=True)
            colors = self.get_scene_face_colors(filter_transparent=True, w_env=False)
            first = next(iter(loader))[0]
            self._ensure_cameras({k: (v.to(device) if torch.is_tensor(v) else v) for k, v in first.items()})
            frames = timed('render', render_rotated_views_u8, meshes, renderer=self.renderer, n_views=NV, elev=30, dist=2.732)
            timed('encode', export.save_video, frames, path / 'rotated_mesh.mp4')
            timed('encode', export.save_scene_as_obj, meshes, path / 'mesh_full.obj')
            timed('encode', export.save_scene_as_obj, clean_mesh, path / 'mesh.obj')
            syn_blocks = self.build_synthetic_blocks()
            if syn_blocks is None:
                return spent
            # GT pointcloud
            gt = getattr(getattr(loader, 'dataset', None), 'pc_gt', None)
            if gt is not None:
                gt = torch.as_tensor(gt)
                gt = gt[torch.randperm(len(gt), generator=torch.Generator().manual_seed(123))[:3000]]
                timed('encode', export.save_ply, path / 'gt.ply', gt)

            renderer, renderer_light = self.renderer, self.renderer_light
            H, W = self.img_size
            count, N, parses = 0, 10, []
            R_traj = get_circle_traj(N_views=NV)[0].to(device)
            n_zeros = int(np.log10(N - 1)) + 1
            BS = getattr(loader, 'batch_size', None)
            grey = _pooled_color(torch.tensor([0.3, 0.3, 0.3], device=device))
            for j, (inp, labels) in enumerate(loader):
                if count >= N:
                    break
                inp = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in inp.items()}
                img_src, R_src, T_src = inp['imgs'], inp['R'], inp['T']
                BS = len(img_src) if BS is None else BS
                B = min(len(img_src), N - count)
                for k in range(B):
                    i = str(j * BS + k).zfill(n_zeros)
                    img = img_src[k:k + 1].float().contiguous()
                    R, T = R_src[k:k + 1], T_src[k:k + 1]
                    still(f'{i}_inp.png', img)
                    rec = timed('render', renderer.render_viz, meshes, R, T)
                    still(f'{i}_rec.png', rec)
                    mask, col = timed('render', renderer.edge_layers, syn_blocks, R, T, (H, W), colors)
                    still(f'{i}_rec_col.png', rec, mask=mask, edge_color=col)
                    still(f'{i}_rec_col_inp.png', img, mask=mask, edge_color=col)
                    rec = timed('render', renderer_light.render_viz, syn_blocks, R, T)
                    still(f'{i}_rec_syn_nobkg.png', rec)
                    mask, _ = timed('render', renderer_light.edge_layers, syn_blocks, R, T, (H, W), colors.new_zeros(3), linewidth=0.7)
                    still(f'{i}_rec_syn_nobkg_edged.png', rec, mask=mask, edge_color=grey)
                    R_v, T_v = (R @ R_traj).contiguous(), T.expand(NV, -1).contiguous()
                    frames = timed('render', render_views_u8, meshes, R_v, T_v, renderer=renderer)
                    timed('encode', export.save_video, frames, path / f'{i}_rec_traj.mp4')
                    frames = timed('render', render_views_u8, syn_blocks, R_v, T_v, renderer=renderer_light)
                    timed('encode', export.save_video, frames, path / f'{i}_rec_traj_syn.mp4')
                if parse:
                    parses.append(timed('render', self.parse_views, {**inp, 'R': R_src[:B], 'T': T_src[:B]}))
                count += B
            if parse:
                timed('encode', export.write_parse, export.join_parses(parses), path / 'parse')
            return spent
        finally:
            self.train(was_training)

    # ------------------------------------------------------------------------------------------------ losses (dbw.py:361-408)
    def _perceptual_term(self, imgs, rec, coarse, view_ids=None, masks=None, count=None):
        """view_ids: the batch's `view_ids` entry, if the caller's loader provides one (trainer.py does) -- handed to a criterion that keeps
        the constant half of its work per training view (lpips_vgg.LPIPSVGG.cache_targets); never needed for the value.
        masks, count: a criterion that declares takes_masks = True (metrics.SSIMTerm) receives them; any other is called on
        imgs * masks and rec * masks, its own normalisation left alone (a target cache was built from imgs * masks: trainer.py)."""
        if self.perceptual_fn is None:
            raise RuntimeError('perceptual_weight > 0 needs model.set_perceptual(fn): lpips is a third-party network '
                               "outside the HIP path (SURVEY.md 8a A10); loss.perceptual_name: 'ssim' installs the built-in SSIM term")
        # the perceptual criterion is a mean over the views it is given: under view-sharded data parallelism the gradients of all ranks
        # are SUMMED, so a rank's term is weighted by its share of the global batch (like the MSE, which is normalised by the
        # global element count) -- the sum over ranks is then the reference's mean over the whole batch
        share = 1.0
        if self.world_size > 1 and getattr(self, '_global_count', None):
            share = imgs.numel() / float(self._global_count)
        if masks is not None and getattr(self.perceptual_fn, 'takes_masks', False):
            value = self.perceptual_fn(imgs, rec, masks=masks, count=count)
            return self.loss_weights['perceptual'] * phase.late_factor(coarse) * share * value
        if masks is not None:
            imgs, rec = imgs * masks, rec * masks
        if view_ids is not None and getattr(self.perceptual_fn, 'target_cache', None) is not None:
            value = self.perceptual_fn(imgs, rec, view_ids=view_ids)
        else:
            value = self.perceptual_fn(imgs, rec)
        return self.loss_weights['perceptual'] * phase.late_factor(coarse) * share * value

    # ------------------------------------------------------------------------------------------------ the surface term
    @torch.no_grad()
    def set_surface_points(self, points):
        """The capture's cloud (N,3), in the normalised frame of R, T and of the posed meshes, for the surface term: kept as a non-persistent
        buffer (a checkpoint does not carry it: the cloud is rebuilt from the scene).  More than surface.max_cloud points are thinned to the
        first max_cloud of a seeded permutation; points with a non-finite coordinate are dropped."""
        p = torch.as_tensor(points).detach().to(device=self.alpha_logit.device, dtype=torch.float32).reshape(-1, 3)
        p = p[torch.isfinite(p).all(1)]
        cap = self.surface_cfg['max_cloud']
        if p.shape[0] > cap:
            perm = torch.randperm(p.shape[0], generator=torch.Generator().manual_seed(SURFACE_THIN_SEED))[:cap]
            p = p[perm.to(p.device)]
        if p.shape[0] == 0:
            raise ValueError('set_surface_points: no finite point')
        self._buffers.pop('_surface_points', None)
        self.register_buffer('_surface_points', p.contiguous(), persistent=False)
        return p.shape[0]

    def _surface_tables(self, nb, ground, dev):
        """Constant tables of the term for `nb` packed blocks: faces (F,3) int32 into [ground vertices, block vertices], the groups' face
        offsets, each vertex's row of the opacities (-1 on the ground), a one for the ground's entry of group_keep.  The faces index the
        vertices by construction (asserted once, here, on the host).  Fifth: each group's row of the opacities (-1 for the ground)."""
        key = (nb, ground, str(dev))
        cache = self.__dict__.setdefault('_surface_table_cache', {})
        if key not in cache:
            nvb, nv = self._bkg_verts.shape[0], self._block_nv
            gf = (self._env_faces[self._n_bkg_faces:].cpu() - nvb) if ground else torch.zeros(0, 3, dtype=torch.int32)
            ngv = self._ground_base.shape[0] if ground else 0
            bf = self._block_faces_all[:nb * self.BNF].cpu() + ngv
            faces = torch.cat([gf, bf], 0).to(torch.int32).contiguous()
            fg = torch.tensor(([0, len(gf)] if ground else [0]) + [len(gf) + (k + 1) * self.BNF for k in range(nb)], dtype=torch.int32)
            vg = torch.cat([torch.full((ngv,), -1), torch.arange(nb).repeat_interleave(nv)]).to(torch.int32)
            assert faces.numel() and 0 <= int(faces.min()) and int(faces.max()) < len(vg)
            ga = torch.tensor(([-1] if ground else []) + list(range(nb)), dtype=torch.int32)
            cache[key] = (faces.to(dev), fg.to(dev), vg.to(dev), torch.ones(1, dtype=torch.int32, device=dev), ga.to(dev))
        return cache[key]

    def _posed_term_scene(self, c, what, dev):
        """What a term on the posed meshes (`what`: its name in the message, c: its config) measures against: the vertex tensors the last
        build_env_scene / build_blocks_scene produced and their constant tables -> (verts (V,3) fp32, faces, face_group, vert_group,
        keep or None, nb), or None when no face is left."""
        ground_v = getattr(self, '_surface_ground_v', None) if c['ground'] else None
        block_v = getattr(self, '_surface_block_v', None)
        if c['ground'] and ground_v is None:
            raise RuntimeError(f'the {what} term reads the vertices of the scene the forward built: call the model, not compute_losses alone')
        if ground_v is None and block_v is None:
            return None
        nb = 0 if block_v is None else block_v.reshape(-1, self._block_nv, 3).shape[0]
        faces, face_group, vert_group, one, _ = self._surface_tables(nb, ground_v is not None, dev)
        parts = [v.reshape(-1, 3) for v in (ground_v, block_v) if v is not None]
        verts = parts[0] if len(parts) == 1 else torch.cat(parts, 0)
        keep = self._keep_mask if (self.sync_free and nb) else None
        if keep is not None and ground_v is not None:
            keep = torch.cat([one, keep.to(torch.int32)])
        return verts.float().contiguous(), faces, face_group, vert_group, None if keep is None else keep.contiguous(), nb

    def _term_step(self, counter):
        """The step a term's draw is numbered by: the trainer's, or -- a model stepped by hand -- the term's own count of training losses."""
        step = getattr(self, '_rng_step', None)
        if step is None:
            step = self.__dict__.setdefault(counter, 0)
            setattr(self, counter, step + 1)
        return int(step)

    def _surface_term(self, dev):
        """weight * the term on the vertex tensors the last build_env_scene / build_blocks_scene produced (no second sq_blocks launch)."""
        c, wgt = self.surface_cfg, float(self.loss_weights['surface'])
        if self.world_size > 1:
            raise NotImplementedError('the surface term under data parallelism: every rank would add the whole term, and the ranks do not '
                                      'share out its points')
        pts = getattr(self, '_surface_points', None)
        if pts is None:
            raise RuntimeError('surface_weight > 0 needs the capture\'s point cloud: model.set_surface_points(points) (train.py feeds '
                               'scene.cloud() of a custom scene)')
        if self.cur_epoch + 1 < c['start_epoch'] or not self.training:
            # (before start_epoch; and in eval mode: the term is a training signal, an evaluation neither pays for the nearest-neighbour search
            # over the cloud nor counts the term in its L_tot -- loss_surface is then 0)
            return torch.zeros((), device=dev)
        scene = self._posed_term_scene(c, 'surface', dev)
        if scene is None:                                 # no face left: every point is at tau
            return torch.full((), wgt * c['tau'] ** 2, device=dev)
        verts, faces, face_group, vert_group, keep, nb = scene
        return ops.surface_term(pts, verts, faces, face_group, keep, self._alpha.float().contiguous() if nb else None, vert_group,
                                n_points=min(c['points'], 1 << 24), tau=c['tau'], back=c['back'] if nb else 0.0,
                                seed=int(getattr(self, '_rng_seed', 227391)) & 0x7fffffffffffffff, step=self._term_step('_surface_calls'),
                                weight=wgt, back_count=float(self.n_blocks * self._block_nv))

    # ------------------------------------------------------------------------------------------------ the free-space term
    @torch.no_grad()
    def set_freespace_rays(self, ends, frame, origins):
        """The capture's depth rays for the free-space term, in the normalised frame of R, T and of the posed meshes: ray j runs from
        origins[frame[j]] (a camera centre) to ends[j] (the measured surface point).  Kept as non-persistent buffers (a checkpoint does not
        carry them: the rays are rebuilt from the scene).  Rays with a non-finite coordinate, or a frame outside the table, are dropped; more
        than freespace.max_rays are thinned to the first max_rays of a seeded permutation -> the number kept."""
        dev = self.alpha_logit.device
        p = torch.as_tensor(ends).detach().to(device=dev, dtype=torch.float32).reshape(-1, 3)
        f = torch.as_tensor(frame).detach().to(device=dev).reshape(-1).to(torch.int64)
        o = torch.as_tensor(origins).detach().to(device=dev, dtype=torch.float32).reshape(-1, 3)
        if f.shape[0] != p.shape[0]:
            raise ValueError(f'set_freespace_rays: {f.shape[0]} frames for {p.shape[0]} ends')
        ok = torch.isfinite(p).all(1) & (f >= 0) & (f < o.shape[0])
        ok &= torch.isfinite(o).all(1)[f.clamp(0, max(o.shape[0] - 1, 0))] if o.shape[0] else torch.zeros_like(ok)
        p, f = p[ok], f[ok]
        cap = self.freespace_cfg['max_rays']
        if p.shape[0] > cap:
            perm = torch.randperm(p.shape[0], generator=torch.Generator().manual_seed(FREESPACE_THIN_SEED))[:cap].to(dev)
            p, f = p[perm], f[perm]
        if p.shape[0] == 0:
            raise ValueError('set_freespace_rays: no finite ray')
        for n, t in (('_freespace_ends', p.contiguous()), ('_freespace_frame', f.to(torch.int32).contiguous()), ('_freespace_origins', o.contiguous())):
            self._buffers.pop(n, None)
            self.register_buffer(n, t, persistent=False)
        return p.shape[0]

    def _freespace_term(self, dev):
        """weight * the term on the vertex tensors the last build_env_scene / build_blocks_scene produced (no second sq_blocks launch)."""
        c, wgt = self.freespace_cfg, float(self.loss_weights['freespace'])
        if self.world_size > 1:
            raise NotImplementedError('the free-space term under data parallelism: every rank would add the whole term, and the ranks do not '
                                      'share out its rays')
        ends = getattr(self, '_freespace_ends', None)
        if ends is None:
            raise RuntimeError('freespace_weight > 0 needs the capture\'s depth rays: model.set_freespace_rays(ends, frame, origins) (train.py '
                               'feeds scene.rays() of a custom scene with depth maps)')
        if self.cur_epoch + 1 < c['start_epoch'] or not self.training:
            # (before start_epoch; and in eval mode: the term is a training signal, an evaluation does not count it in its L_tot)
            return torch.zeros((), device=dev)
        scene = self._posed_term_scene(c, 'free-space', dev)
        if scene is None:                                 # no face left: no ray is stopped
            return torch.zeros((), device=dev)
        verts, faces, face_group, _, keep, nb = scene
        group_alpha = self._surface_tables(nb, bool(c['ground']), dev)[4]
        return ops.freespace_term(ends, self._freespace_frame, self._freespace_origins, verts, faces, face_group, keep, group_alpha,
                                  self._alpha.float().contiguous() if nb else None, n_rays=min(c['rays'], 1 << 24), tau=c['tau'],
                                  margin=c['margin'], seed=int(getattr(self, '_rng_seed', 227391)) & 0x7fffffffffffffff,
                                  step=self._term_step('_freespace_calls'), weight=wgt)

    def compute_losses(self, imgs, rec, layers=None, rgb_value=None, masks=None, mask_count=None, exposure=None):
        """The loss dict of _image_and_regulariser_losses (same arguments), plus -- with surface_weight > 0 -- the surface term
        and -- with freespace_weight > 0 -- the free-space term, both on the vertices of the scene the forward built (zero in
        eval mode and before their start_epoch); without a weight no line of its term runs."""
        losses = self._image_and_regulariser_losses(imgs, rec, layers=layers, rgb_value=rgb_value, masks=masks, mask_count=mask_count, exposure=exposure)
        if 'surface' in self.loss_weights:
            total = losses.pop('total')
            losses['surface'] = self._surface_term(imgs.device)
            losses['total'] = total + losses['surface']
        if 'freespace' in self.loss_weights:                # (the same shape, after it)
            total = losses.pop('total')
            losses['freespace'] = self._freespace_term(imgs.device)
            losses['total'] = total + losses['freespace']
        return losses

    def _image_and_regulariser_losses(self, imgs, rec, layers=None, rgb_value=None, masks=None, mask_count=None, exposure=None):
        """masks (B,1,H,W) weights in [0, 1] with mask_count = 3 * their sum (a host number; computed with one host read when None): the
        two image terms under the validity mask -- layers must be given --, the regularisers unchanged.
        exposure = (theta (V,6), ids (B)[, ids on the host]): the per-view exposures of DESIGN.md 6s and the batch's rows of them -- both
        image terms see rec = exp(g) * composite + b (ops.composite_mse_exposure), with or without masks; layers must be given; the
        regularisers do not see theta."""
        w = self.loss_weights
        if 'surface' in w or 'freespace' in w:
            w = {k: v for k, v in w.items() if k not in ('surface', 'freespace')}       # (compute_losses adds those terms)
        dev = imgs.device
        # (the epoch's loss factors in eval mode too; view-independent regularisers: every rank computes them identically, scaled by
        # 1 / world_size so that the sum all-reduce of gradients counts them once)
        ph = phase.phase_of(self, self.training)
        coarse, rs, ws = ph.coarse_epoch, ph.rs, self.world_size
        if masks is not None or exposure is not None:
            what, refusal = 'masks', None if masks is None else self._mask_refusal()
            if refusal is None and exposure is not None:
                what, refusal = 'exposure', self._exposure_refusal()
            refusal = refusal or (None if layers is not None else 'compute_losses needs the rendered layers')
            if refusal is not None:
                raise NotImplementedError(f'a batch with {what}: {refusal}')
            if masks is None:
                count = float(imgs.numel() if getattr(self, '_global_count', None) is None else self._global_count)
            else:
                count = ops.mask_count(masks) if mask_count is None else float(mask_count)
            # composite + masked MSE as one node with two outputs (its backward: one launch fed by the gradients of both), the regularisers
            # through the regularisers-only form of ops.fused_losses, the perceptual term on the node's rec
            if exposure is not None:
                rgb, rec = ops.composite_mse_exposure(layers[0], layers[1], imgs, masks, ph.w_rgb, count, exposure[0], exposure[1],
                                                      ids_host=exposure[2] if len(exposure) > 2 else None)
            else:
                rgb, rec = ops.composite_mse_masked(layers[0], layers[1], imgs, masks, ph.w_rgb, count)
            cfg = {'rgb': None, 'count': count, 'parsimony': ph.w_parsimony, 'tv': ph.w_tv, 'tv_ground_factor': ph.tv_factor,
                   'overlap': ph.w_overlap, 'overlap_consts': (float(self.ratio_block_scene), float(self.scale_min), OVERLAP_TEMPERATURE, OVERLAP_N_BLOCKS)}
            u = None
            if cfg['overlap']:
                u = self._overlap_u_override
                if u is None:
                    u = torch.rand(self.n_blocks, OVERLAP_N_POINTS, 3, device=dev)
            vals = ops.fused_losses(None, None, imgs, self._alpha_full, self._bkg_maps, self._blocks_maps, self._ground_maps,
                                    self.sq_eps, self.S, self.R_6d, self.T, u, cfg)
            losses = {k: vals[_FUSED_SLOT[k]] for k in w if k in _FUSED_SLOT}
            losses['rgb'] = rgb
            total = vals.sum() + rgb
            if 'perceptual' in w:
                losses['perceptual'] = self._perceptual_term(imgs, rec, coarse, getattr(self, '_view_ids', None), masks=masks, count=count)
                total = total + losses['perceptual']
            losses = {k: losses[k] for k in w}
            losses['total'] = total
            return losses
        if (layers is not None or rgb_value is not None) and 'rgb' in w and self.default_criteria:
            # training path: composite + MSE and the regularisers as ONE autograd node (ops.fused_losses), the phase's weights
            # folded into the kernels' scales
            count = imgs.numel() if getattr(self, '_global_count', None) is None else self._global_count
            cfg = {'rgb': ph.w_rgb, 'count': float(count), 'parsimony': ph.w_parsimony, 'tv': ph.w_tv, 'tv_ground_factor': ph.tv_factor,
                   'overlap': ph.w_overlap, 'overlap_consts': (float(self.ratio_block_scene), float(self.scale_min), OVERLAP_TEMPERATURE, OVERLAP_N_BLOCKS)}
            u = None
            if cfg['overlap']:
                u = self._overlap_u_override
                if u is None:
                    u = torch.rand(self.n_blocks, OVERLAP_N_POINTS, 3, device=dev)
            fg_l, env_l = layers if layers is not None else (None, None)
            vals = ops.fused_losses(fg_l, env_l, imgs, self._alpha_full, self._bkg_maps, self._blocks_maps, self._ground_maps,
                                    self.sq_eps, self.S, self.R_6d, self.T, u, cfg)
            losses = {}
            for k in w:
                if k in _FUSED_SLOT:
                    losses[k] = vals[_FUSED_SLOT[k]]
            total = vals.sum()
            if rgb_value is not None:       # reconstruction term already reduced by the fg pass's epilogue (slot 0 of vals is 0)
                losses['rgb'] = rgb_value
                total = total + rgb_value
            if 'perceptual' in w:
                losses['perceptual'] = self._perceptual_term(imgs, ops.composite(*layers), coarse, getattr(self, '_view_ids', None))
                total = total + losses['perceptual']
            losses = {k: losses[k] for k in w}
            losses['total'] = total
            return losses
        losses = {k: torch.zeros((), device=dev) for k in w}          # (fill kernel: hipGraph-capturable, unlike an H2D copy)
        empty = imgs.shape[0] == 0                                     # no views on this rank in this step: regularisers only
        if 'rgb' in losses and not empty:
            # a mean over the GLOBAL batch under view-sharded data parallelism (the ranks' gradients are summed)
            share = imgs.numel() / float(self._global_count) if (ws > 1 and getattr(self, '_global_count', None)) else 1.0
            losses['rgb'] = w['rgb'] * share * _CRITERIA[self.criterion_name](imgs, rec if rec is not None else ops.composite(*layers))
        if 'perceptual' in losses and not empty:
            losses['perceptual'] = self._perceptual_term(imgs, rec if rec is not None else ops.composite(*layers), coarse, getattr(self, '_view_ids', None))
        if 'parsimony' in losses:
            factor = 1 if coarse else 0
            alpha = self._alpha_full if coarse else (self._alpha_full > 0.5).float()
            losses['parsimony'] = w['parsimony'] * factor * rs * safe_pow(alpha, 0.5).mean()
        if 'tv' in losses:
            factor = ph.tv_factor
            if self.tv_type == 'l2sq':
                tv = ops.tv_l2sq(self._bkg_maps) + ops.tv_l2sq(self._blocks_maps, wrap_x=True) + ops.tv_l2sq(self._ground_maps) * factor
            else:       # dbw.py:378-387 with tv_norm_funcs['l1' | 'l2'], in torch on the prepared maps
                norm, bm = _TV_NORMS[self.tv_type], self._blocks_maps
                tv = sum(norm(torch.diff(self._bkg_maps, dim=k)).mean() for k in (1, 2))
                tv = tv + norm(torch.diff(bm, dim=2, append=bm[:, :, 0:1])).sum(0).mean() + norm(torch.diff(bm, dim=1)).sum(0).mean()
                tv = tv + sum(norm(torch.diff(self._ground_maps, dim=k)).mean() for k in (1, 2)) * factor
            losses['tv'] = w['tv'] * factor * rs * tv
        if 'overlap' in losses and coarse:
            # (the term is switched off after the coarse phase, dbw.py:390: no samples are drawn then -- the fused and the native path
            # do not draw either, and the ranks' default generators have to stay in lock step)
            u = self._overlap_u_override
            if u is None:
                u = torch.rand(self.n_blocks, OVERLAP_N_POINTS, 3, device=dev)
            ov = ops.overlap_loss(self.sq_eps, self.S, self.R_6d, self.T, self._alpha_full, u, self.ratio_block_scene, self.scale_min,
                                  OVERLAP_TEMPERATURE, OVERLAP_N_BLOCKS)
            losses['overlap'] = w['overlap'] * rs * ov
        losses['total'] = sum(losses.values())
        return losses
