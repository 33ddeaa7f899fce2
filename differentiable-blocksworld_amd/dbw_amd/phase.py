"""The constants of a training phase, derived from the model in ONE place (the reference's rules: src/model/dbw.py:297-334 build_blocks,
361-408 compute_losses), and the conditions under which the decoupled fused training path runs.  The autograd forward (dbw.py), the
launch-by-launch step (native_step.py) and the one-call step (c_step.py) are held to each other by the tests: they take the phase from
here, so that they agree on it by construction."""
from typing import NamedTuple, Optional

from . import ops


class Phase(NamedTuple):
    coarse_epoch: bool              # is_live('coarse_learning'), the epoch alone: the loss factors follow it in eval mode too
    coarse: bool                    # training and coarse_epoch: opacity noise, decimated block maps, the coarse renderer's blocks unfiltered
    decim_env: int                  # decimation of the sky / ground maps
    decim_blocks: int               # ... of the block maps: only while coarse (dbw.py:329-334)
    blocks_decimated: bool          # the in-tile LDS hash and the `_dec` descriptors; else texture bins and the `_all` descriptors
    fine_renderer: bool             # renderer_fine draws the blocks
    noise_scale: float              # std of the opacity noise, 0: none
    mask_threshold: float           # transparency mask on the noise-free opacity (0.5 filter_transparent, 0.01 kill_blocks), -1: none
    masked: bool
    rs: float                       # 1 / world_size: a rank's share of the view-independent terms
    w_rgb: Optional[float]          # the weights as the kernels take them; None: the term is off
    w_parsimony: Optional[float]    # (parsimony and overlap only act while coarse, dbw.py:373-405)
    w_overlap: Optional[float]
    tv_factor: float                # 1 | 0.1 behind the coarse phase, applied once more to the ground map
    w_tv: Optional[float]
    w_tv_ground: Optional[float]
    tv_value_scale: float           # deferred texture gradients: full TV weight in the kernels, the reported value scaled instead
    perceptual_factor: float

    def texture_rows(self):
        """(texture parameter, decimation, wrap_x, tv weight) of the sky, the blocks and the ground, in the order of the kernels' sets."""
        tv, tv_g = self.w_tv or 0.0, self.w_tv_ground or 0.0
        return (('texture_bkg', self.decim_env, 0, tv), ('textures', self.decim_blocks, 1, tv), ('texture_ground', self.decim_env, 0, tv_g))


def late_factor(coarse_epoch):
    """dbw.py:370,378: the TV and the perceptual term count a tenth behind the coarse phase."""
    return 1.0 if coarse_epoch else 0.1


def phase_of(model, training=True, filter_transparent=None, defer=False):
    """filter_transparent: None = the training iteration's (blocks are filtered once the coarse phase is over); defer: the C step's deferred
    texture gradients (c_step.py).  Double arithmetic that ends in `float` kernel arguments: the order of the products is part of the result."""
    w = model.loss_weights
    coarse_epoch = bool(model.is_live('coarse_learning'))
    coarse = bool(training) and coarse_epoch
    decim_env = int(model.decim_factor) if (training and model.is_live('decimate_txt')) else 1
    decim_blocks = decim_env if coarse else 1
    ft = (not coarse) if filter_transparent is None else bool(filter_transparent)
    masked = bool(ft or model.kill_blocks)
    rs = 1.0 / model.world_size
    tv_factor = late_factor(coarse_epoch)
    w_tv = float(w['tv']) * tv_factor * (1.0 if defer else rs) if 'tv' in w else None
    return Phase(coarse_epoch=coarse_epoch, coarse=coarse, decim_env=decim_env, decim_blocks=decim_blocks, blocks_decimated=decim_blocks > 1,
                 fine_renderer=not coarse_epoch, noise_scale=float(model.opacity_noise) if (model.opacity_noise and coarse) else 0.0,
                 mask_threshold=(0.5 if ft else 0.01) if masked else -1.0, masked=masked, rs=rs,
                 w_rgb=float(w['rgb']) if 'rgb' in w else None,
                 w_parsimony=float(w['parsimony']) * rs if ('parsimony' in w and coarse_epoch) else None,
                 w_overlap=float(w['overlap']) * rs if ('overlap' in w and coarse_epoch) else None,
                 tv_factor=tv_factor, w_tv=w_tv, w_tv_ground=None if w_tv is None else w_tv * tv_factor,
                 tv_value_scale=rs if defer else 1.0, perceptual_factor=late_factor(coarse_epoch))


def env_map_desc(model, ph):
    return model._env_map_desc if ph.decim_env == 1 else model._env_map_desc_dec


def block_map_desc(model, ph):
    return model._block_map_desc_dec if ph.blocks_decimated else model._block_map_desc_all


def block_texbins(model, ph, nb):
    """Full-resolution block maps: texel gradients go through the texture-space bins of the first `nb` blocks (coarse phase 8.6 -> 4.2
    ms/step, fine phase 3.1 -> 2.8 ms/step on the bench config); decimated maps use the in-tile LDS hash: None."""
    if ph.blocks_decimated:
        return None
    nbins = nb * model._bins_per_block
    return model._block_bin_base[:nb], model._block_bin_info[:nbins], nbins


def fast_path_refusal(model, renderer=None):
    """-> the first reason why the decoupled fused training path (render + loss epilogue, exp-only uv kernels) cannot run this model, or
    None.  What the model's fused forward, NativeStep and CStep share; each adds what is its own.  renderer: the phase's renderer once the
    cameras are set (its intrinsics are then checked too); default: the configuration alone.  The text is for messages: nothing branches on it."""
    m, r = model, renderer or model.renderer
    if not m.decouple_rendering:
        return 'decouple_rendering is off: one joined scene'
    if 'rgb' not in m.loss_weights:
        return 'no rgb term'
    if not m.default_criteria:
        return f'criteria {m.criterion_name} / {m.tv_type}: the kernels have mse and l2sq'
    if not r.detach_bary:
        return 'detach_bary is off: no uv-fragments'
    if r.faces_per_pixel < 2:
        return 'one face per pixel'
    if r.cam_name != 'perspective' or (renderer is not None and r.cameras.K is None):
        return 'no perspective cameras with intrinsics K'
    if not (m.renderer.clip_inside and m.renderer_fine.clip_inside):
        return 'clip_inside is off: the sigmoid opacity has the generic shading kernels only'
    if not (ops.FUSED_FORWARD and ops.FUSED_BACKWARD and ops.TILED_FRAGMENTS and ops.UV_FRAGMENTS):
        return 'a fused / tiled / uv-fragment kernel is switched off (ops)'
    if m.blocks_n_faces >= (1 << 20) or m.n_blocks + 2 >= (1 << 11):
        return 'too many faces or maps for the packed face | map word'
    if 'surface' in m.loss_weights:
        return 'a surface term'
    if 'freespace' in m.loss_weights:
        return 'a free-space term'
    return None
