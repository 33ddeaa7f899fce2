"""CPU: dbw_amd/phase.py -- the constants of a training phase that the autograd forward, the launch-by-launch step and the one-call step
all take from one record -- against literals worked out from the reference's rules (src/model/dbw.py:297-334 build_blocks, 361-408
compute_losses) for the configuration of tests/test_gpu_c_step.py: 4 blocks, coarse_learning 1500, decimate_txt 750 by 8, kill_blocks,
opacity noise, weights rgb 1 / parsimony 0.01 / tv 0.1 / overlap 1.  And the shared eligibility predicate, one condition at a time."""
import pytest
import torch

import dbw_amd
from dbw_amd import ops, phase as P
from dbw_amd.native_step import NativeStep
from dbw_amd.parallel import FlatParams
from test_gpu_c_step import _cfg


def _model(epoch=0, edit=None, world_size=1):
    cfg = _cfg()
    if edit is not None:
        edit(cfg['model'])
    torch.manual_seed(227391)
    model = dbw_amd.create_model(cfg, (48, 64)).train()
    model.set_cur_epoch(epoch)
    model.world_size = world_size
    return model


def test_coarse_phase_with_decimated_maps():
    m = _model(0)
    ph = P.phase_of(m)
    assert ph.coarse_epoch is True and ph.coarse is True and ph.fine_renderer is False
    assert (ph.decim_env, ph.decim_blocks, ph.blocks_decimated) == (8, 8, True)
    assert (ph.noise_scale, ph.mask_threshold, ph.masked) == (1.0, 0.01, True)
    assert (ph.rs, ph.w_rgb, ph.w_parsimony, ph.w_tv, ph.w_tv_ground, ph.w_overlap) == (1.0, 1.0, 0.01, 0.1, 0.1, 1.0)
    assert (ph.tv_factor, ph.tv_value_scale, ph.perceptual_factor) == (1.0, 1.0, 1.0)
    assert P.block_texbins(m, ph, 4) is None
    assert P.env_map_desc(m, ph) is m._env_map_desc_dec and P.block_map_desc(m, ph) is m._block_map_desc_dec
    assert ph.texture_rows() == (('texture_bkg', 8, 0, 0.1), ('textures', 8, 1, 0.1), ('texture_ground', 8, 0, 0.1))


def test_coarse_phase_with_full_resolution_maps():
    m = _model(800)
    ph = P.phase_of(m)
    assert ph.coarse_epoch is True and ph.coarse is True and ph.fine_renderer is False
    assert (ph.decim_env, ph.decim_blocks, ph.blocks_decimated) == (1, 1, False)
    assert (ph.noise_scale, ph.mask_threshold, ph.masked) == (1.0, 0.01, True)
    assert (ph.w_rgb, ph.w_parsimony, ph.w_tv, ph.w_tv_ground, ph.w_overlap, ph.tv_value_scale) == (1.0, 0.01, 0.1, 0.1, 1.0, 1.0)
    base, info, nbins = P.block_texbins(m, ph, 3)
    assert nbins == 3 * m._bins_per_block and base.shape[0] == 3 and info.shape[0] == nbins
    assert base.data_ptr() == m._block_bin_base.data_ptr() and info.data_ptr() == m._block_bin_info.data_ptr()
    assert P.env_map_desc(m, ph) is m._env_map_desc and P.block_map_desc(m, ph) is m._block_map_desc_all


def test_fine_phase_and_the_roundings_of_its_tv_weights():
    m = _model(1600)
    ph = P.phase_of(m)
    assert ph.coarse_epoch is False and ph.coarse is False and ph.fine_renderer is True
    assert (ph.decim_env, ph.decim_blocks, ph.blocks_decimated) == (1, 1, False)
    assert (ph.noise_scale, ph.mask_threshold, ph.masked) == (0.0, 0.5, True)
    assert ph.w_parsimony is None and ph.w_overlap is None and ph.w_rgb == 1.0
    # 0.1 * 0.1 * 1.0 and that times 0.1 once more, in this order, in doubles: not 0.01 and 0.001
    assert ph.w_tv == 0.010000000000000002 and ph.w_tv_ground == 0.0010000000000000002
    assert ph.tv_factor == 0.1 and ph.perceptual_factor == 0.1
    assert ph.texture_rows() == (('texture_bkg', 1, 0, 0.010000000000000002), ('textures', 1, 1, 0.010000000000000002),
                                 ('texture_ground', 1, 0, 0.0010000000000000002))
    assert P.block_texbins(m, ph, 4) is not None


def test_a_rank_of_two_takes_half_of_the_view_independent_terms():
    m = _model(0, world_size=2)
    ph = P.phase_of(m)
    assert (ph.rs, ph.w_rgb, ph.w_parsimony, ph.w_tv, ph.w_overlap, ph.tv_value_scale) == (0.5, 1.0, 0.005, 0.05, 0.5, 1.0)
    ph = P.phase_of(m, defer=True)          # the TV gradient is added behind the all-reduce: full weight, the reported value halved
    assert (ph.w_tv, ph.w_tv_ground, ph.tv_value_scale, ph.w_parsimony, ph.w_overlap) == (0.1, 0.1, 0.5, 0.005, 0.5)


def test_transparency_threshold():
    def no_kill(c):
        c['rend_optim']['kill_blocks'] = False
    ph = P.phase_of(_model(0, no_kill))
    assert (ph.mask_threshold, ph.masked) == (-1.0, False)
    ph = P.phase_of(_model(1600, no_kill))
    assert (ph.mask_threshold, ph.masked) == (0.5, True)
    for edit in (None, no_kill):
        ph = P.phase_of(_model(0, edit), filter_transparent=True)
        assert (ph.mask_threshold, ph.masked, ph.coarse) == (0.5, True, True)


def test_eval_mode_keeps_the_loss_factors_of_the_epoch():
    m = _model(0).eval()
    ph = P.phase_of(m, training=False)
    assert ph.coarse is False and (ph.decim_env, ph.decim_blocks, ph.blocks_decimated, ph.noise_scale) == (1, 1, False, 0.0)
    assert ph.coarse_epoch is True and ph.fine_renderer is False
    assert (ph.tv_factor, ph.perceptual_factor, ph.w_parsimony, ph.w_tv, ph.w_tv_ground, ph.w_overlap) == (1.0, 1.0, 0.01, 0.1, 0.1, 1.0)


@pytest.mark.parametrize('epoch', [0, 800, 1600])
def test_a_term_without_a_weight_is_off_in_every_phase(epoch):
    def drop(c):
        for k in ('tv_weight', 'parsimony_weight', 'overlap_weight'):
            del c['loss'][k]
    ph = P.phase_of(_model(epoch, drop))
    assert ph.w_parsimony is None and ph.w_tv is None and ph.w_tv_ground is None and ph.w_overlap is None and ph.w_rgb == 1.0
    assert [row[3] for row in ph.texture_rows()] == [0.0, 0.0, 0.0]


def _set(path, value):
    def edit(c):
        node = c
        for k in path[:-1]:
            node = node.setdefault(k, {})
        node[path[-1]] = value
    return edit


def test_fast_path_refusal_one_condition_at_a_time(monkeypatch):
    m = _model(0)
    assert P.fast_path_refusal(m) is None
    for edit in (_set(('renderer', 'detach_bary'), False), _set(('renderer', 'faces_per_pixel'), 1),
                 _set(('rend_optim', 'decouple_rendering'), False), _set(('renderer', 'clip_inside'), False),
                 _set(('loss', 'rgb_weight'), 0), _set(('loss', 'name'), 'l1'), _set(('renderer', 'cameras', 'name'), 'fov')):
        assert isinstance(P.fast_path_refusal(_model(0, edit)), str)
    for r in ('renderer', 'renderer_fine'):          # clip_inside off on either renderer
        m = _model(0)
        getattr(m, r).clip_inside = False
        assert P.fast_path_refusal(m) is not None
    for switch in ('FUSED_FORWARD', 'FUSED_BACKWARD', 'TILED_FRAGMENTS', 'UV_FRAGMENTS'):
        with monkeypatch.context() as mp:
            mp.setattr(ops, switch, False)
            assert P.fast_path_refusal(_model(0)) is not None
    m = _model(0)
    assert P.fast_path_refusal(m) is None
    # with the phase's renderer given, its intrinsics are part of the question: none before the first sample has set them
    assert P.fast_path_refusal(m, m.renderer) is not None
    m.renderer.update_cameras(device='cpu', K=torch.eye(4)[None])
    assert P.fast_path_refusal(m, m.renderer) is None


def test_native_step_adds_sync_free_and_refuses_a_perceptual_weight():
    def step_of(edit=None):
        m = _model(0, edit)
        m.sync_free = True
        return m, NativeStep(m, FlatParams(m))
    m, step = step_of()
    assert step.supported() is True
    m.sync_free = False
    assert step.supported() is False
    assert step_of(_set(('loss', 'perceptual_weight'), 0.1))[1].supported() is False
    assert step_of(_set(('renderer', 'clip_inside'), False))[1].supported() is False
