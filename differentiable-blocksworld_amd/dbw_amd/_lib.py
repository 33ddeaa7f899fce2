"""ctypes binding of libdbw_hip.so (C ABI declared in include/dbw_hip.h).

The library is the product: there is NO CPU fallback.  If it cannot be loaded, or a call fails, a RuntimeError is
raised (never a silent eager/PyTorch path)."""
import collections
import ctypes
import functools
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libdbw_hip.so')
_lib = None


@functools.lru_cache(maxsize=None)
def header_define(header, macro):
    """The integer `#define macro` of include/<header>: the one place a revision or a shared constant is written down (the library returns
    it, the tests and __graft_entry__.build() compare the loaded library with it)."""
    with open(os.path.join(_HERE, '..', '..', 'include', header)) as f:
        return int(re.search(r'#define %s (\d+)' % macro, f.read()).group(1))


ABI_VERSION = header_define('dbw_hip.h', 'DBW_ABI_VERSION')

c_p = ctypes.c_void_p
c_i = ctypes.c_int
c_f = ctypes.c_float
c_i64 = ctypes.c_int64
c_d = ctypes.c_double
c_sz = ctypes.c_size_t



class TextureSet(ctypes.Structure):
    """dbw_texture_set of include/dbw_hip.h (one texture tensor of a multi-set launch)."""
    _fields_ = [('texture', c_p), ('n', c_i), ('h', c_i), ('w', c_i), ('decim', c_i), ('maps', c_p), ('sig', c_p), ('wrap_x', c_i),
                ('tv_scale', c_f), ('grad_sig_out', c_p), ('grad_maps', c_p), ('grad_sig', c_p), ('grad_texture', c_p)]


class StepDesc(ctypes.Structure):
    """dbw_step_desc of include/dbw_hip.h (field order = the header's; tests/test_abi.py compares the two)."""
    _fields_ = ([(n, c_i) for n in ('H', 'W', 'faces_per_pixel', 'max_views', 'n_blocks', 'block_nv', 'block_nf', 'n_sky_verts', 'n_ground_verts',
                                    'n_sky_faces', 'n_ground_faces', 'txt_size', 'env_txt_size', 'decim_env', 'decim_blocks', 'coarse')]
                + [(n, c_f) for n in ('sigma', 'blur_radius', 'z_clip', 'cam_eps')] + [('perspective_correct', c_i)]
                + [('bg_fg', c_f * 3), ('bg_env', c_f * 3)]
                + [(n, c_f) for n in ('S_world', 'ratio_block_scene', 'scale_min', 'opacity_noise', 'mask_threshold', 'w_rgb', 'w_parsimony', 'w_tv_bkg',
                                      'w_tv_blocks', 'w_tv_ground', 'w_overlap')]
                + [('overlap_points', c_i), ('overlap_temperature', c_f), ('overlap_n_blocks', c_f)]
                + [(n, c_p) for n in ('R_world', 'T_world', 'Kmat', 'ground_base', 'env_verts', 'env_faces', 'env_face_uvs', 'env_face_map', 'env_map_desc',
                                      'trig', 'block_faces', 'block_face_uvs', 'block_face_map', 'block_map_desc', 'block_bin_base', 'block_bin_info')]
                + [('n_bins', c_i)]
                + [(n, c_p) for n in ('sq_eps', 'S', 'R6', 'T', 'alpha_logit', 'R6_ground', 'T_ground', 'texture_bkg', 'texture_ground', 'textures',
                                      'g_sq_eps', 'g_S', 'g_R6', 'g_T', 'g_alpha_logit', 'g_R6_ground', 'g_T_ground', 'g_texture_bkg', 'g_texture_ground',
                                      'g_textures', 'flat_param', 'flat_grad', 'exp_avg', 'exp_avg_sq')]
                + [('group_end', c_i64 * 2), ('small_grads', c_p), ('n_small_grads', c_i), ('fuse', c_i), ('backward_order', c_i),
                   ('binned_concurrent', c_i), ('serial_setup_max_views', c_i), ('seed', ctypes.c_uint64), ('sync_events', c_i), ('tv_value_scale', ctypes.c_float)])


class StepInputs(ctypes.Structure):
    """dbw_step_inputs of include/dbw_hip.h."""
    _fields_ = [('imgs', c_p), ('imgs_tiled', c_i), ('R', c_p), ('T', c_p), ('B', c_i), ('global_count', c_d), ('noise_override', c_p),
                ('overlap_u_override', c_p), ('with_adam', c_i), ('adam_step', c_i), ('lr', c_f * 2), ('beta1', c_f), ('beta2', c_f), ('adam_eps', c_f),
                ('read_losses', c_i), ('phase', c_i), ('rec_out', c_p), ('grad_rec', c_p), ('single_stream', c_i), ('arena_is_clean', c_i), ('rng_step', ctypes.c_uint64),
                ('defer_textures', c_i)]


def texture_sets(sets):
    """list of dicts (missing fields = 0 / NULL) -> (ctypes array, count)"""
    arr = (TextureSet * len(sets))()
    for a, d in zip(arr, sets):
        for k, v in d.items():
            setattr(a, k, v)
    return arr, len(sets)


# name -> argtypes, exactly the prototypes of include/dbw_hip.h (checked by tests/test_abi.py)
SIGNATURES = {
    'dbw_project_clip_fwd': [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_f, c_i, c_f, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p],
    'dbw_project_clip_bwd': [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_f, c_f, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p],
    'dbw_rasterize_fwd': [c_p, c_p, c_p, c_p, c_i, c_i64, c_i, c_i, c_i, c_f, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_sz, c_p],
    'dbw_rasterize_bwd': [c_p, c_p, c_p, c_p, c_p, c_i, c_i64, c_i, c_i, c_i, c_i, c_i, c_p, c_p],
    'dbw_shade_blend_fwd': [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p, c_p, c_p],
    'dbw_shade_blend_bwd': [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p,
                            c_p, c_p, c_p, c_p, c_p, c_i, c_p],
    'dbw_render_fwd_fused': [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i64, c_i, c_i, c_i, c_i, c_f, c_f,
                             c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_i, c_i, c_i, c_p],
    'dbw_render_fwd_fused_mse': [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i64, c_i, c_i, c_i, c_i, c_f, c_f,
                                 c_i, c_p, c_p, c_p, c_p, c_p, c_sz, c_p, c_p, c_f, c_p, c_p, c_p, c_i, c_i, c_p],
    'dbw_render_bwd_fused': [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p,
                             c_p, c_p, c_i, c_i, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_p, c_i, c_p, c_i, c_p, c_i, c_p],
    'dbw_texbin_reduce': [c_p, c_p, c_p, c_i, c_p, c_i, c_p, c_p],
    'dbw_bin_layout': [c_p, c_i64, c_d, c_i, c_p, c_p],
    'dbw_texture_prep_fwd': [c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p],
    'dbw_texture_prep_bwd': [c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p],
    'dbw_sq_blocks_fwd': [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_f, c_f, c_f, c_p, c_p, c_p, c_p],
    'dbw_sq_blocks_bwd': [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_f, c_f, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_p],
    'dbw_posed_mesh_fwd': [c_p, c_i, c_p, c_p, c_f, c_p, c_p, c_p, c_p],
    'dbw_posed_mesh_bwd': [c_p, c_i, c_p, c_p, c_f, c_p, c_p, c_p, c_p, c_p],
    'dbw_composite_mse': [c_p, c_p, c_p, c_i, c_i, c_i, c_f, c_p, c_p, c_p, c_p, c_p, c_p],
    'dbw_tv_l2sq': [c_p, c_i, c_i, c_i, c_i, c_f, c_p, c_p, c_p],
    'dbw_overlap_loss': [c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_f, c_f, c_f, c_f, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p],
    'dbw_block_alpha_fwd': [c_p, c_p, c_f, c_f, c_i, c_p, c_p, c_p, c_p],
    'dbw_block_alpha_bwd': [c_p, c_p, c_p, c_i, c_p, c_i, c_p, c_p],
    'dbw_sqrt_mean': [c_p, c_i, c_f, c_f, c_p, c_p, c_p],
    'dbw_adam_step': [c_p, c_p, c_p, c_p, c_i64, c_f, c_f, c_f, c_f, c_i, c_p],
    'dbw_texture_prep_fwd_sets': [c_p, c_i, c_p],
    'dbw_texture_prep_bwd_sets': [c_p, c_i, c_p],
    'dbw_tv_l2sq_sets': [c_p, c_i, c_p, c_p],
    'dbw_adam_step_groups': [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_f, c_f, c_f, c_i, c_p, c_i64, c_p, c_p],
    'dbw_lpips_head_fwd': [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p],
    'dbw_lpips_head_bwd': [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p],
    'dbw_debug_train_step_last_timeout': [c_p, c_p],
    'dbw_debug_train_step_counters': [c_p, c_p, c_p],
    'dbw_bias_relu': [c_p, c_p, c_i, c_i, c_i, c_p, c_p],
    'dbw_maxpool2_fwd': [c_p, c_i, c_i, c_i, c_p, c_p],
    'dbw_maxpool2_bwd': [c_p, c_p, c_i, c_i, c_i, c_p, c_p],
    'dbw_train_step_run': [c_p, c_p, c_p, c_p],
    'dbw_train_step_finish': [c_p, c_p, c_p],
    'dbw_train_step_losses': [c_p, c_p],
    'dbw_train_step_wait_blocks_ready': [c_p, c_p],
    'dbw_train_step_sync_timeouts': [c_p],
    'dbw_debug_train_step_force_timeout': [c_p],
    'dbw_debug_train_step_hasty_prologue_wait': [c_p],
    'dbw_train_step_profile': [c_p, c_i],
    'dbw_train_step_kernel_times': [c_p, c_p],
}
# entry points that do not return an error code: name -> (restype, argtypes)
OTHER_SIGNATURES = {
    'dbw_train_step_workspace_bytes': (c_sz, [c_p]),
    'dbw_train_step_create': (c_p, [c_p, c_p, c_sz]),
    'dbw_train_step_destroy': (None, [c_p]),
    'dbw_train_step_offset': (c_i64, [c_p, c_i]),
    'dbw_train_step_void_flag_offset': (c_i64, [c_p]),
    'dbw_train_step_voided_runs': (c_i, [c_p]),
    'dbw_lpips_head_blocks': (c_i, [c_i, c_i]),
}

# the 3D evaluation entry points: name -> argtypes, exactly the prototypes of include/dbw_eval.h (checked by tests/test_abi_families.py).
# A table of their own: SIGNATURES / OTHER_SIGNATURES stay the prototypes of include/dbw_hip.h.
EVAL_SIGNATURES = {
    'dbw_nn_points': [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p],
    'dbw_dtu_lattice_counts': [c_p, c_i64, c_p, c_p],
    'dbw_dtu_lattice_points': [c_p, c_i64, c_p, c_p, c_i64, c_p, c_p],
    'dbw_radius_downsample_round': [c_p, c_p, c_p, c_i64, c_i64, c_i64, c_d, c_p, c_p, c_p],
    # plane RANSAC (csrc/plane_fit.hip), added under revision 1 of the header
    'dbw_eval_plane_fit': [c_p, c_i64, c_i, c_i, c_f, c_i64, c_p, c_p, c_f, c_p, c_i, c_f, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p],
    # k-means with per-cluster PCA (csrc/cluster_fit.hip), added under revision 1 of the header
    'dbw_eval_cluster_fit': [c_p, c_i64, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p],
    # the surface term (csrc/surface_term.hip), added under revision 1 of the header
    'dbw_eval_surface_fwd': [c_p, c_i64, c_i64, c_i64, c_i64, c_p, c_i, c_p, c_p, c_i, c_p, c_p, c_i, c_p, c_p, c_i, c_d, c_f, c_f, c_i, c_p, c_p, c_p, c_p],
    'dbw_eval_surface_bwd': [c_p, c_i64, c_i64, c_i64, c_i64, c_p, c_i, c_p, c_i, c_i, c_p, c_p, c_i, c_d, c_f, c_f, c_f, c_p, c_i, c_p, c_p, c_p, c_p, c_p],
    # the free-space term (csrc/freespace_term.hip), added under revision 1 of the header
    'dbw_eval_freespace_fwd': [c_p, c_p, c_p, c_i64, c_i, c_i64, c_i64, c_i64, c_p, c_i, c_p, c_p, c_i, c_p, c_p, c_p, c_i, c_p, c_i, c_f, c_f, c_i, c_i, c_p, c_p, c_p,
                               c_p],
    'dbw_eval_freespace_bwd': [c_p, c_p, c_p, c_i64, c_i, c_i64, c_i64, c_i64, c_p, c_i, c_p, c_i, c_i, c_p, c_i, c_f, c_f, c_f, c_p, c_i, c_p, c_p, c_p, c_p, c_p],
}
EVAL_OTHER_SIGNATURES = {
    'dbw_eval_plane_workspace_bytes': (c_sz, [c_i64, c_i]),
    'dbw_eval_cluster_workspace_bytes': (c_sz, [c_i64, c_i]),
    'dbw_eval_surface_workspace_bytes': (c_sz, [c_i64, c_i, c_i, c_i, c_i]),
    'dbw_eval_freespace_workspace_bytes': (c_sz, [c_i64, c_i, c_i, c_i, c_i]),
}
EVAL_SURFACE_SEGMENT = header_define('dbw_eval.h', 'DBW_EVAL_SURFACE_SEGMENT')
EVAL_FREESPACE_SEGMENT = header_define('dbw_eval.h', 'DBW_EVAL_FREESPACE_SEGMENT')
EVAL_PLANE_ORTHOGONAL, EVAL_PLANE_VERTICAL = 0, 1             # DBW_EVAL_PLANE_* of include/dbw_eval.h
EVAL_ABI_VERSION = header_define('dbw_eval.h', 'DBW_EVAL_ABI_VERSION')

# the lit visualisation renders: name -> argtypes, exactly the int-returning prototypes of include/dbw_viz.h (checked by
# tests/test_abi_families.py); the one size_t-returning entry point next to them, like dbw_rasterize_workspace_bytes next to SIGNATURES
VIZ_SIGNATURES = {
    'dbw_vertex_normals': [c_p, c_p, c_p, c_p, c_i, c_i, c_p, c_p],
    'dbw_render_lit_fwd': [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i64, c_i, c_i,
                           c_i, c_i, c_f, c_f, c_i, c_p, c_i, c_p, c_p, c_sz, c_p],
    # scene parsing maps (csrc/scene_parse.hip), added under revision 1 of the header
    'dbw_viz_parse_fwd': [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i64, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p],
}
VIZ_OTHER_SIGNATURES = {
    'dbw_render_lit_workspace_bytes': (c_sz, [c_i64, c_i, c_i, c_i, c_i, c_i]),
    'dbw_viz_parse_workspace_bytes': (c_sz, [c_i64, c_i, c_i, c_i, c_i]),
}
VIZ_MAX_LABELS = header_define('dbw_viz.h', 'DBW_VIZ_MAX_LABELS')
VIZ_NO_LABEL = header_define('dbw_viz.h', 'DBW_VIZ_NO_LABEL')
VIZ_ABI_VERSION = header_define('dbw_viz.h', 'DBW_VIZ_ABI_VERSION')

# the 8-bit frame export: name -> argtypes, exactly the int-returning prototypes of include/dbw_export.h (checked by
# tests/test_abi_families.py).  A table of its own, like the two above.
EXPORT_SIGNATURES = {
    'dbw_frames_u8': [c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p],
}
FRAME_HWC, FRAME_EDGE_FIRST, FRAME_CLAMP_INPUT = 1, 2, 4      # DBW_FRAME_* of include/dbw_export.h
EXPORT_ABI_VERSION = header_define('dbw_export.h', 'DBW_EXPORT_ABI_VERSION')

# the image ingest: name -> argtypes, exactly the int-returning prototypes of include/dbw_ingest.h (checked by tests/test_abi_families.py);
# the one size_t-returning entry point next to them.  dbw_resample_table returns its ksize (> 0) or a negative DBW_ERR_*: not for call().
INGEST_SIGNATURES = {
    'dbw_resample_table': [c_i, c_i, c_p, c_sz],
    'dbw_images_resample_u8': [c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_sz, c_i, c_p],
}
INGEST_OTHER_SIGNATURES = {
    'dbw_images_resample_workspace_bytes': (c_sz, [c_i, c_i, c_i, c_i, c_i]),
}
RESAMPLE_AUTO, RESAMPLE_GENERAL, RESAMPLE_FUSED = 0, 1, 2     # DBW_RESAMPLE_* of include/dbw_ingest.h
INGEST_ABI_VERSION = header_define('dbw_ingest.h', 'DBW_INGEST_ABI_VERSION')

# the camera of a custom capture, its lens and its pose: name -> argtypes, exactly the int-returning prototypes of include/dbw_lens.h (checked by
# tests/test_abi_families.py); the one size_t-returning entry point next to them.
LENS_SIGNATURES = {
    'dbw_images_undistort_u8': [c_p, c_i, c_i, c_i, c_p, c_p, c_p],
    # the validity map of a rectified frame, added under revision 1 of the header
    'dbw_lens_valid_u8': [c_i, c_i, c_p, c_p, c_p],
    # frames with a camera each rectified to one pinhole (csrc/lens_rectify.hip), added under revision 1 of the header
    'dbw_lens_rectify_u8': [c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p],
    'dbw_lens_rectify_valid_u8': [c_i, c_i, c_i, c_p, c_p, c_p, c_p],
    # camera pose refinement (csrc/camera_grad.hip), added under revision 1 of the header
    'dbw_lens_pose_grad': [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_f, c_f, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p, c_p, c_i, c_p],
    'dbw_lens_pose_apply': [c_p, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_p],
    'dbw_lens_pose_chain': [c_p, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_p, c_p],
    # the point cloud of a capture's depth maps (csrc/depth_cloud.hip), added under revision 1 of the header
    'dbw_lens_depth_cloud': [c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_i64, c_p, c_p],
    # the depth rays of a capture (csrc/depth_cloud.hip), added under revision 1 of the header
    'dbw_lens_depth_rays': [c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p],
    # intrinsics refinement (csrc/camera_grad.hip), added under revision 1 of the header
    'dbw_lens_intrinsics_grad': [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_f, c_f, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p, c_i, c_p],
    'dbw_lens_intrinsics_apply': [c_p, c_p, c_p, c_p],
    'dbw_lens_intrinsics_chain': [c_p, c_p, c_p, c_p, c_p],
}
LENS_OTHER_SIGNATURES = {
    'dbw_lens_pose_grad_workspace_bytes': (c_sz, [c_i, c_i]),
    'dbw_lens_intrinsics_grad_workspace_bytes': (c_sz, [c_i, c_i]),
    'dbw_lens_depth_cloud_workspace_bytes': (c_sz, [c_i]),
}
LENS_N_PARAMS = 12                                            # DBW_LENS_N_PARAMS of include/dbw_lens.h
LENS_RECT_N_PARAMS = 16                                       # DBW_LENS_RECT_N_PARAMS
LENS_ABI_VERSION = header_define('dbw_lens.h', 'DBW_LENS_ABI_VERSION')

# the run monitor: name -> argtypes, exactly the int-returning prototypes of include/dbw_monitor.h (checked by tests/test_abi_families.py);
# the one size_t-returning entry point next to them.
MONITOR_SIGNATURES = {
    'dbw_image_scores': [c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p],
    'dbw_meter_add': [c_p, c_p, c_i, c_d, c_i64, c_p],
    'dbw_meter_reset': [c_p, c_i, c_p],
    # SSIM as a loss term (csrc/ssim_term.hip), added under revision 1 of the header
    'dbw_monitor_ssim_term': [c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p],
    # the image terms under a validity mask (csrc/masked_loss.hip, csrc/ssim_term.hip), added under revision 1 of the header
    'dbw_monitor_masked_composite': [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_d, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p],
    'dbw_monitor_masked_ssim_term': [c_p, c_p, c_p, c_i, c_i, c_i, c_d, c_p, c_p, c_p, c_p],
    # the reconstruction term under a per-view exposure (csrc/exposure_loss.hip), added under revision 1 of the header
    'dbw_monitor_exposure_composite': [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_d, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p],
}
MONITOR_OTHER_SIGNATURES = {
    'dbw_image_scores_workspace_bytes': (c_sz, [c_i, c_i, c_i, c_i]),
    'dbw_monitor_ssim_term_workspace_bytes': (c_sz, [c_i, c_i, c_i]),
    'dbw_monitor_masked_composite_workspace_bytes': (c_sz, [c_i, c_i, c_i]),
    'dbw_monitor_masked_ssim_term_workspace_bytes': (c_sz, [c_i, c_i, c_i]),
    'dbw_monitor_exposure_composite_workspace_bytes': (c_sz, [c_i, c_i, c_i]),
}
METER_MAX_VALUES = 16                                         # DBW_METER_MAX_VALUES of include/dbw_monitor.h
MONITOR_ABI_VERSION = header_define('dbw_monitor.h', 'DBW_MONITOR_ABI_VERSION')

# the gradient ICP: name -> argtypes, exactly the int-returning prototypes of include/dbw_icp.h (checked by tests/test_abi_families.py); the one
# size_t-returning entry point next to them.
ICP_SIGNATURES = {
    'dbw_icp_run': [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_d, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p],
}
ICP_OTHER_SIGNATURES = {
    'dbw_icp_workspace_bytes': (c_sz, [c_i, c_i, c_i, c_i]),
}
ICP_TRACE_PER_INSTANCE = 15                                   # DBW_ICP_TRACE_PER_INSTANCE of include/dbw_icp.h
ICP_ABI_VERSION = header_define('dbw_icp.h', 'DBW_ICP_ABI_VERSION')

# the add-on boundaries, one row per header beside include/dbw_hip.h: a new family is a row here and an id of tests/test_abi_families.py.
# `what` completes "the loaded libdbw_hip.so has no ..." of family().
Family = collections.namedtuple('Family', 'header macro version_fn signatures other_signatures what')
FAMILIES = {
    'eval': Family('dbw_eval.h', 'DBW_EVAL_ABI_VERSION', 'dbw_eval_abi_version', EVAL_SIGNATURES, EVAL_OTHER_SIGNATURES, '3D evaluation entry points'),
    'viz': Family('dbw_viz.h', 'DBW_VIZ_ABI_VERSION', 'dbw_viz_abi_version', VIZ_SIGNATURES, VIZ_OTHER_SIGNATURES, 'lit render entry points'),
    'export': Family('dbw_export.h', 'DBW_EXPORT_ABI_VERSION', 'dbw_export_abi_version', EXPORT_SIGNATURES, {}, 'frame export entry point'),
    'ingest': Family('dbw_ingest.h', 'DBW_INGEST_ABI_VERSION', 'dbw_ingest_abi_version', INGEST_SIGNATURES, INGEST_OTHER_SIGNATURES,
                     'image ingest entry point'),
    'lens': Family('dbw_lens.h', 'DBW_LENS_ABI_VERSION', 'dbw_lens_abi_version', LENS_SIGNATURES, LENS_OTHER_SIGNATURES,
                   'lens rectification and pose refinement entry points'),
    'monitor': Family('dbw_monitor.h', 'DBW_MONITOR_ABI_VERSION', 'dbw_monitor_abi_version', MONITOR_SIGNATURES, MONITOR_OTHER_SIGNATURES,
                      'run monitor entry points'),
    'icp': Family('dbw_icp.h', 'DBW_ICP_ABI_VERSION', 'dbw_icp_abi_version', ICP_SIGNATURES, ICP_OTHER_SIGNATURES, 'gradient ICP entry points'),
}


def load():
    """Load (building in-tree with hipcc if the .so is absent or stale and hipcc exists)."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        import importlib.util
        spec = importlib.util.spec_from_file_location('_dbw_build', os.path.join(_HERE, '..', 'build.py'))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        if b.needs_build() and os.path.exists(os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')):
            b.build()
    except Exception as e:                      # a stale-but-present library is still usable; a missing one is fatal below
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f'libdbw_hip.so is missing and could not be built: {e}') from e
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f'{LIB_PATH} not found: run `python differentiable-blocksworld_amd/build.py` '
                           '(there is no CPU fallback for the render path)')
    # DBW_HIP_LIB: load an alternative build of the same sources (tools/variants.sh, kernel tuning sweeps)
    lib = ctypes.CDLL(os.environ.get('DBW_HIP_LIB') or LIB_PATH)
    lib.dbw_last_error.restype = ctypes.c_char_p
    lib.dbw_abi_version.restype = c_i
    if not os.environ.get('DBW_HIP_LIB') and lib.dbw_abi_version() != ABI_VERSION:
        raise RuntimeError(f'{LIB_PATH} was built for ABI {lib.dbw_abi_version()}, include/dbw_hip.h declares {ABI_VERSION}: rebuild '
                           '(python differentiable-blocksworld_amd/build.py --force)')
    if hasattr(lib, 'dbw_bin_subcursors'):      # (absent from tuning builds of older sources, tools/variants.sh: 16 there)
        lib.dbw_bin_subcursors.restype = c_i
    lib.dbw_rasterize_workspace_bytes.restype = c_sz
    lib.dbw_rasterize_workspace_bytes.argtypes = [c_i64]
    lib.dbw_rasterize_workspace_bytes_binned.restype = c_sz
    lib.dbw_rasterize_workspace_bytes_binned.argtypes = [c_i64, c_i, c_i, c_i]
    for name, argtypes in SIGNATURES.items():
        if name.startswith('dbw_train_step') and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = c_i
    for name, (restype, argtypes) in OTHER_SIGNATURES.items():
        if hasattr(lib, name):                  # (absent from tuning builds of older sources)
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argtypes, restype
    for f in FAMILIES.values():
        if not hasattr(lib, f.version_fn):      # (absent from tuning builds of older sources: family() refuses to run on them)
            continue
        getattr(lib, f.version_fn).restype = c_i
        for name, argtypes in f.signatures.items():
            if hasattr(lib, name):              # (a function added under a header's revision is absent from builds of older sources: family() says so)
                fn = getattr(lib, name)
                fn.argtypes = argtypes
                fn.restype = c_i
        for name, (restype, argtypes) in f.other_signatures.items():
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.argtypes, fn.restype = argtypes, restype
    _lib = lib
    return lib


def family(name):
    """The loaded library, once it is known to hold the add-on family `name` of FAMILIES at the revision its header declares.  A library
    without the family still loads (tuning builds of older sources through DBW_HIP_LIB): the refusal comes here, where the family is used."""
    f = FAMILIES[name]
    lib = load()
    if not hasattr(lib, f.version_fn):
        raise RuntimeError(f'the loaded libdbw_hip.so has no {f.what} (include/{f.header}): rebuild it')
    got, want = getattr(lib, f.version_fn)(), header_define(f.header, f.macro)
    if got != want:
        raise RuntimeError(f'the library was built for {name} ABI {got}, include/{f.header} declares {want}: rebuild it')
    # functions added under an unchanged revision: a library that holds some of the family's entry points holds all of them.  The entry
    # points (the int-returning functions of f.signatures) decide: a size query of f.other_signatures is defined in the source of the entry
    # point it sizes the workspace of, so it is there exactly when that entry point is; the message names everything that is absent.
    names = list(f.signatures) + list(f.other_signatures)
    missing = [n for n in names if not hasattr(lib, n)]
    if any(n in f.signatures for n in missing) and len(missing) < len(names):
        raise RuntimeError(f'the loaded libdbw_hip.so has the {name} family of include/{f.header} at revision {got} but not '
                           f'{", ".join(missing)}: it was built from older sources, rebuild it')
    return lib


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RuntimeError(f'{name} failed (rc={rc}): {lib.dbw_last_error().decode()}')
