"""torch.autograd wrappers over the C ABI (include/dbw_hip.h).  PyTorch is plumbing here: device memory, the current
HIP stream and autograd bookkeeping; every arithmetic step of the path is a kernel of libdbw_hip.so.

Operator-level mirrors of what the reference reaches in PyTorch3D:
  rasterize_meshes(...)            <-> pytorch3d.renderer.mesh.rasterize_meshes._C.rasterize_meshes (+ backward)
  render_scene(...)                <-> MeshRasterizer.transform + clip_faces + rasterize + TexturesUV.sample_textures
                                        + layered_rgb_blend (src/model/renderer.py:84-98,219-273)
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib

MAX_FACES_PER_PIXEL = 25
ALPHA_SPREAD = 64          # partial sums per per-map opacity gradient (csrc/shade_common.h: DBW_ALPHA_SPREAD)

def bin_subcursors():
    """Cursors per texture bin of the loaded library (include/dbw_hip.h: DBW_BIN_SUBCURSORS, dbw_bin_subcursors())."""
    lib = _lib.load()
    return int(lib.dbw_bin_subcursors()) if hasattr(lib, 'dbw_bin_subcursors') else 16


def __getattr__(name):             # ops.BIN_SUBCURSORS: the library's value, asked for on first use
    if name == 'BIN_SUBCURSORS':
        return bin_subcursors()
    raise AttributeError(name)

COARSE_BINS = True        # two-level face binning in the rasteriser (64x64-pixel coarse bins); False: every tile scans every face
TEXTURE_BINS = True       # full-resolution texel gradients: bin records by 32x32-texel tile and reduce in LDS (vs 12 atomics/fragment)
UV_FRAGMENTS = True       # detach_bary passes: the forward stores resolved (u, v, face|map) per fragment for the backward
TILED_FRAGMENTS = True    # fused path keeps its fragments in the 8x8-tile planar layout (coalesced); needs both FUSED_* = True
FUSED_FORWARD = True      # one kernel for raster + shade + blend (False: the two operator-level kernels)
FUSED_BACKWARD = True     # one kernel for blend-backward + rasteriser-backward (False: the two operator-level kernels)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


class ZeroArena:
    """Per-step pool of zero-initialised scratch (gradient accumulators, cursors, workspaces).  An iteration used to issue ~30
    `fill` launches of a few microseconds each for them; with the arena enabled they are carved out of one buffer that
    `begin_step()` clears with a single launch.  Opt-in (ShardedTrainStep enables it): a tensor handed out is only valid until
    the next begin_step(), which is safe when the parameters' .grad buffers are preallocated (gradients are accumulated into
    them and nothing of the arena outlives the step) but not for callers that let autograd keep the returned gradient."""

    def __init__(self):
        self.enabled = False
        self.buf, self.off, self.want, self.clean = {}, {}, {}, {}

    def begin_step(self, device):
        if not self.enabled:
            return
        used, want = self.off.get(device, 0), self.want.get(device, 0)
        buf = self.buf.get(device)
        if buf is None or want > buf.numel():
            self.buf[device] = torch.zeros(max(int(want * 1.25), 1 << 20), dtype=torch.uint8, device=device)
        elif used and not self.clean.pop(device, False):
            buf[:used].zero_()
        self.clean.pop(device, None)
        self.off[device], self.want[device] = 0, 0

    def end_step(self, device):
        """-> the part of the arena this step dirtied (or None), for a caller that clears it itself at the END of the step (the fused Adam
        launch does, ops.adam_step_groups_(zero=...)): the next begin_step then issues no fill.  Nothing may take arena memory between
        this call and the next begin_step."""
        device = torch.device(device)
        buf, used = self.buf.get(device), self.off.get(device, 0)
        if not self.enabled or buf is None or not used or self.want.get(device, 0) > buf.numel():
            return None
        self.clean[device] = True
        return buf[:min((used + 15) // 16 * 16, buf.numel())]

    def zeros(self, shape, dtype, device):
        device = torch.device(device)
        if isinstance(shape, int):
            shape = (shape,)
        n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        n_al = (n + 255) & ~255
        if self.enabled:
            self.want[device] = self.want.get(device, 0) + n_al
            buf, off = self.buf.get(device), self.off.get(device, 0)
            if buf is not None and off + n_al <= buf.numel():
                self.off[device] = off + n_al
                return buf[off:off + n].view(dtype).view(shape)
        return torch.zeros(shape, dtype=dtype, device=device)

    def zeros_like(self, t):
        return self.zeros(tuple(t.shape), t.dtype, t.device)


ARENA = ZeroArena()


def _bg_ptr(bg):
    """background colour: HOST pointer to 3 floats (include/dbw_hip.h) -- a ctypes array kept alive by the caller."""
    return 0 if bg is None else ctypes.cast(bg, ctypes.c_void_p).value


def make_bg(color):
    return (ctypes.c_float * 3)(*[float(c) for c in color])


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _chk(t, dtype, name):
    if not t.is_cuda:
        raise RuntimeError(f'{name} must live on the GPU: the dbw_amd render path has no CPU implementation')
    if t.dtype != dtype:
        raise TypeError(f'{name}: expected {dtype}, got {t.dtype}')
    return t.contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# rasterize_meshes  (operator-level drop-in, int64 indices at the Python boundary like PyTorch3D)
# ---------------------------------------------------------------------------------------------------------------------
def _workspace_bytes(Ft, N, H, W):
    lib = _lib.load()
    return lib.dbw_rasterize_workspace_bytes_binned(Ft, N, H, W) if COARSE_BINS else lib.dbw_rasterize_workspace_bytes(Ft)


def _raster_fwd(face_verts, first, num, neighbor, N, H, W, K, blur, pc, cb, cull, need_zbuf=True):
    dev = face_verts.device
    Ft = face_verts.shape[0]
    ws_bytes = _workspace_bytes(Ft, N, H, W)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)
    p2f = torch.empty(N, H, W, K, dtype=torch.int32, device=dev)
    zbuf = torch.empty(N, H, W, K, dtype=torch.float32, device=dev) if need_zbuf else None
    bary = torch.empty(N, H, W, K, 3, dtype=torch.float32, device=dev)
    dists = torch.empty(N, H, W, K, dtype=torch.float32, device=dev)
    _lib.call('dbw_rasterize_fwd', _ptr(face_verts), _ptr(first), _ptr(num), _ptr(neighbor), N, Ft, H, W, K, float(blur),
              int(pc), int(cb), int(cull), _ptr(p2f), _ptr(zbuf), _ptr(bary), _ptr(dists), _ptr(ws), ws_bytes, _stream(face_verts))
    return p2f, zbuf, bary, dists


class _RasterizeMeshes(torch.autograd.Function):
    @staticmethod
    def forward(ctx, face_verts, first, num, neighbor, image_size, blur, K, pc, cb, cull):
        H, W = image_size
        fv = _chk(face_verts.detach(), torch.float32, 'face_verts')
        p2f, zbuf, bary, dists = _raster_fwd(fv, first, num, neighbor, first.numel(), H, W, K, blur, pc, cb, cull)
        ctx.save_for_backward(fv, p2f)
        ctx.cfg = (pc, cb)
        p2f64 = p2f.long()
        ctx.mark_non_differentiable(p2f64)
        return p2f64, zbuf, bary, dists

    @staticmethod
    def backward(ctx, _g, g_zbuf, g_bary, g_dists):
        fv, p2f = ctx.saved_tensors
        pc, cb = ctx.cfg
        N, H, W, K = p2f.shape
        g = torch.zeros_like(fv)
        gz = None if g_zbuf is None else g_zbuf.contiguous()
        gb = None if g_bary is None else g_bary.contiguous()
        gd = None if g_dists is None else g_dists.contiguous()
        _lib.call('dbw_rasterize_bwd', _ptr(fv), _ptr(p2f), _ptr(gz), _ptr(gb), _ptr(gd), N, fv.shape[0], H, W, K, int(pc),
                  int(cb), _ptr(g), _stream(fv))
        return g, None, None, None, None, None, None, None, None, None


def rasterize_meshes(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx, image_size, blur_radius,
                     faces_per_pixel, bin_size=0, max_faces_per_bin=0, perspective_correct=False, clip_barycentric_coords=False,
                     cull_backfaces=False):
    """Positional drop-in for PyTorch3D 0.7.1's `_C.rasterize_meshes` (pytorch3d/renderer/mesh/rasterize_meshes.py; reached by the
    reference through src/model/renderer.py:53-54,92-94): the same twelve arguments in the same order.
    face_verts (F,3,3) packed NDC faces of N meshes -> (pix_to_face int64, zbuf, bary_coords, dists), each (N,H,W,K[,3]), -1 where
    empty; gradients flow to face_verts through zbuf, bary_coords and dists (autograd calls the backward kernel; the stand-alone
    `rasterize_meshes_backward` below is the `_C.rasterize_meshes_backward` twin).
    bin_size / max_faces_per_bin select PyTorch3D's coarse-to-fine CUDA path and size its bins; they never change its result unless a
    bin overflows (which PyTorch3D reports as an error).  This rasteriser has its own two-level binning without capacity limits, so
    both are accepted (None or any int >= 0) and ignored: the result is always the naive rasterisation (bin_size = 0)."""
    if isinstance(image_size, int):
        image_size = (image_size, image_size)
    if bin_size is not None and bin_size < 0:
        raise ValueError('bin_size must be >= 0')
    if max_faces_per_bin is not None and max_faces_per_bin < 0:
        raise ValueError('max_faces_per_bin must be >= 0')
    if faces_per_pixel > MAX_FACES_PER_PIXEL:
        raise ValueError(f'faces_per_pixel={faces_per_pixel} > {MAX_FACES_PER_PIXEL}')
    first = _chk(mesh_to_face_first_idx.to(torch.int32), torch.int32, 'mesh_to_face_first_idx')
    num = _chk(num_faces_per_mesh.to(torch.int32), torch.int32, 'num_faces_per_mesh')
    nb = None if clipped_faces_neighbor_idx is None else _chk(clipped_faces_neighbor_idx.to(torch.int32), torch.int32, 'neighbor')
    return _RasterizeMeshes.apply(face_verts, first, num, nb, tuple(image_size), float(blur_radius), int(faces_per_pixel),
                                  bool(perspective_correct), bool(clip_barycentric_coords), bool(cull_backfaces))


def rasterize_meshes_backward(face_verts, pix_to_face, grad_zbuf, grad_bary, grad_dists, perspective_correct, clip_barycentric_coords):
    """Positional drop-in for PyTorch3D 0.7.1's `_C.rasterize_meshes_backward`: face_verts (F,3,3), pix_to_face (N,H,W,K) int64 (or
    int32), grad_zbuf / grad_dists (N,H,W,K), grad_bary (N,H,W,K,3) -> grad_face_verts (F,3,3)."""
    fv = _chk(face_verts.detach(), torch.float32, 'face_verts')
    p2f = _chk(pix_to_face.to(torch.int32), torch.int32, 'pix_to_face')
    N, H, W, K = p2f.shape
    gz, gb, gd = [_chk(t.detach(), torch.float32, n) for t, n in ((grad_zbuf, 'grad_zbuf'), (grad_bary, 'grad_bary'), (grad_dists, 'grad_dists'))]
    if gz.shape != p2f.shape or gd.shape != p2f.shape or gb.shape != p2f.shape + (3,):
        raise ValueError('gradient shapes must be (N,H,W,K), (N,H,W,K,3), (N,H,W,K)')
    g = torch.zeros_like(fv)
    _lib.call('dbw_rasterize_bwd', _ptr(fv), _ptr(p2f), _ptr(gz), _ptr(gb), _ptr(gd), N, fv.shape[0], H, W, K, int(bool(perspective_correct)),
              int(bool(clip_barycentric_coords)), _ptr(g), _stream(fv))
    return g


# ---------------------------------------------------------------------------------------------------------------------
# project + clip
# ---------------------------------------------------------------------------------------------------------------------
def project_clip(verts, faces_i32, R, T, Kmat, eps=1e-8, z_clip=0.001, perspective_correct=True):
    """-> dict of device tensors (no grad): face_verts (B,2F,3,3), first_idx, num_faces, c2o, neighbor, clip_code, clip_w."""
    dev = verts.device
    B, V, F_ = R.shape[0], verts.shape[0], faces_i32.shape[0]
    out = dict(face_verts=torch.empty(B, 2 * F_, 3, 3, dtype=torch.float32, device=dev),
               first_idx=torch.empty(B, dtype=torch.int32, device=dev), num_faces=torch.empty(B, dtype=torch.int32, device=dev),
               c2o=torch.empty(B, 2 * F_, dtype=torch.int32, device=dev), neighbor=torch.empty(B, 2 * F_, dtype=torch.int32, device=dev),
               clip_code=torch.empty(B, 2 * F_, dtype=torch.int32, device=dev),
               clip_w=torch.empty(B, 2 * F_, 2, dtype=torch.float32, device=dev))
    _lib.call('dbw_project_clip_fwd', _ptr(verts), _ptr(faces_i32), _ptr(R), _ptr(T), _ptr(Kmat), B, V, F_, float(eps),
              int(z_clip is not None), float(z_clip or 0.0), int(perspective_correct), _ptr(out['face_verts']),
              _ptr(out['first_idx']), _ptr(out['num_faces']), _ptr(out['c2o']), _ptr(out['neighbor']), _ptr(out['clip_code']),
              _ptr(out['clip_w']), _stream(verts))
    return out


def project_clip_bwd(verts, faces_i32, R, T, Kmat, cl, g_face_verts, eps=1e-8, z_clip=0.001, perspective_correct=True):
    B, V, F_ = R.shape[0], verts.shape[0], faces_i32.shape[0]
    g = ARENA.zeros_like(verts)
    _lib.call('dbw_project_clip_bwd', _ptr(verts), _ptr(faces_i32), _ptr(R), _ptr(T), _ptr(Kmat), B, V, F_, float(eps),
              float(z_clip or 0.0), int(perspective_correct), _ptr(cl['num_faces']), _ptr(cl['c2o']), _ptr(cl['clip_code']),
              _ptr(cl['clip_w']), _ptr(g_face_verts), _ptr(g), _stream(verts))
    return g


def _camera_grad(fn, outs, accumulate, verts, faces_i32, R, T, Kmat, cl, g_face_verts, eps, z_clip, perspective_correct):
    """The call behind project_clip_bwd_cam and project_clip_bwd_k (csrc/camera_grad.hip): `fn` with its workspace, writing the tensors
    `outs`, or adding to them where `accumulate`."""
    _lib.family('lens')
    B, V, F_ = R.shape[0], verts.shape[0], faces_i32.shape[0]
    ws_bytes = int(getattr(_lib.load(), fn + '_workspace_bytes')(B, F_))
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=verts.device)
    _lib.call(fn, _ptr(verts), _ptr(faces_i32), _ptr(R), _ptr(T), _ptr(Kmat), B, V, F_, float(eps), float(z_clip or 0.0),
              int(perspective_correct), _ptr(cl['num_faces']), _ptr(cl['c2o']), _ptr(cl['clip_code']), _ptr(cl['clip_w']), _ptr(g_face_verts),
              _ptr(ws), ws_bytes, *[_ptr(t) for t in outs], int(accumulate), _stream(verts))


def project_clip_bwd_cam(verts, faces_i32, R, T, Kmat, cl, g_face_verts, eps=1e-8, z_clip=0.001, perspective_correct=True, out=None):
    """dbw_lens_pose_grad: the gradient of the clipped faces with respect to each view's camera, -> (g_R (B,3,3), g_T (B,3)).  The same
    per-slot work as project_clip_bwd, summed over the slots of a view instead of over the views (csrc/camera_grad.hip; fixed summation
    order, no atomics).  out=(g_R, g_T): the sums are ADDED to these (the second pass over the same views) and the pair is returned."""
    B = R.shape[0]
    g_R, g_T = out if out is not None else (torch.empty(B, 3, 3, dtype=torch.float32, device=verts.device),
                                            torch.empty(B, 3, dtype=torch.float32, device=verts.device))
    _camera_grad('dbw_lens_pose_grad', (g_R, g_T), out is not None, verts, faces_i32, R, T, Kmat, cl, g_face_verts, eps, z_clip, perspective_correct)
    return g_R, g_T


def _cam_grads(ctx, iR, g_R, g_T):
    """The entries of a backward's result for R and T: what was asked for of (g_R, g_T)."""
    return (g_R if ctx.needs_input_grad[iR] else None), (g_T if ctx.needs_input_grad[iR + 1] else None)


def project_clip_bwd_k(verts, faces_i32, R, T, Kmat, cl, g_face_verts, eps=1e-8, z_clip=0.001, perspective_correct=True, out=None):
    """dbw_lens_intrinsics_grad: the gradient of the clipped faces with respect to the pinhole matrix the views share, -> g_K (4,4), the full
    gradient of the matrix (row 2, which the projection never reads, is 0).  The per-slot work of project_clip_bwd, summed over the slots of
    every view (csrc/camera_grad.hip; fixed summation order, no atomics).  out=g_K: the sum is ADDED to it (the second pass over the
    same views) and it is returned."""
    g_K = out if out is not None else torch.empty(4, 4, dtype=torch.float32, device=verts.device)
    if R.shape[0] == 0:
        return g_K if out is not None else g_K.zero_()
    _camera_grad('dbw_lens_intrinsics_grad', (g_K,), out is not None, verts, faces_i32, R, T, Kmat, cl, g_face_verts, eps, z_clip, perspective_correct)
    return g_K


# ---------------------------------------------------------------------------------------------------------------------
# shade + blend on given fragments
# ---------------------------------------------------------------------------------------------------------------------
def _alpha_len(faces_alpha, map_desc, F_):
    """alpha_len of the C ABI: F or N*F for per-face opacities, -M for one opacity per texture map (include/dbw_hip.h)."""
    if faces_alpha is None:
        return 0
    n = faces_alpha.numel()
    return -n if (n == map_desc.shape[0] and n != F_) else n


def _shade_args(p2f, bary, dists, cl, face_uvs, face_map, map_desc, maps, faces_alpha, F_, sigma, bg, dims=None):
    N, H, W, K = p2f.shape if dims is None else dims      # dims: explicit (N,H,W,K) when the fragments use the tiled layout
    c2o, code, cw = (cl['c2o'], cl['clip_code'], cl['clip_w']) if cl is not None else (None, None, None)
    return (_ptr(p2f), _ptr(bary), _ptr(dists), _ptr(c2o), _ptr(code), _ptr(cw), 2 * F_, _ptr(face_uvs), _ptr(face_map),
            _ptr(map_desc), _ptr(maps), _ptr(faces_alpha), _alpha_len(faces_alpha, map_desc, F_), N, H, W, K, F_,
            float(sigma), _bg_ptr(bg))


def shade_blend_fwd(p2f, bary, dists, cl, face_uvs, face_map, map_desc, maps, faces_alpha, F_, sigma, bg):
    N, H, W, K = p2f.shape
    img = torch.empty(N, 4, H, W, dtype=torch.float32, device=p2f.device)
    _lib.call('dbw_shade_blend_fwd', *_shade_args(p2f, bary, dists, cl, face_uvs, face_map, map_desc, maps, faces_alpha, F_, sigma, bg),
              _ptr(img), _stream(p2f))
    return img


def shade_blend_bwd(p2f, bary, dists, cl, face_uvs, face_map, map_desc, maps, faces_alpha, F_, sigma, bg, g_img,
                    want_dists=True, want_bary=False, lds_aggregate=False):
    dev = p2f.device
    N, H, W, K = p2f.shape
    g_maps = torch.zeros_like(maps)
    g_alpha = torch.zeros_like(faces_alpha) if faces_alpha is not None else None
    g_dists = torch.empty(N, H, W, K, dtype=torch.float32, device=dev) if want_dists else None
    g_bary = torch.empty(N, H, W, K, 3, dtype=torch.float32, device=dev) if want_bary else None
    _lib.call('dbw_shade_blend_bwd', *_shade_args(p2f, bary, dists, cl, face_uvs, face_map, map_desc, maps, faces_alpha, F_, sigma, bg),
              _ptr(g_img), _ptr(g_maps), _ptr(g_alpha), _ptr(g_dists), _ptr(g_bary), int(lds_aggregate), _stream(p2f))
    return g_maps, g_alpha, g_dists, g_bary


# ---------------------------------------------------------------------------------------------------------------------
# The whole Renderer.forward as ONE autograd node: verts/maps/faces_alpha -> (B,4,H,W)
# ---------------------------------------------------------------------------------------------------------------------
class RenderCfg:
    __slots__ = ('H', 'W', 'K', 'sigma', 'blur', 'z_clip', 'persp', 'detach_bary', 'eps', 'F', 'lds_aggregate', 'texbins', 'const_faces', 'bin_demand')

    def __init__(self, H, W, K, sigma, z_clip, persp, detach_bary, F_, eps=1e-8, lds_aggregate=False, texbins=None, const_faces=0, clip_inside=True):
        self.lds_aggregate = lds_aggregate
        self.const_faces = int(const_faces)   # the first that many faces have constant vertices (sky dome): no geometry gradient for them
        self.texbins = texbins          # (bin_base, bin_info, nbins): texture-space binning of texel gradients when not aggregating
        self.bin_demand = None          # optional BinDemand of the caller (one per pass, kept across steps): record sub-ranges by demand
        # sigma as the library takes it: > 0 exp(-max(d, 0) / sigma), 0 hard, < 0 sigmoid(-d / |sigma|) = clip_inside False (renderer.py:257-258)
        self.H, self.W, self.K, self.sigma, self.z_clip, self.persp = H, W, K, float(sigma) if clip_inside else -float(sigma), z_clip, persp
        self.blur = math.log(1. / 1e-4 - 1.) * float(sigma)            # renderer.py:51
        self.detach_bary, self.eps, self.F = detach_bary, eps, F_


def _all_geometry(cfg, camera_grads):
    """The cfg a pass's backward runs under.  const_faces spares the backward the geometry gradient of faces whose vertices are constants (the
    sky dome): right for the vertex gradient, which nobody reads there -- but a camera or K gradient sums over EVERY face a view shows, and
    the sky moves in the image with the camera like anything else.  With such a gradient asked for, the same cfg without the skip."""
    if not camera_grads or not cfg.const_faces:
        return cfg
    import copy
    full = copy.copy(cfg)
    full.const_faces = 0
    return full


HARD_UV_FRAGMENTS = True  # hard single-layer passes (K = 1, sigma = 0) store (u, v, face|map) per pixel: frag_layout 3


def hard_layout(cfg, fa, map_desc):
    """frag_layout of a fused pass that keeps barycentric fragments by default: 3 for the hard single-layer pass whose backward goes
    through the LDS texel table (include/dbw_hip.h), else 1."""
    ok = (HARD_UV_FRAGMENTS and cfg.K == 1 and cfg.sigma == 0.0 and fa is None and cfg.lds_aggregate and cfg.F < (1 << 20)
          and map_desc.shape[0] < (1 << 11))
    return 3 if ok else 1


def tiled_image_empty(B, C, H, W, device):
    """Uninitialised image in the 8x8-tile planar layout of include/dbw_hip.h (image_layout 1): (B, ceil(H/8), ceil(W/8), C, 64)."""
    return torch.empty(B, (H + 7) // 8, (W + 7) // 8, C, 64, dtype=torch.float32, device=device)


def tile_image(img):
    """(B, C, H, W) -> the 8x8-tile planar layout (B, ceil(H/8), ceil(W/8), C, 64); rows / columns beyond the image are zero."""
    B, C, H, W = img.shape
    ty, tx = (H + 7) // 8, (W + 7) // 8
    if (H, W) != (ty * 8, tx * 8):
        img = torch.nn.functional.pad(img, (0, tx * 8 - W, 0, ty * 8 - H))
    return img.reshape(B, C, ty, 8, tx, 8).permute(0, 2, 4, 1, 3, 5).reshape(B, ty, tx, C, 64).contiguous()      # (reshape: imgs may be a strided view)


def untile_image(t, H, W):
    """Inverse of tile_image: (B, ty, tx, C, 64) -> (B, C, H, W)."""
    B, ty, tx, C, _ = t.shape
    return t.view(B, ty, tx, C, 8, 8).permute(0, 3, 1, 4, 2, 5).reshape(B, C, ty * 8, tx * 8)[:, :, :H, :W].contiguous()


def _render_fwd_fused(fvc, cl, B, cfg, face_uvs, face_map, map_desc, maps, fa, bg, tiled=None, stage=0, state=None, img_tiled=False):
    """stage 1: only the per-face set-up of the pass (needs no texture values) -> `state` for the stage-2 call that renders."""
    TILED_FRAGMENTS = globals()['TILED_FRAGMENTS'] if tiled is None else tiled
    dev = fvc.device
    Ft = fvc.shape[0]
    if stage == 2:
        ws, ws_bytes, out = state
    else:
        ws_bytes = _workspace_bytes(Ft, B, cfg.H, cfg.W)
        ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)
        if TILED_FRAGMENTS:     # internal 8x8-tile planar layouts (include/dbw_hip.h: frag_layout 1, 2, 3)
            ty, tx = (cfg.H + 7) // 8, (cfg.W + 7) // 8
            p2f = torch.empty(B, ty, tx, cfg.K, 64, dtype=torch.int32, device=dev)
            bary = torch.empty(B, ty, tx, cfg.K, 8 if int(TILED_FRAGMENTS) == 2 else 3, 64, dtype=torch.float32, device=dev)
            dists = torch.empty(B, ty, tx, cfg.K, 64, dtype=torch.float32, device=dev)
        else:
            p2f = torch.empty(B, cfg.H, cfg.W, cfg.K, dtype=torch.int32, device=dev)
            bary = torch.empty(B, cfg.H, cfg.W, cfg.K, 3, dtype=torch.float32, device=dev)
            dists = torch.empty(B, cfg.H, cfg.W, cfg.K, dtype=torch.float32, device=dev)
        img = tiled_image_empty(B, 4, cfg.H, cfg.W, dev) if img_tiled else torch.empty(B, 4, cfg.H, cfg.W, dtype=torch.float32, device=dev)
        out = (p2f, bary, dists, img)
    p2f, bary, dists, img = out
    if int(TILED_FRAGMENTS) == 2 and maps.numel() >= (1 << 30):
        raise RuntimeError(f'uv-fragment passes address their texels with 32-bit byte offsets: the maps buffer ({maps.numel()} floats) must hold fewer than 2^30')
    _lib.call('dbw_render_fwd_fused', _ptr(fvc), _ptr(cl['first_idx']), _ptr(cl['num_faces']), _ptr(cl['neighbor']), _ptr(cl['c2o']),
              _ptr(cl['clip_code']), _ptr(cl['clip_w']), 2 * cfg.F, _ptr(face_uvs), _ptr(face_map), _ptr(map_desc), _ptr(maps), _ptr(fa),
              _alpha_len(fa, map_desc, cfg.F), B, Ft, cfg.H, cfg.W, cfg.K, cfg.F, float(cfg.sigma), float(cfg.blur), int(cfg.persp),
              _bg_ptr(bg), _ptr(p2f), _ptr(bary), _ptr(dists), _ptr(img), _ptr(ws), ws_bytes, int(TILED_FRAGMENTS), int(stage),
              int(img_tiled), _stream(fvc))   # frag_layout 0 / 1 / 2
    return (ws, ws_bytes, out) if stage == 1 else out


class _RenderScene(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, maps, faces_alpha, faces_i32, R, T, Kmat, face_uvs, face_map, map_desc, bg, cfg):
        verts_c = _chk(verts.detach(), torch.float32, 'verts')
        maps_c = _chk(maps.detach(), torch.float32, 'maps')
        fa = None if faces_alpha is None else _chk(faces_alpha.detach(), torch.float32, 'faces_alpha')
        B = R.shape[0]
        cl = project_clip(verts_c, faces_i32, R, T, Kmat, cfg.eps, cfg.z_clip, cfg.persp)
        fvc = cl['face_verts'].view(-1, 3, 3)
        ctx.tiled = int(FUSED_FORWARD and FUSED_BACKWARD and TILED_FRAGMENTS)
        if ctx.tiled and UV_FRAGMENTS and cfg.detach_bary and cfg.F < (1 << 20) and map_desc.shape[0] < (1 << 11):
            ctx.tiled = 2          # fragments carry (u, v, face|map) instead of barycentrics
        elif ctx.tiled:
            ctx.tiled = hard_layout(cfg, fa, map_desc)
        if FUSED_FORWARD:
            p2f, bary, dists, img = _render_fwd_fused(fvc, cl, B, cfg, face_uvs, face_map, map_desc, maps_c, fa, bg, ctx.tiled)
        else:
            p2f, _, bary, dists = _raster_fwd(fvc, cl['first_idx'], cl['num_faces'], cl['neighbor'].view(-1), B, cfg.H, cfg.W, cfg.K,
                                              cfg.blur, cfg.persp, True, False, need_zbuf=False)
            img = shade_blend_fwd(p2f, bary, dists, cl, face_uvs, face_map, map_desc, maps_c, fa, cfg.F, cfg.sigma, bg)
        ctx.cfg, ctx.cl = cfg, cl
        ctx.has_alpha = fa is not None
        ctx.bg = bg
        ctx.save_for_backward(verts_c, maps_c, fa if fa is not None else verts_c.new_empty(0), faces_i32, R, T, Kmat, face_uvs,
                              face_map, map_desc, p2f, bary, dists)
        return img

    @staticmethod
    def backward(ctx, g_img):
        verts, maps, fa, faces_i32, R, T, Kmat, face_uvs, face_map, map_desc, p2f, bary, dists = ctx.saved_tensors
        cfg, cl, bg = ctx.cfg, ctx.cl, ctx.bg
        fa = fa if ctx.has_alpha else None
        need_verts = ctx.needs_input_grad[0]
        need_cam = ctx.needs_input_grad[4] or ctx.needs_input_grad[5]        # camera pose refinement: R, T of the views
        need_K = ctx.needs_input_grad[6]                                     # intrinsics refinement: the K they share
        need_geom = need_verts or need_cam or need_K
        want_dists = need_geom and cfg.sigma != 0
        want_bary = need_geom and not cfg.detach_bary
        g_R = g_T = g_K = None
        if FUSED_BACKWARD and (ctx.tiled or (need_geom and (want_dists or want_bary))):
            g_maps, g_alpha, g_fvc = _fused_bwd(p2f, bary, dists, cl, face_uvs, face_map, map_desc, maps, fa, _all_geometry(cfg, need_cam or need_K), bg,
                                                ctx.tiled, g_img.contiguous(), R.shape[0], None)
            g_verts = project_clip_bwd(verts, faces_i32, R, T, Kmat, cl, g_fvc, cfg.eps, cfg.z_clip, cfg.persp) if need_verts else None
            if need_cam:
                g_R, g_T = _cam_grads(ctx, 4, *project_clip_bwd_cam(verts, faces_i32, R, T, Kmat, cl, g_fvc, cfg.eps, cfg.z_clip, cfg.persp))
            if need_K:
                g_K = project_clip_bwd_k(verts, faces_i32, R, T, Kmat, cl, g_fvc, cfg.eps, cfg.z_clip, cfg.persp)
            return g_verts, g_maps, g_alpha, None, g_R, g_T, g_K, None, None, None, None, None
        if ctx.tiled:
            raise RuntimeError('tiled fragments can only be consumed by the fused backward')
        g_maps, g_alpha, g_dists, g_bary = shade_blend_bwd(p2f, bary, dists, cl, face_uvs, face_map, map_desc, maps, fa, cfg.F,
                                                           cfg.sigma, bg, g_img.contiguous(), want_dists, want_bary, cfg.lds_aggregate)
        g_verts = None
        if need_geom and (want_dists or want_bary):
            fvc = cl['face_verts'].view(-1, 3, 3)
            g_fvc = torch.zeros_like(fvc)
            B = R.shape[0]
            _lib.call('dbw_rasterize_bwd', _ptr(fvc), _ptr(p2f), 0, _ptr(g_bary), _ptr(g_dists), B, fvc.shape[0], cfg.H, cfg.W,
                      cfg.K, int(cfg.persp), 1, _ptr(g_fvc), _stream(fvc))
            g_verts = project_clip_bwd(verts, faces_i32, R, T, Kmat, cl, g_fvc, cfg.eps, cfg.z_clip, cfg.persp) if need_verts else None
            if need_cam:
                g_R, g_T = _cam_grads(ctx, 4, *project_clip_bwd_cam(verts, faces_i32, R, T, Kmat, cl, g_fvc, cfg.eps, cfg.z_clip, cfg.persp))
            if need_K:
                g_K = project_clip_bwd_k(verts, faces_i32, R, T, Kmat, cl, g_fvc, cfg.eps, cfg.z_clip, cfg.persp)
        elif need_geom:
            g_verts = torch.zeros_like(verts) if need_verts else None
            if need_cam:
                g_R, g_T = _cam_grads(ctx, 4, torch.zeros_like(R), torch.zeros_like(T))
            if need_K:
                g_K = torch.zeros_like(Kmat)
        return g_verts, g_maps, g_alpha, None, g_R, g_T, g_K, None, None, None, None, None


_UNIFORM_LAYOUTS = {}


def uniform_bin_layout(nbins, cap, device):
    """The layout table of equal shares (include/dbw_hip.h: bin_layout): nbins * cap records divided evenly over the sub-ranges;
    computed once per geometry (dbw_bin_layout on an all-zero demand) and kept."""
    device = torch.device(device)
    key = (nbins, cap, device)
    lay = _UNIFORM_LAYOUTS.get(key)
    if lay is None:
        n = nbins * bin_subcursors()
        lay = torch.zeros(n, 2, dtype=torch.int32, device=device)
        with torch.cuda.device(device):
            _lib.call('dbw_bin_layout', _ptr(torch.zeros(n, dtype=torch.int32, device=device)), n, float(nbins) * float(cap), 1, _ptr(lay),
                      torch.cuda.current_stream(device).cuda_stream)
        _UNIFORM_LAYOUTS[key] = lay
    return lay


class BinDemand:
    """Record sub-ranges of the texture bins sized by demand (include/dbw_hip.h: bin_layout, dbw_bin_layout).  After a backward pass
    bin_cursor holds how many records every sub-range was asked for; a caller that runs the same pass step after step
    (native_step.py) keeps one of these per pass, and the next launch divides the SAME total -- texbin_capacity(...) records per bin on
    average -- in proportion to that demand (+ 25 %, at least MIN records each) instead of in equal shares.  One small kernel on the
    device, no host read, the record buffer keeps its size.  With equal shares the hot bins of a large scene overflow into the atomic
    fallback: config 5's backward took 56 ms at full resolution, 9.6 ms with four times the memory.
    Two cursor arrays are kept and used in turn (this launch's cursors are the next launch's demand); they are never reallocated, so a
    captured hipGraph that replays one launch keeps reading a valid -- if frozen -- demand."""
    MIN = 64

    def __init__(self):
        self.key, self.cursors, self.layouts, self.turn, self.ready = None, None, None, 0, False

    def _fit(self, nbins, device):
        n = nbins * bin_subcursors()
        if self.key != (n, device):
            self.key = (n, device)
            self.cursors = [torch.zeros(n, dtype=torch.int32, device=device) for _ in range(2)]
            self.layouts = [torch.zeros(n, 2, dtype=torch.int32, device=device) for _ in range(2)]
            self.turn, self.ready = 0, False
        return n

    def prepare(self, nbins, cap, device):
        """Enqueue, on the current stream, the layout of the NEXT launch from the cursors of the previous one (call it early in the
        step, off the critical path; begin() does it itself otherwise)."""
        n = self._fit(nbins, device)
        if not self.ready:
            return None
        lay = self.layouts[self.turn]
        _lib.call('dbw_bin_layout', _ptr(self.cursors[1 - self.turn]), n, float(nbins) * float(cap), self.MIN, _ptr(lay),
                  torch.cuda.current_stream(device).cuda_stream)
        self.prepared = (nbins, cap, lay)
        return lay

    def begin(self, nbins, cap, device):
        """-> (zeroed cursors of this launch, layout or None for the first launch / after a change of geometry)."""
        self._fit(nbins, device)
        lay = None
        if self.ready:
            pre = getattr(self, 'prepared', None)
            lay = pre[2] if (pre is not None and pre[:2] == (nbins, cap) and pre[2] is self.layouts[self.turn]) else self.prepare(nbins, cap, device)
        self.prepared = None
        cur = self.cursors[self.turn]
        cur.zero_()
        self.turn, self.ready = 1 - self.turn, True
        return cur, lay


def _fused_bwd(p2f, bary, dists, cl, face_uvs, face_map, map_desc, maps, fa, cfg, bg, tiled, g_img, B, gscale, after_kernel=None, img_tiled=False,
               bin_demand=None):
    """dbw_render_bwd_fused (+ dbw_texbin_reduce when the texel gradients go through texture-space bins) of one pass.
    gscale: device scalar multiplying g_img inside the kernel (or None).  -> grad maps, grad faces_alpha (or None), grad face_verts_c.
    bin_demand: a BinDemand kept by the caller across steps -> the bins' record sub-ranges follow the previous step's demand."""
    fvc = cl['face_verts'].view(-1, 3, 3)
    per_map = fa is not None and _alpha_len(fa, map_desc, cfg.F) < 0        # then 64 partial sums per opacity (include/dbw_hip.h)
    g_maps = ARENA.zeros_like(maps)
    g_alpha = None if fa is None else (ARENA.zeros(fa.numel() * ALPHA_SPREAD, torch.float32, fa.device) if per_map else ARENA.zeros_like(fa))
    g_fvc = ARENA.zeros_like(fvc)
    bins = cfg.texbins if (TEXTURE_BINS and not cfg.lds_aggregate) else None
    bin_base = cursor = records = layout = None
    cap = 0
    if bins is not None and bins[2] > 0:
        bin_base, bin_info, nbins = bins
        cap = texbin_capacity(B, cfg.H, cfg.W, cfg.K, nbins)
        if bin_demand is None:
            bin_demand = cfg.bin_demand
        if bin_demand is not None:
            cursor, layout = bin_demand.begin(nbins, cap, fvc.device)
        else:
            cursor = ARENA.zeros(nbins * bin_subcursors(), torch.int32, fvc.device)
        if layout is None:
            layout = uniform_bin_layout(nbins, cap, fvc.device)         # (first launch, or a caller that keeps no demand: equal shares)
        records = torch.empty(nbins * cap * 8, dtype=torch.int32, device=fvc.device)
    _lib.call('dbw_render_bwd_fused', *_shade_args(p2f, bary, dists, cl, face_uvs, face_map, map_desc, maps, fa, cfg.F, cfg.sigma, bg,
                                                   (B, cfg.H, cfg.W, cfg.K)),
              _ptr(g_img), _ptr(fvc), int(cfg.persp), int(cfg.detach_bary), _ptr(g_maps), _ptr(g_alpha), _ptr(g_fvc),
              int(cfg.lds_aggregate), int(tiled), _ptr(bin_base), _ptr(cursor), _ptr(records), cap, _ptr(layout), int(cfg.const_faces),
              _ptr(gscale), int(img_tiled), _stream(fvc))
    if after_kernel is not None:
        after_kernel()            # (the big kernel is enqueued; the bin reduction, a low-occupancy kernel, may share the GPU with other work)
    if records is not None:
        _lib.call('dbw_texbin_reduce', _ptr(bin_info), _ptr(cursor), _ptr(records), cap, _ptr(layout), nbins, _ptr(g_maps), _stream(fvc))
    return g_maps, g_alpha, g_fvc


def render_fwd_fused_mse(cl, B, cfg, face_uvs, face_map, map_desc, maps, fa, bg, env_img, imgs, scale, stage=0, state=None, img_tiled=False):
    """dbw_render_fwd_fused_mse on the clipped faces `cl` of the fg scene (no grad bookkeeping): uv-fragments + per-tile sums of
    squared differences + d loss / d fg image, d loss / d env image.  -> p2f, bary, dists, part, g_fg, g_env.
    stage 1 (env_img / imgs may be None): only the per-face set-up, on the current stream -> `state` for the stage-2 call that
    renders (the caller orders the two calls)."""
    fvc = cl['face_verts'].view(-1, 3, 3)
    dev, Ft = fvc.device, fvc.shape[0]
    if stage == 2:
        ws, ws_bytes, out = state
    else:
        ws_bytes = _workspace_bytes(Ft, B, cfg.H, cfg.W)
        ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)
        ty, tx = (cfg.H + 7) // 8, (cfg.W + 7) // 8
        p2f = torch.empty(B, ty, tx, cfg.K, 64, dtype=torch.int32, device=dev)
        bary = torch.empty(B, ty, tx, cfg.K, 8, 64, dtype=torch.float32, device=dev)
        dists = torch.empty(B, ty, tx, cfg.K, 64, dtype=torch.float32, device=dev)
        part = torch.empty(B * ty * tx, dtype=torch.float32, device=dev)
        g_fg = tiled_image_empty(B, 4, cfg.H, cfg.W, dev) if img_tiled else torch.empty(B, 4, cfg.H, cfg.W, dtype=torch.float32, device=dev)
        g_env = torch.empty_like(g_fg)
        out = (p2f, bary, dists, part, g_fg, g_env)
    p2f, bary, dists, part, g_fg, g_env = out
    if maps.numel() >= (1 << 30):
        raise RuntimeError(f'uv-fragment passes address their texels with 32-bit byte offsets: the maps buffer ({maps.numel()} floats) must hold fewer than 2^30')
    _lib.call('dbw_render_fwd_fused_mse', _ptr(fvc), _ptr(cl['first_idx']), _ptr(cl['num_faces']), _ptr(cl['neighbor']), _ptr(cl['c2o']),
              _ptr(cl['clip_code']), _ptr(cl['clip_w']), 2 * cfg.F, _ptr(face_uvs), _ptr(face_map), _ptr(map_desc), _ptr(maps), _ptr(fa),
              _alpha_len(fa, map_desc, cfg.F), B, Ft, cfg.H, cfg.W, cfg.K, cfg.F, float(cfg.sigma), float(cfg.blur), int(cfg.persp),
              _bg_ptr(bg), _ptr(p2f), _ptr(bary), _ptr(dists), _ptr(ws), ws_bytes, _ptr(env_img), _ptr(imgs), float(scale), _ptr(part),
              _ptr(g_fg), _ptr(g_env), int(stage), int(img_tiled), _stream(fvc))
    return (ws, ws_bytes, out) if stage == 1 else out


class _DecoupledRenderMSE(torch.autograd.Function):
    """The whole decoupled training render + reconstruction loss (dbw.py:213-223,366-367) as ONE autograd node:
    env pass (sky + ground, hard, 1 face per pixel) -> fg pass (blocks, soft, K faces per pixel) whose epilogue composites over the
    env image and takes the MSE against the targets on registers (dbw_render_fwd_fused_mse) -> scalar loss.  Neither the fg image
    nor the composite ever exists in memory; the two backward passes read the per-pixel loss gradients the forward left behind,
    scaled inside the kernels by the upstream gradient (a device scalar: no host sync, no elementwise pass)."""

    @staticmethod
    def forward(ctx, verts_e, maps_e, verts_f, maps_f, alpha, imgs, scale, R, T, Kmat, env_tab, fg_tab, cfg_e, cfg_f, bg_e, bg_f):
        ve, me = _chk(verts_e.detach(), torch.float32, 'env verts'), _chk(maps_e.detach(), torch.float32, 'env maps')
        vf, mf = _chk(verts_f.detach(), torch.float32, 'fg verts'), _chk(maps_f.detach(), torch.float32, 'fg maps')
        fa = None if alpha is None else _chk(alpha.detach(), torch.float32, 'faces_alpha')
        imgs = _chk(imgs, torch.float32, 'imgs')
        faces_e, uv_e, fmap_e, desc_e = env_tab
        faces_f, uv_f, fmap_f, desc_f = fg_tab
        B, dev = R.shape[0], ve.device
        # env pass: barycentric fragments (layout 1), image kept (the fg epilogue reads it)
        cl_e = project_clip(ve, faces_e, R, T, Kmat, cfg_e.eps, cfg_e.z_clip, cfg_e.persp)
        lay_e = ctx.lay_e = hard_layout(cfg_e, None, desc_e)
        p2f_e, bary_e, dists_e, img_e = _render_fwd_fused(cl_e['face_verts'].view(-1, 3, 3), cl_e, B, cfg_e, uv_e, fmap_e, desc_e, me, None, bg_e, lay_e)
        # fg pass with the composite + MSE epilogue
        cl_f = project_clip(vf, faces_f, R, T, Kmat, cfg_f.eps, cfg_f.z_clip, cfg_f.persp)
        p2f, bary, dists, part, g_fg, g_env = render_fwd_fused_mse(cl_f, B, cfg_f, uv_f, fmap_f, desc_f, mf, fa, bg_f, img_e, imgs, scale)
        ctx.save_for_backward(ve, me, vf, mf, fa if fa is not None else ve.new_empty(0), R, T, Kmat, p2f_e, bary_e, dists_e, p2f, bary, dists, g_fg, g_env)
        ctx.misc = (env_tab, fg_tab, cfg_e, cfg_f, bg_e, bg_f, cl_e, cl_f, fa is not None)
        return part.sum() * float(scale)

    @staticmethod
    def backward(ctx, go):
        ve, me, vf, mf, fa, R, T, Kmat, p2f_e, bary_e, dists_e, p2f, bary, dists, g_fg, g_env = ctx.saved_tensors
        env_tab, fg_tab, cfg_e, cfg_f, bg_e, bg_f, cl_e, cl_f, has_alpha = ctx.misc
        ctx.misc = None
        fa = fa if has_alpha else None
        faces_e, uv_e, fmap_e, desc_e = env_tab
        faces_f, uv_f, fmap_f, desc_f = fg_tab
        B = R.shape[0]
        gs = go.detach().to(torch.float32).reshape(1).contiguous()
        gm_f, ga, g_fvc_f = _fused_bwd(p2f, bary, dists, cl_f, uv_f, fmap_f, desc_f, mf, fa, cfg_f, bg_f, 2, g_fg, B, gs)
        gv_f = project_clip_bwd(vf, faces_f, R, T, Kmat, cl_f, g_fvc_f, cfg_f.eps, cfg_f.z_clip, cfg_f.persp) if ctx.needs_input_grad[2] else None
        need_cam = ctx.needs_input_grad[7] or ctx.needs_input_grad[8] or ctx.needs_input_grad[9]
        gm_e, _, g_fvc_e = _fused_bwd(p2f_e, bary_e, dists_e, cl_e, uv_e, fmap_e, desc_e, me, None, _all_geometry(cfg_e, need_cam), bg_e, ctx.lay_e, g_env, B, gs)
        gv_e = project_clip_bwd(ve, faces_e, R, T, Kmat, cl_e, g_fvc_e, cfg_e.eps, cfg_e.z_clip, cfg_e.persp) if ctx.needs_input_grad[0] else None
        g_R = g_T = None
        if ctx.needs_input_grad[7] or ctx.needs_input_grad[8]:
            # camera pose refinement: env then fg into one pair of buffers, so that the order of the sum is fixed
            cam = project_clip_bwd_cam(ve, faces_e, R, T, Kmat, cl_e, g_fvc_e, cfg_e.eps, cfg_e.z_clip, cfg_e.persp)
            cam = project_clip_bwd_cam(vf, faces_f, R, T, Kmat, cl_f, g_fvc_f, cfg_f.eps, cfg_f.z_clip, cfg_f.persp, out=cam)
            g_R, g_T = _cam_grads(ctx, 7, *cam)
        g_K = None
        if ctx.needs_input_grad[9]:
            # intrinsics refinement: env then fg into one buffer, like the pair above
            g_K = project_clip_bwd_k(ve, faces_e, R, T, Kmat, cl_e, g_fvc_e, cfg_e.eps, cfg_e.z_clip, cfg_e.persp)
            g_K = project_clip_bwd_k(vf, faces_f, R, T, Kmat, cl_f, g_fvc_f, cfg_f.eps, cfg_f.z_clip, cfg_f.persp, out=g_K)
        return (gv_e, gm_e, gv_f, gm_f, ga, None, None, g_R, g_T, g_K) + (None,) * 6


def render_decoupled_mse(env, fg, alpha, imgs, scale, R, T, Kmat, cfg_e, cfg_f, bg_e, bg_f):
    """env / fg: PackedScene-like (verts, maps, faces, face_uvs, face_map, map_desc); alpha: per-face opacities of fg or None;
    -> scale * sum((imgs - (fg_rgb * mask + (1 - mask) * env_rgb))^2) as a scalar tensor (scale = weight / element count)."""
    if cfg_f.K < 2 or not cfg_f.detach_bary or cfg_e.K != 1:
        raise ValueError('render_decoupled_mse: soft detach_bary fg pass over a hard single-layer env pass')
    return _DecoupledRenderMSE.apply(env.verts, env.maps, fg.verts, fg.maps, alpha, imgs, float(scale), R, T, Kmat,
                                     (env.faces, env.face_uvs, env.face_map, env.map_desc), (fg.faces, fg.face_uvs, fg.face_map, fg.map_desc),
                                     cfg_e, cfg_f, bg_e, bg_f)


def texbin_capacity(B, H, W, K, nbins):
    """Records per texture bin: room for max(K/2, 2) fragments per pixel spread evenly over the bins (a soft K-layer render
    fills ~20 % of its slots, a hard 1-layer render all of them; what does not fit falls back to atomics), at most 16 GiB
    of the 288 GB (config 5 -- 25 views of 1080x1920, K = 16 -- asks for 13 GB)."""
    import os
    cap = int(min(max(int(float(os.environ.get('DBW_CAP_SCALE', 1)) * B * H * W * max(K, 4)) // (2 * nbins), 256), (16 << 30) // (32 * nbins)))
    sub = bin_subcursors()
    return (cap + sub - 1) // sub * sub          # a bin's range = DBW_BIN_SUBCURSORS equal sub-ranges


def render_scene(verts, maps, faces_alpha, faces_i32, R, T, Kmat, face_uvs, face_map, map_desc, bg, cfg):
    """verts (V,3) world, maps flat fp32, faces_alpha None | (F,) | (B*F,) -> image (B,4,H,W)."""
    if cfg.K > MAX_FACES_PER_PIXEL:
        raise ValueError(f'faces_per_pixel={cfg.K} > {MAX_FACES_PER_PIXEL}')
    return _RenderScene.apply(verts, maps, faces_alpha, faces_i32, R, T, Kmat, face_uvs, face_map, map_desc, bg, cfg)


def render_fragments(verts, faces_i32, R, T, Kmat, cfg):
    """Debug/parity helper (no grad): the raw fragments of a render pass, in clipped indexing + the clip tables."""
    cl = project_clip(verts, faces_i32, R, T, Kmat, cfg.eps, cfg.z_clip, cfg.persp)
    fvc = cl['face_verts'].view(-1, 3, 3)
    p2f, zbuf, bary, dists = _raster_fwd(fvc, cl['first_idx'], cl['num_faces'], cl['neighbor'].view(-1), R.shape[0], cfg.H, cfg.W,
                                         cfg.K, cfg.blur, cfg.persp, True, False, need_zbuf=True)
    return cl, p2f, zbuf, bary, dists


# ---------------------------------------------------------------------------------------------------------------------
# lit visualisation renders (include/dbw_viz.h): directional light, flat / Phong shading, forward only
# ---------------------------------------------------------------------------------------------------------------------
def vertex_adjacency(faces_i32, V):
    """CSR vertex -> (face, corner) adjacency of dbw_vertex_normals: (adj_start (V+1,) int32, adj (3F,) int32 entries face * 4 + corner), a
    vertex's entries in ascending (face, corner) order.  Integer plumbing, built once per topology."""
    flat = faces_i32.reshape(-1).long()
    order = torch.argsort(flat, stable=True)              # entry e = face * 3 + corner
    adj = (torch.div(order, 3, rounding_mode='floor') * 4 + order % 3).to(torch.int32).contiguous()
    start = torch.zeros(V + 1, dtype=torch.int64, device=faces_i32.device)
    start[1:] = torch.cumsum(torch.bincount(flat, minlength=V)[:V], 0)
    return start.to(torch.int32).contiguous(), adj


def _viz_lib():
    return _lib.family('viz')


def vertex_normals(verts, faces_i32, adjacency=None):
    """(V,3) area-weighted unit vertex normals (PyTorch3D's verts_normals_packed) of a packed scene; no grad."""
    _viz_lib()
    verts_c = _chk(verts.detach(), torch.float32, 'verts')
    faces_c = _chk(faces_i32, torch.int32, 'faces')
    V, F_ = verts_c.shape[0], faces_c.shape[0]
    start, adj = adjacency if adjacency is not None else vertex_adjacency(faces_c, V)
    out = torch.empty(V, 3, dtype=torch.float32, device=verts_c.device)
    _lib.call('dbw_vertex_normals', _ptr(verts_c), _ptr(faces_c), _ptr(start), _ptr(adj), V, F_, _ptr(out), _stream(verts_c))
    return out


def light_dir_world(direction, R):
    """The light is fixed to the camera (renderer.py:87-89): direction (1 | B, 3) @ R[b]^T -> (B,3), element-wise so that a view's
    direction does not depend on the batch it is rendered in."""
    d = direction.to(device=R.device, dtype=torch.float32).reshape(-1, 3)
    return (d[:, 0:1] * R[:, :, 0] + d[:, 1:2] * R[:, :, 1] + d[:, 2:3] * R[:, :, 2]).contiguous()


def render_scene_lit(verts, maps, faces_alpha, faces_i32, R, T, Kmat, face_uvs, face_map, map_desc, bg, cfg, direction, ambient, diffuse,
                     phong=False, ssaa=1, adjacency=None):
    """The lit render pass (include/dbw_viz.h: dbw_render_lit_fwd): colour = (ambient + diffuse * relu(n . d)) * texel, layered blend,
    with ssaa == 4 rendered at 4x cfg.H x cfg.W and box-filtered in the kernel.  -> image (B,4,cfg.H,cfg.W).  direction (1 | B, 3): towards
    the light, camera space; ambient / diffuse: three floats each.  Forward only: there is no autograd node."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (verts, maps, faces_alpha)):
        raise NotImplementedError('render_scene_lit is forward only (the reference calls its lit renderers under no_grad): a differentiable '
                                  'lit pass does not exist; call it under torch.no_grad() or detach the inputs')
    if cfg.K > MAX_FACES_PER_PIXEL:
        raise ValueError(f'faces_per_pixel={cfg.K} > {MAX_FACES_PER_PIXEL}')
    if ssaa not in (1, 4):
        raise ValueError(f'ssaa must be 1 or 4, got {ssaa}')
    if ssaa == 4 and cfg.K != 1:
        raise NotImplementedError('ssaa=4 resolves its 4x4 blocks inside the single-layer kernel: faces_per_pixel must be 1')
    lib = _viz_lib()
    verts_c = _chk(verts.detach(), torch.float32, 'verts')
    maps_c = _chk(maps.detach(), torch.float32, 'maps')
    fa = None if faces_alpha is None else _chk(faces_alpha.detach(), torch.float32, 'faces_alpha')
    dev = verts_c.device
    B = R.shape[0]
    normals = vertex_normals(verts_c, faces_i32, adjacency) if phong else None
    ldir = light_dir_world(direction, R)
    cl = project_clip(verts_c, faces_i32, R, T, Kmat, cfg.eps, cfg.z_clip, cfg.persp)
    fvc = cl['face_verts'].view(-1, 3, 3)
    Ft = fvc.shape[0]
    ws_bytes = lib.dbw_render_lit_workspace_bytes(Ft, B, cfg.F, cfg.H, cfg.W, ssaa)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)
    img = torch.empty(B, 4, cfg.H, cfg.W, dtype=torch.float32, device=dev)
    ka, kd = make_bg(ambient), make_bg(diffuse)
    _lib.call('dbw_render_lit_fwd', _ptr(fvc), _ptr(cl['first_idx']), _ptr(cl['num_faces']), _ptr(cl['neighbor']), _ptr(cl['c2o']),
              _ptr(cl['clip_code']), _ptr(cl['clip_w']), 2 * cfg.F, _ptr(face_uvs), _ptr(face_map), _ptr(map_desc), _ptr(maps_c), _ptr(fa),
              _alpha_len(fa, map_desc, cfg.F), _ptr(verts_c), _ptr(faces_i32), _ptr(normals), _ptr(ldir), _bg_ptr(ka), _bg_ptr(kd), B, Ft,
              cfg.H, cfg.W, cfg.K, cfg.F, float(cfg.sigma), float(cfg.blur), int(cfg.persp), _bg_ptr(bg), int(ssaa), _ptr(img), _ptr(ws),
              ws_bytes, _stream(verts_c))
    return img


def parse_scene(verts, faces_i32, face_label, R, T, Kmat, cfg):
    """Scene parsing maps of a packed scene for the len(R) views (include/dbw_viz.h: dbw_viz_parse_fwd), hard rasterisation at cfg.H x
    cfg.W (cfg.K, cfg.sigma and cfg.blur are not looked at), no grad.  face_label: one label in [0, 64) per face of the scene.
    -> label (B,H,W) uint8: label of the nearest face, 255 where there is none; depth (B,H,W) fp32: its view-space z, -1 where there is
    none; cover (B,H,W) int64: bit l set where some face with label l covers the pixel, occluded or not; counts (B,64,2) int32: per view and
    label [amodal area, visible area] in pixels.

    Who checks the labels: a `face_label` on the CPU (a tensor or a sequence: the usual case, parse_views builds its table there) is handed to
    the library as the host copy it validates before any launch, and uploaded; a tensor on the GPU is taken as it is -- its builder vouches
    for it (the kernel folds a label into [0, 64), so a bad table gives wrong maps, never a wild access) -- and is never read back."""
    lib = _viz_lib()
    verts_c = _chk(verts.detach(), torch.float32, 'verts')
    faces_c = _chk(faces_i32, torch.int32, 'faces')
    dev = verts_c.device
    B, F_ = R.shape[0], faces_c.shape[0]
    host = None
    if not (torch.is_tensor(face_label) and face_label.is_cuda):
        host = torch.as_tensor(face_label).to(torch.int32).reshape(-1).contiguous()
        lab = host.to(dev)
    else:
        lab = _chk(face_label, torch.int32, 'face_label').reshape(-1)
    if lab.numel() != F_:
        raise ValueError(f'face_label has {lab.numel()} entries for {F_} faces')
    cl = project_clip(verts_c, faces_c, R, T, Kmat, cfg.eps, cfg.z_clip, cfg.persp)
    fvc = cl['face_verts'].view(-1, 3, 3)
    Ft = fvc.shape[0]
    ws_bytes = lib.dbw_viz_parse_workspace_bytes(Ft, B, F_, cfg.H, cfg.W)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)
    label = torch.empty(B, cfg.H, cfg.W, dtype=torch.uint8, device=dev)
    depth = torch.empty(B, cfg.H, cfg.W, dtype=torch.float32, device=dev)
    cover = torch.empty(B, cfg.H, cfg.W, dtype=torch.int64, device=dev)
    counts = torch.empty(B, _lib.VIZ_MAX_LABELS, 2, dtype=torch.int32, device=dev)
    _lib.call('dbw_viz_parse_fwd', _ptr(fvc), _ptr(cl['first_idx']), _ptr(cl['num_faces']), _ptr(cl['neighbor']), _ptr(cl['c2o']), 2 * F_, B, Ft,
              cfg.H, cfg.W, F_, int(cfg.persp), _ptr(lab), _ptr(host), _ptr(label), _ptr(depth), _ptr(cover), _ptr(counts), _ptr(ws), ws_bytes,
              _stream(verts_c))
    return label, depth, cover, counts


# ---------------------------------------------------------------------------------------------------------------------
# 8-bit frame export (include/dbw_export.h)
# ---------------------------------------------------------------------------------------------------------------------
def frames_u8(src, bkg=None, mask=None, edge_color=None, hwc=False, edge_first=False, clamp_input=False, out=None):
    """dbw_frames_u8: fp32 frames on the GPU -> (N,H,W,3) uint8 on the GPU, as the reference's convert_to_img quantises (clamp to [0, 1],
    times 255, truncate).  src (N,C,H,W), C = 3 or 4 -- or (N,H,W,3) with hwc, the layout of the prepared texture maps.  bkg: three floats
    or a (3,H,W) tensor, composited under a C = 4 source (premultiplied rgb: rgb * alpha + (1 - alpha) * bkg).  mask (N,1,H,W) with
    edge_color three floats or (N,3,H,W): img * (1 - mask) + mask * colour, behind the composite, or in front of it with edge_first.
    clamp_input clamps the source channels to [0, 1] first.  out: an (N,H,W,3) uint8 GPU tensor to fill."""
    lib = _lib.family('export')
    src_c = _chk(src, torch.float32, 'src')
    if src_c.dim() != 4:
        raise ValueError(f'src: four dimensions, got {tuple(src_c.shape)}')
    (N, H, W, C) = src_c.shape if hwc else (src_c.shape[0], src_c.shape[2], src_c.shape[3], src_c.shape[1])
    dev = src_c.device
    bkg3 = bkg_img = edge3 = edge_img = mask_c = None
    if bkg is not None:
        if torch.is_tensor(bkg) and bkg.dim() == 3:
            bkg_img = _chk(bkg, torch.float32, 'bkg')
            if tuple(bkg_img.shape) != (3, H, W):
                raise ValueError(f'bkg: (3,{H},{W}), got {tuple(bkg_img.shape)}')
        else:
            bkg3 = make_bg(torch.as_tensor(bkg).reshape(3).tolist())
    if mask is not None:
        mask_c = _chk(mask, torch.float32, 'mask')
        if tuple(mask_c.shape) != (N, 1, H, W):
            raise ValueError(f'mask: ({N},1,{H},{W}), got {tuple(mask_c.shape)}')
        if torch.is_tensor(edge_color) and edge_color.dim() == 4:
            edge_img = _chk(edge_color, torch.float32, 'edge_color')
            if tuple(edge_img.shape) != (N, 3, H, W):
                raise ValueError(f'edge_color: ({N},3,{H},{W}), got {tuple(edge_img.shape)}')
        elif edge_color is not None:
            edge3 = make_bg(torch.as_tensor(edge_color).reshape(3).tolist())
    if out is None:
        out = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (N, H, W, 3)):
        raise ValueError(f'out: a contiguous ({N},{H},{W},3) uint8 GPU tensor')
    flags = (_lib.FRAME_HWC if hwc else 0) | (_lib.FRAME_EDGE_FIRST if edge_first else 0) | (_lib.FRAME_CLAMP_INPUT if clamp_input else 0)
    if N == 0:                  # (an empty tensor has no address to validate)
        return out
    _lib.call('dbw_frames_u8', _ptr(src_c), N, C, H, W, flags, _bg_ptr(bkg3), _ptr(bkg_img), _ptr(mask_c), _bg_ptr(edge3), _ptr(edge_img),
              _ptr(out), _stream(src_c))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# run monitor (include/dbw_monitor.h)
# ---------------------------------------------------------------------------------------------------------------------
def _monitor_lib():
    return _lib.family('monitor')


def image_score_sums(a, b, padding=False, return_map=False):
    """dbw_image_scores as it stands: a, b (N,3,H,W) fp32 on the GPU -> out (N,2) fp64 on the GPU, [sum (a - b)^2, sum of the SSIM map] per
    image (and the (N,3,H',W') map with return_map).  Two launches on the current stream, no host read."""
    lib = _monitor_lib()
    a_c, b_c = _chk(a, torch.float32, 'a'), _chk(b, torch.float32, 'b')
    if a_c.dim() != 4 or a_c.shape[1] != 3 or a_c.shape != b_c.shape:
        raise ValueError(f'a, b: two (N,3,H,W) tensors, got {tuple(a_c.shape)} and {tuple(b_c.shape)}')
    N, _, H, W = a_c.shape
    if not padding and (H < 11 or W < 11):
        raise ValueError(f'images of {(H, W)} hold no 11 x 11 window: SSIM without padding needs H >= 11 and W >= 11')
    Hp, Wp = (H, W) if padding else (H - 10, W - 10)
    dev = a_c.device
    out = torch.empty(N, 2, dtype=torch.float64, device=dev)
    ssim_map = torch.empty(N, 3, Hp, Wp, dtype=torch.float32, device=dev) if return_map else None
    if N > 0:
        ws = torch.empty(lib.dbw_image_scores_workspace_bytes(N, H, W, int(bool(padding))) // 8, dtype=torch.float64, device=dev)
        _lib.call('dbw_image_scores', _ptr(a_c), _ptr(b_c), N, H, W, int(bool(padding)), _ptr(ws), _ptr(ssim_map), _ptr(out), _stream(a_c))
    return (out, ssim_map) if return_map else out


def image_scores(a, b, padding=False, return_map=False):
    """Mean squared error and mean SSIM per image of a against b, (N,3,H,W) fp32 in [0, 1] -> (mse (N,), ssim (N,)) fp64 on the device of
    the inputs (and the (N,3,H',W') SSIM map with return_map); padding=False keeps the windows inside the image, as the evaluation does.
    On the GPU one dbw_image_scores; CPU tensors go through metrics.ssim_map."""
    if not a.is_cuda:
        from .metrics import ssim_map as _ssim_map
        if a.dim() != 4 or a.shape[1] != 3 or a.shape != b.shape:
            raise ValueError(f'a, b: two (N,3,H,W) tensors, got {tuple(a.shape)} and {tuple(b.shape)}')
        if not padding and (a.shape[2] < 11 or a.shape[3] < 11):
            raise ValueError(f'images of {tuple(a.shape[2:])} hold no 11 x 11 window: SSIM without padding needs H >= 11 and W >= 11')
        m = _ssim_map(a.float(), b.float(), padding=bool(padding))
        mse = ((a.double() - b.double()) ** 2).flatten(1).mean(1)
        res = (mse, m.double().flatten(1).mean(1))
        return res + (m,) if return_map else res
    r = image_score_sums(a, b, padding, return_map)
    out, m = r if return_map else (r, None)
    H, W = a.shape[2:]
    Hp, Wp = (H, W) if padding else (H - 10, W - 10)
    res = (out[:, 0] / (3 * H * W), out[:, 1] / (3 * Hp * Wp))
    return res + (m,) if return_map else res


def _ssim_term_call(imgs, rec, masks, count, with_grad):
    """dbw_monitor_ssim_term (masks None) or dbw_monitor_masked_ssim_term: the checks, the outputs, the workspace and the call."""
    lib = _monitor_lib()
    a_c, b_c = _chk(imgs, torch.float32, 'imgs'), _chk(rec, torch.float32, 'rec')
    if a_c.dim() != 4 or a_c.shape[1] != 3 or a_c.shape != b_c.shape or a_c.shape[0] == 0:
        raise ValueError(f'imgs, rec: two (N,3,H,W) tensors, N > 0, got {tuple(a_c.shape)} and {tuple(b_c.shape)}')
    N, _, H, W = a_c.shape
    name, m_args, c_args = 'dbw_monitor_ssim_term', (), ()
    if masks is not None:
        m_c = _chk(masks, torch.float32, 'masks')
        if tuple(m_c.shape) != (N, 1, H, W):
            raise ValueError(f'masks: {(N, 1, H, W)}, got {tuple(m_c.shape)}')
        name, m_args, c_args = 'dbw_monitor_masked_ssim_term', (_ptr(m_c),), (float(count),)
    dev = a_c.device
    value = torch.empty(1, dtype=torch.float64, device=dev)
    grad = torch.empty_like(b_c) if with_grad else None
    ws = torch.empty(getattr(lib, name + '_workspace_bytes')(N, H, W) // 8, dtype=torch.float64, device=dev)
    _lib.call(name, _ptr(a_c), _ptr(b_c), *m_args, N, H, W, *c_args, _ptr(ws), _ptr(grad), _ptr(value), _stream(a_c))
    return value, grad


def ssim_term_value_grad(imgs, rec, with_grad=True):
    """dbw_monitor_ssim_term as it stands: imgs, rec (N,3,H,W) fp32 contiguous on the GPU, N > 0 -> (value (1,) fp64 = mean(1 - SSIM) with
    zero padding, d value / d rec (N,3,H,W) fp32 -- None without with_grad).  Two launches on the current stream, no host read."""
    return _ssim_term_call(imgs, rec, None, None, with_grad)


def mask_count(masks):
    """count = 3 * sum(masks) as a python float: ONE host read (a synchronisation); a training loop passes the number instead."""
    return 3.0 * float(masks.sum(dtype=torch.float64))


def masked_ssim_term_value_grad(imgs, rec, masks, count, with_grad=True):
    """dbw_monitor_masked_ssim_term as it stands: imgs, rec (N,3,H,W), masks (N,1,H,W) fp32 contiguous on the GPU, N > 0, count a host
    number -> (value (1,) fp64 = sum masks (1 - SSIM(masks imgs, masks rec)) / count, d value / d rec (N,3,H,W) fp32 -- None without
    with_grad).  Two launches on the current stream, no host read."""
    return _ssim_term_call(imgs, rec, masks, count, with_grad)


class _SsimTerm(torch.autograd.Function):
    """The term as one node, plain (masks None) or under the mask: the forward leaves the gradient beside the value where rec requires
    one, the backward scales it by the incoming scalar."""

    @staticmethod
    def forward(ctx, imgs, rec, masks=None, count=None):
        with_grad = ctx.needs_input_grad[1]
        if masks is None:
            value, grad = ssim_term_value_grad(imgs, rec.detach(), with_grad=with_grad)
        else:
            value, grad = masked_ssim_term_value_grad(imgs, rec.detach(), masks, count, with_grad=with_grad)
        ctx.save_for_backward(grad)
        return value[0].to(rec.dtype)

    @staticmethod
    def backward(ctx, g):
        grad, = ctx.saved_tensors
        return None, grad * g, None, None


def _ssim_term_kernel_ok(imgs, rec):
    return (imgs.is_cuda and rec.is_cuda and imgs.dtype == rec.dtype == torch.float32 and imgs.is_contiguous() and rec.is_contiguous()
            and not imgs.requires_grad and imgs.dim() == 4 and imgs.shape == rec.shape and imgs.shape[1] == 3 and imgs.numel() > 0)


def ssim_term(imgs, rec, masks=None, count=None):
    """The SSIM term of the loss: mean over n, c, y, x of 1 - SSIM(imgs, rec), (N,3,H,W) in [0, 1], 11 taps, sigma 1.5, zero padding (the
    reference's SSIMLoss(padding=True), averaged over the batch) -> scalar on the device of the inputs, differentiable in rec.
    fp32 contiguous GPU tensors: one dbw_monitor_ssim_term, which leaves the gradient beside the value where rec requires one; the backward
    scales it by the incoming scalar.  imgs gets no gradient there.  Anything the kernel does not take (CPU tensors, another dtype, strides,
    imgs that requires a gradient, an empty batch) goes through metrics.ssim_map(padding=True) and autograd.
    masks (N,1,H,W) weights in [0, 1]: the term under a validity mask,
        s = ssim_map(imgs * masks, rec * masks, padding=True);  ((1 - s) * masks).sum() / count,   count = 3 * masks.sum(),
    0 for count == 0 -- one dbw_monitor_masked_ssim_term under the same conditions (masks fp32 contiguous, no gradient), the formula in
    torch otherwise.  count=None costs one masks.sum() host read (mask_count); a training loop passes the number."""
    if masks is not None:
        if count is None:
            count = mask_count(masks)
        count = float(count)
        if (_ssim_term_kernel_ok(imgs, rec) and masks.is_cuda and masks.dtype == torch.float32 and masks.is_contiguous()
                and not masks.requires_grad and tuple(masks.shape) == (imgs.shape[0], 1) + tuple(imgs.shape[2:])):
            return _SsimTerm.apply(imgs, rec, masks, count)
        from .metrics import ssim_map as _ssim_map
        if imgs.dim() != 4 or imgs.shape != rec.shape or masks.dim() != 4:
            raise ValueError(f'imgs, rec: two (N,C,H,W) tensors, masks (N,1,H,W); got {tuple(imgs.shape)}, {tuple(rec.shape)}, {tuple(masks.shape)}')
        total = ((1 - _ssim_map(imgs * masks, rec * masks, padding=True)) * masks).sum()
        return total / count if count > 0 else total * 0.0
    if not _ssim_term_kernel_ok(imgs, rec):
        from .metrics import ssim_map as _ssim_map
        if imgs.dim() != 4 or imgs.shape != rec.shape:
            raise ValueError(f'imgs, rec: two (N,C,H,W) tensors, got {tuple(imgs.shape)} and {tuple(rec.shape)}')
        return (1 - _ssim_map(imgs, rec, padding=True)).mean()
    return _SsimTerm.apply(imgs, rec)


# ---------------------------------------------------------------------------------------------------------------------
# image ingest (include/dbw_ingest.h)
# ---------------------------------------------------------------------------------------------------------------------
_RESAMPLE_TABLES = {}
_RESAMPLE_FORMS = {'auto': _lib.RESAMPLE_AUTO, 'general': _lib.RESAMPLE_GENERAL, 'fused': _lib.RESAMPLE_FUSED}


def resample_table(in_size, out_size, device=None):
    """dbw_resample_table: the (out_size, ksize + 2) int32 rows [xmin, n, k_0 .. k_{ksize-1}] of one axis, on the host -- or, with a
    device, the copy of them resident there, made once per (in_size, out_size, device)."""
    lib = _lib.family('ingest')
    key = (int(in_size), int(out_size), None if device is None else str(torch.device(device)))
    if key not in _RESAMPLE_TABLES:
        if device is not None:
            _RESAMPLE_TABLES[key] = resample_table(in_size, out_size).to(device)
        else:
            ksize = lib.dbw_resample_table(key[0], key[1], None, 0)
            if ksize <= 0:
                raise RuntimeError(f'dbw_resample_table failed (rc={ksize}): {lib.dbw_last_error().decode()}')
            t = torch.zeros(key[1], ksize + 2, dtype=torch.int32)
            rc = lib.dbw_resample_table(key[0], key[1], t.data_ptr(), t.numel())
            if rc != ksize:
                raise RuntimeError(f'dbw_resample_table failed (rc={rc}): {lib.dbw_last_error().decode()}')
            _RESAMPLE_TABLES[key] = t
    return _RESAMPLE_TABLES[key]


def resample_u8(src_u8, size, out='f32', form='auto'):
    """dbw_images_resample_u8: (N,Hin,Win,3) uint8 frames on the GPU -> what the reference's Compose([Resize(size), ToTensor()]) makes of
    them on the host, bit for bit (Pillow's antialiased BILINEAR resample in 8-bit fixed point, then uint8 / 255 in fp32).  size (Hout,Wout).
    out: 'f32' -> (N,3,Hout,Wout) fp32, the layout of views['imgs']; 'u8' -> (N,Hout,Wout,3) uint8; 'both' -> the pair.  form: 'auto', or
    'general' / 'fused' to force one of the two kernel forms (the same bytes; 'fused' refuses ratios above 5)."""
    lib = _lib.family('ingest')
    if out not in ('f32', 'u8', 'both') or form not in _RESAMPLE_FORMS:
        raise ValueError(f"out: 'f32', 'u8' or 'both', form: 'auto', 'general' or 'fused'; got {out!r}, {form!r}")
    src = _chk(src_u8, torch.uint8, 'src_u8')
    if src.dim() != 4 or src.shape[3] != 3:
        raise ValueError(f'src_u8: (N,Hin,Win,3), got {tuple(src.shape)}')
    N, Hin, Win, _ = src.shape
    Hout, Wout = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if Hout <= 0 or Wout <= 0 or Hin <= 0 or Win <= 0:
        raise ValueError(f'bad size: {(Hin, Win)} -> {(Hout, Wout)}')
    dev = src.device
    f32 = torch.empty(N, 3, Hout, Wout, dtype=torch.float32, device=dev) if out != 'u8' else None
    u8 = torch.empty(N, Hout, Wout, 3, dtype=torch.uint8, device=dev) if out != 'f32' else None
    if N > 0:
        tx = resample_table(Win, Wout, dev) if Win != Wout else None
        ty = resample_table(Hin, Hout, dev) if Hin != Hout else None
        ws_bytes = 0 if form == 'fused' else lib.dbw_images_resample_workspace_bytes(N, Hin, Win, Hout, Wout)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
        _lib.call('dbw_images_resample_u8', _ptr(src), N, Hin, Win, Hout, Wout, _ptr(tx), _ptr(ty), _ptr(f32), _ptr(u8), _ptr(ws), ws_bytes,
                  _RESAMPLE_FORMS[form], _stream(src))
    return {'f32': f32, 'u8': u8, 'both': (f32, u8)}[out]


# ---------------------------------------------------------------------------------------------------------------------
# lens rectification (include/dbw_lens.h)
# ---------------------------------------------------------------------------------------------------------------------
def lens_params(intr, dist, zoom=1.0):
    """The HOST `lens` array of dbw_images_undistort_u8, a (12,) fp32 CPU tensor [fx, fy, cx, cy, 1/(zoom fx), 1/(zoom fy), k1, k2, k3, k4, p1, p2], from
    intr = (fx, fy, cx, cy) in pixels of the source frames and dist = (k1, k2, k3, k4, p1, p2).  The reciprocals are taken in fp64 and
    rounded once."""
    intr, dist = [float(v) for v in intr], [float(v) for v in dist]
    if len(intr) != 4 or len(dist) != 6:
        raise ValueError(f'intr: (fx, fy, cx, cy), dist: (k1, k2, k3, k4, p1, p2); got {len(intr)} and {len(dist)} values')
    zoom = float(zoom)
    if not (zoom > 0 and intr[0] > 0 and intr[1] > 0):
        raise ValueError(f'zoom and the focal lengths must be positive, got zoom={zoom}, fx={intr[0]}, fy={intr[1]}')
    return torch.tensor(intr + [1.0 / (zoom * intr[0]), 1.0 / (zoom * intr[1])] + dist, dtype=torch.float64).to(torch.float32)


def undistort_u8(raw_u8, intr, dist, zoom=1.0):
    """dbw_images_undistort_u8: (N,H,W,3) uint8 frames on the GPU, taken through a lens with OpenCV's radial-tangential distortion `dist` =
    (k1, k2, k3, k4, p1, p2) and the intrinsics `intr` = (fx, fy, cx, cy), -> the (N,H,W,3) uint8 frames of the pinhole camera with the
    focal lengths zoom * (fx, fy) and the same principal point, bilinear (csrc/lens_math.h).  One map for all N frames."""
    lib = _lib.family('lens')
    src = _chk(raw_u8, torch.uint8, 'raw_u8')
    if src.dim() != 4 or src.shape[3] != 3:
        raise ValueError(f'raw_u8: (N,H,W,3), got {tuple(src.shape)}')
    N, H, W, _ = src.shape
    if H < 2 or W < 2:
        raise ValueError(f'frames of {(H, W)}: at least 2 x 2')
    lens = lens_params(intr, dist, zoom)
    out = torch.empty_like(src)
    if N > 0:
        _lib.call('dbw_images_undistort_u8', _ptr(src), N, H, W, lens.data_ptr(), _ptr(out), _stream(src))
    return out


def lens_valid_u8(H, W, intr, dist, zoom=1.0, device='cuda'):
    """dbw_lens_valid_u8: the (H,W) uint8 validity map of the frames undistort_u8 makes with the same arguments, on `device` -- 255 where
    the output pixel reads inside the source frame (not clamped), 0 elsewhere.  One map per scene."""
    _lib.family('lens')
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f'a frame of {(H, W)}')
    lens = lens_params(intr, dist, zoom)
    out = torch.empty(H, W, dtype=torch.uint8, device=device)
    if not out.is_cuda:
        raise RuntimeError('lens_valid_u8 runs on the GPU (there is no CPU fallback)')
    _lib.call('dbw_lens_valid_u8', H, W, lens.data_ptr(), _ptr(out), _stream(out))
    return out


LENS_MODELS = {'OPENCV': 0, 'PINHOLE': 0, 'OPENCV_FISHEYE': 1}         # the model id of a row of lens_table


def lens_table(intrs, dists, models):
    """The HOST `cams` table of dbw_lens_rectify_u8, an (N,16) fp32 CPU tensor with one row [model, fx, fy, cx, cy, k1, k2, k3, k4, p1, p2,
    0, 0, 0, 0, 0] per frame, from intrs (N,4) = (fx, fy, cx, cy) in pixels, dists (N,6) = (k1, k2, k3, k4, p1, p2) and models (N,) of 0
    (radial-tangential) or 1 (fisheye)."""
    intrs = torch.as_tensor(intrs, dtype=torch.float64).reshape(-1, 4)
    dists = torch.as_tensor(dists, dtype=torch.float64).reshape(-1, 6)
    models = torch.as_tensor(models, dtype=torch.float64).reshape(-1)
    N = intrs.shape[0]
    if dists.shape[0] != N or models.shape[0] != N:
        raise ValueError(f'intrs (N,4), dists (N,6), models (N,): got {N}, {dists.shape[0]} and {models.shape[0]} rows')
    if not bool(((models == 0) | (models == 1)).all()):
        raise ValueError('models: 0 (radial-tangential) or 1 (fisheye)')
    if not bool((intrs[:, :2] > 0).all()):
        raise ValueError('the focal lengths must be positive')
    table = torch.zeros(N, _lib.LENS_RECT_N_PARAMS, dtype=torch.float64)
    table[:, 0], table[:, 1:5], table[:, 5:11] = models, intrs, dists
    return table.to(torch.float32)


def lens_target(intr0, zoom=1.0):
    """The HOST `target` array of dbw_lens_rectify_u8, a (4,) fp32 CPU tensor [cx0, cy0, 1/(zoom fx0), 1/(zoom fy0)], from the pinhole camera
    intr0 = (fx0, fy0, cx0, cy0) every frame is resampled into.  The reciprocals are taken in fp64 and rounded once."""
    intr0 = [float(v) for v in intr0]
    if len(intr0) != 4:
        raise ValueError(f'intr0: (fx, fy, cx, cy), got {len(intr0)} values')
    zoom = float(zoom)
    if not (zoom > 0 and intr0[0] > 0 and intr0[1] > 0):
        raise ValueError(f'zoom and the focal lengths must be positive, got zoom={zoom}, fx={intr0[0]}, fy={intr0[1]}')
    return torch.tensor([intr0[2], intr0[3], 1.0 / (zoom * intr0[0]), 1.0 / (zoom * intr0[1])], dtype=torch.float64).to(torch.float32)


def _rect_tables(table_rows, target, N):
    table = torch.as_tensor(table_rows, dtype=torch.float32).contiguous()
    target = torch.as_tensor(target, dtype=torch.float32).contiguous()
    if table.is_cuda or target.is_cuda:
        raise ValueError('table_rows and target are HOST arrays (ops.lens_table, ops.lens_target)')
    if tuple(table.shape) != (N, _lib.LENS_RECT_N_PARAMS) or tuple(target.shape) != (4,):
        raise ValueError(f'table_rows: ({N},{_lib.LENS_RECT_N_PARAMS}), target: (4,); got {tuple(table.shape)} and {tuple(target.shape)}')
    return table, target


def rectify_u8(raw_u8, table_rows, target):
    """dbw_lens_rectify_u8: (N,H,W,3) uint8 frames on the GPU, frame n taken by the camera of row n of table_rows (ops.lens_table: a model,
    intrinsics and coefficients of its own), -> the (N,H,W,3) uint8 frames of the one pinhole camera `target` (ops.lens_target), bilinear
    (csrc/lens_math.h)."""
    _lib.family('lens')
    src = _chk(raw_u8, torch.uint8, 'raw_u8')
    if src.dim() != 4 or src.shape[3] != 3:
        raise ValueError(f'raw_u8: (N,H,W,3), got {tuple(src.shape)}')
    N, H, W, _ = src.shape
    if H < 2 or W < 2:
        raise ValueError(f'frames of {(H, W)}: at least 2 x 2')
    table, target = _rect_tables(table_rows, target, N)
    out = torch.empty_like(src)
    if N > 0:
        _lib.call('dbw_lens_rectify_u8', _ptr(src), N, H, W, table.data_ptr(), target.data_ptr(), _ptr(out), _stream(src))
    return out


def rectify_valid_u8(H, W, table_rows, target, device='cuda'):
    """dbw_lens_rectify_valid_u8: the (N,H,W) uint8 validity maps of the frames rectify_u8 makes with the same arguments, on `device` -- 255
    where the output pixel reads inside its source frame (not clamped), 0 elsewhere."""
    _lib.family('lens')
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f'a frame of {(H, W)}')
    table, target = _rect_tables(table_rows, target, len(table_rows))
    out = torch.empty(table.shape[0], H, W, dtype=torch.uint8, device=device)
    if not out.is_cuda:
        raise RuntimeError('rectify_valid_u8 runs on the GPU (there is no CPU fallback)')
    if table.shape[0] > 0:
        _lib.call('dbw_lens_rectify_valid_u8', table.shape[0], H, W, table.data_ptr(), target.data_ptr(), _ptr(out), _stream(out))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the point cloud of a capture's depth maps (include/dbw_lens.h)
# ---------------------------------------------------------------------------------------------------------------------
DEPTH_SUB = 1024                # quantisation steps of a cell along an axis (csrc/depth_math.h: 1 << DEPTH_SUB_BITS)
DEPTH_MAX_GRID = 256


def depth_box(lo, hi, grid):
    """The HOST `box` array of dbw_lens_depth_cloud, 4 fp32 [lo_x, lo_y, lo_z, inv_step] as a numpy array, from the corners lo, hi (a number
    or 3 numbers each) of a CUBE and the cells per axis: inv_step = grid * 1024 / (hi - lo), taken in fp64 and rounded once."""
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), (3,)), np.broadcast_to(np.asarray(hi, np.float64), (3,))
    side = hi - lo
    if not (np.isfinite(side).all() and side[0] > 0 and side[1] == side[0] and side[2] == side[0]):
        raise ValueError(f'lo, hi: the corners of a cube (hi - lo the same positive number on the three axes), got {lo.tolist()} and {hi.tolist()}')
    if not 1 <= int(grid) <= DEPTH_MAX_GRID:
        raise ValueError(f'grid: 1 .. {DEPTH_MAX_GRID}, got {grid}')
    return np.array([lo[0], lo[1], lo[2], int(grid) * float(DEPTH_SUB) / side[0]], dtype=np.float64).astype(np.float32)


def _depth_args(shape, cams, target, poses, lo, hi, grid, d_range, stride, edge, min_count):
    """The arguments the kernel and the numpy path share, checked: (cams (N,16), target (4,), poses (N,12), box (4,)) as contiguous fp32
    numpy arrays and (G, d_min, d_max, stride, edge_permille, min_count) as ints."""
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f'depth: (N,H,W) with N, H, W >= 1, got {tuple(shape)}')
    N = shape[0]
    as_np = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32)
    cams, target, poses = as_np(cams), as_np(target), as_np(poses).reshape(-1, 12)
    if cams.shape != (N, _lib.LENS_RECT_N_PARAMS) or target.shape != (4,) or poses.shape != (N, 12):
        raise ValueError(f'cams: ({N},{_lib.LENS_RECT_N_PARAMS}), target: (4,), poses: ({N},12); got {cams.shape}, {target.shape} and {poses.shape}')
    box = depth_box(lo, hi, grid)
    for name, a in (('cams', cams), ('target', target), ('poses', poses), ('box', box)):
        if not np.isfinite(a).all():
            raise ValueError(f'{name}: a value that is not finite')
    if not (box[3] > 0 and (target[2:] > 0).all() and (cams[:, 1:3] > 0).all() and np.isin(cams[:, 0], (0.0, 1.0)).all()):
        raise ValueError('inv_step, the focal lengths and the reciprocals of the target must be positive, a model id 0 or 1')
    d_min, d_max = int(d_range[0]), int(d_range[1])
    permille = int(round(float(edge) * 1000))
    stride, min_count = int(stride), int(min_count)
    if not (1 <= d_min <= d_max <= 65535 and stride >= 1 and 0 <= permille <= 1000 and min_count >= 1):
        raise ValueError(f'd_range: 1 <= d_min <= d_max <= 65535, stride >= 1, edge in [0, 1], min_count >= 1; got {d_range}, {stride}, {edge}, {min_count}')
    return cams, target, poses, box, int(grid), d_min, d_max, stride, permille, min_count


def depth_cloud(depth, cams, target, poses, lo, hi, grid=128, d_range=(1, 65535), stride=1, edge=0.0, min_count=1, device=None, return_info=False,
                workspace=None):
    """dbw_lens_depth_cloud: (N,H,W) 16-bit depth maps -> (points (M,3) float32, counts (M,) int32) on depth's device, one point per cell of
    the grid^3 cells of the cube [lo, hi] that at least min_count samples fall into, in ascending cell order (csrc/depth_math.h).
    depth: a torch.int16 tensor holding the 16 bits (or torch.uint16), or a numpy uint16 array, which is uploaded to `device` ('cuda' by
    default).  cams (N,16) and target (4,): ops.lens_table and ops.lens_target at the depth maps' resolution; poses (N,12): rows [A, t],
    camera (x right, y down, z forward, in depth units) to world; d_range = (d_min, d_max) in depth units; stride: every stride-th row and
    column of the target; edge: a sample whose source pixel has a 4-neighbour that is 0 or differs by more than edge * d is dropped (0:
    off).  The one host read is M.  return_info: also [M, samples accumulated, samples outside the box] as a list.  workspace: a uint8
    tensor of dbw_lens_depth_cloud_workspace_bytes(grid) bytes to use instead of a fresh one (its contents do not matter: the call clears it)."""
    lib = _lib.family('lens')
    if isinstance(depth, np.ndarray):
        if depth.dtype != np.uint16:
            raise TypeError(f'depth: a numpy array of uint16, got {depth.dtype}')
        depth = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(device or 'cuda')
    if depth.dtype not in (torch.int16, getattr(torch, 'uint16', torch.int16)):
        raise TypeError(f'depth: torch.int16 holding the 16 bits (or torch.uint16), got {depth.dtype}')
    if not depth.is_cuda:
        raise RuntimeError('depth_cloud runs on the GPU (ops.depth_cloud_host is the numpy path)')
    depth = depth.contiguous()
    cams, target, poses, box, G, d_min, d_max, stride, permille, min_count = _depth_args(depth.shape, cams, target, poses, lo, hi, grid, d_range,
                                                                                        stride, edge, min_count)
    N, H, W = depth.shape
    samples = N * -(-H // stride) * -(-W // stride)
    if samples >= 1 << 31:
        raise ValueError(f'{samples} samples: below 2^31 a call')
    capacity = min(G ** 3, samples)
    dev = depth.device
    need = lib.dbw_lens_depth_cloud_workspace_bytes(G)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError(f'workspace: a contiguous uint8 tensor of at least {need} bytes on {dev}')
    points = torch.empty(capacity, 3, dtype=torch.float32, device=dev)
    counts = torch.empty(capacity, dtype=torch.int32, device=dev)
    info = torch.empty(3, dtype=torch.int64, device=dev)
    _lib.call('dbw_lens_depth_cloud', _ptr(depth), N, H, W, cams.ctypes.data, target.ctypes.data, poses.ctypes.data, box.ctypes.data, G, d_min, d_max,
              stride, permille, min_count, _ptr(workspace), _ptr(points), _ptr(counts), capacity, _ptr(info), _stream(depth))
    info = [int(v) for v in info.tolist()]
    out = (points[:info[0]], counts[:info[0]])
    return out + (info,) if return_info else out


def _lens_atan32(t):
    """lens_atan of csrc/lens_math.h on a float32 array t >= 0, operation by operation."""
    F = np.float32
    big = t > F(2.414213562373095)
    mid = ~big & (t > F(0.4142135623730950))
    a = np.where(big, -(F(1.0) / t), np.where(mid, (t - F(1.0)) / (t + F(1.0)), t))
    y0 = np.where(big, F(1.5707963267948966), np.where(mid, F(0.7853981633974483), F(0.0)))
    z = a * a
    q = ((F(8.05374449538e-2) * z - F(1.38776856032e-1)) * z + F(1.99777106478e-1)) * z - F(3.33329491539e-1)
    return y0 + ((q * z) * a + a)


def _lens_rect_source32(cam, target, i, j):
    """lens_rect_source of csrc/lens_math.h on int arrays (i, j), operation by operation in float32 -> (x, y, u, v)."""
    F = np.float32
    model, fx, fy, cx, cy, k1, k2, k3, k4, p1, p2 = [F(v) for v in cam[:11]]
    cx0, cy0, inv_fx0, inv_fy0 = [F(v) for v in target]
    x = (j.astype(F) + F(0.5) - cx0) * inv_fx0
    y = (i.astype(F) + F(0.5) - cy0) * inv_fy0
    xx, yy, xy = x * x, y * y, x * y
    r2 = xx + yy
    if model == F(1.0):
        r = np.sqrt(r2)
        th = _lens_atan32(r)
        t2 = th * th
        td = th * (F(1.0) + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
        s = np.where(r2 == F(0.0), F(1.0), td / r)
        return x, y, (x * s) * fx + cx - F(0.5), (y * s) * fy + cy - F(0.5)
    d = F(1.0) + r2 * (k1 + r2 * (k2 + r2 * (k3 + r2 * k4)))
    xd = x * d + (F(2.0) * p1) * xy + p2 * (r2 + F(2.0) * xx)
    yd = y * d + (F(2.0) * p2) * xy + p1 * (r2 + F(2.0) * yy)
    return x, y, xd * fx + cx - F(0.5), yd * fy + cy - F(0.5)


def depth_cloud_host(depth, cams, target, poses, lo, hi, grid=128, d_range=(1, 65535), stride=1, edge=0.0, min_count=1, return_info=False):
    """ops.depth_cloud in numpy, for a run without a GPU: depth (N,H,W) uint16 (numpy, or a CPU tensor of int16 / uint16 bits) -> (points
    (M,3) float32, counts (M,) int32) as numpy arrays, the same bytes as the kernel: csrc/depth_math.h operation by operation in float32,
    the cells' counts and sums added up as integers (np.add.at), the points formed in float64 and rounded once."""
    F = np.float32
    if torch.is_tensor(depth):
        depth = depth.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
    depth = np.ascontiguousarray(depth)
    if depth.dtype != np.uint16:
        raise TypeError(f'depth: uint16, got {depth.dtype}')
    cams, target, poses, box, G, d_min, d_max, stride, permille, min_count = _depth_args(depth.shape, cams, target, poses, lo, hi, grid, d_range,
                                                                                        stride, edge, min_count)
    N, H, W = depth.shape
    i, j = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing='ij')
    i, j = i.reshape(-1), j.reshape(-1)
    count = np.zeros(G ** 3, np.uint32)
    sums = np.zeros((3, G ** 3), np.uint64)
    lim = F(G * DEPTH_SUB)
    n_in = n_out = 0
    with np.errstate(all='ignore'):
        for n in range(N):
            x, y, u, v = _lens_rect_source32(cams[n], target, i, j)
            fu, fv = np.floor(u + F(0.5)), np.floor(v + F(0.5))
            keep = (fu >= F(0.0)) & (fu <= F(W - 1)) & (fv >= F(0.0)) & (fv <= F(H - 1))                     # (False for a NaN)
            sx, sy = np.where(keep, fu, F(0.0)).astype(np.int64), np.where(keep, fv, F(0.0)).astype(np.int64)
            frame = depth[n].astype(np.int64)
            d = frame[sy, sx]
            keep &= (d >= d_min) & (d <= d_max)
            if permille > 0:
                for inside, ny, nx in ((sx > 0, sy, sx - 1), (sx < W - 1, sy, sx + 1), (sy > 0, sy - 1, sx), (sy < H - 1, sy + 1, sx)):
                    nb = frame[np.clip(ny, 0, H - 1), np.clip(nx, 0, W - 1)]
                    keep &= ~(inside & ((nb == 0) | (1000 * np.abs(d - nb) > permille * d)))
            z = d.astype(F)
            cx, cy = x * z, y * z
            A = poses[n]
            q, inside = [], keep.copy()
            for a in range(3):
                p = ((A[3 * a] * cx + A[3 * a + 1] * cy) + A[3 * a + 2] * z) + A[9 + a]
                f = np.floor((p - box[a]) * box[3])
                ok = (f >= F(0.0)) & (f < lim)                                                          # (False for a NaN)
                inside &= ok
                q.append(np.where(ok, f, F(0.0)).astype(np.int64))
            n_in += int(inside.sum())
            n_out += int((keep & ~inside).sum())
            cell = (((q[0] >> 10) * G + (q[1] >> 10)) * G + (q[2] >> 10))[inside]
            np.add.at(count, cell, np.uint32(1))
            for a in range(3):
                np.add.at(sums[a], cell, q[a][inside].astype(np.uint64))
    rows = np.nonzero(count >= min_count)[0]
    c = count[rows].astype(np.float64)
    points = np.stack([box[a].astype(np.float64) + ((sums[a][rows].astype(np.float64) + 0.5 * c) / c) / np.float64(box[3]) for a in range(3)], 1)
    out = (points.astype(F).reshape(-1, 3), count[rows].astype(np.int32))
    return out + ([len(rows), n_in, n_out],) if return_info else out


def _depth_ray_args(shape, cams, target, poses, d_range, stride, edge):
    cams, target, poses, _, _, d_min, d_max, stride, permille, _ = _depth_args(shape, cams, target, poses, 0.0, 1.0, 1, d_range, stride, edge, 1)
    return cams, target, poses, d_min, d_max, stride, permille


def depth_rays(depth, cams, target, poses, d_range=(1, 65535), stride=1, edge=0.0, device=None):
    """dbw_lens_depth_rays: (N,H,W) 16-bit depth maps -> the dense record array (N, ceil(H/stride), ceil(W/stride), 4) int32 on depth's device:
    the three fp32 words of the ray's end -- the world point exactly as ops.depth_cloud forms it before its cube -- and the frame, -1 (after
    three zeros) where there is no measurement (lens, range, edge rule, a coordinate that is not finite).  Arguments as ops.depth_cloud's,
    without the grid and the cube.  Nothing is read by the host; ops.depth_rays_compact keeps the valid records."""
    _lib.family('lens')
    if isinstance(depth, np.ndarray):
        if depth.dtype != np.uint16:
            raise TypeError(f'depth: a numpy array of uint16, got {depth.dtype}')
        depth = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(device or 'cuda')
    if depth.dtype not in (torch.int16, getattr(torch, 'uint16', torch.int16)):
        raise TypeError(f'depth: torch.int16 holding the 16 bits (or torch.uint16), got {depth.dtype}')
    if not depth.is_cuda:
        raise RuntimeError('depth_rays runs on the GPU (ops.depth_rays_host is the numpy path)')
    depth = depth.contiguous()
    cams, target, poses, d_min, d_max, stride, permille = _depth_ray_args(depth.shape, cams, target, poses, d_range, stride, edge)
    N, H, W = depth.shape
    Hs, Ws = -(-H // stride), -(-W // stride)
    if N * Hs * Ws >= 1 << 31:
        raise ValueError(f'{N * Hs * Ws} samples: below 2^31 a call')
    rays = torch.empty(N, Hs, Ws, 4, dtype=torch.int32, device=depth.device)
    _lib.call('dbw_lens_depth_rays', _ptr(depth), N, H, W, cams.ctypes.data, target.ctypes.data, poses.ctypes.data, d_min, d_max, stride, permille,
              _ptr(rays), _stream(depth))
    return rays


def depth_rays_host(depth, cams, target, poses, d_range=(1, 65535), stride=1, edge=0.0):
    """ops.depth_rays in numpy, for a run without a GPU: -> (N, Hs, Ws, 4) int32 as a numpy array, the same bytes as the kernel
    (csrc/depth_math.h depth_ray_end operation by operation in float32)."""
    F = np.float32
    if torch.is_tensor(depth):
        depth = depth.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
    depth = np.ascontiguousarray(depth)
    if depth.dtype != np.uint16:
        raise TypeError(f'depth: uint16, got {depth.dtype}')
    cams, target, poses, d_min, d_max, stride, permille = _depth_ray_args(depth.shape, cams, target, poses, d_range, stride, edge)
    N, H, W = depth.shape
    i, j = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing='ij')
    Hs, Ws = i.shape
    i, j = i.reshape(-1), j.reshape(-1)
    out = np.zeros((N, Hs * Ws, 4), np.int32)
    with np.errstate(all='ignore'):
        for n in range(N):
            x, y, u, v = _lens_rect_source32(cams[n], target, i, j)
            fu, fv = np.floor(u + F(0.5)), np.floor(v + F(0.5))
            keep = (fu >= F(0.0)) & (fu <= F(W - 1)) & (fv >= F(0.0)) & (fv <= F(H - 1))                     # (False for a NaN)
            sx, sy = np.where(keep, fu, F(0.0)).astype(np.int64), np.where(keep, fv, F(0.0)).astype(np.int64)
            frame = depth[n].astype(np.int64)
            d = frame[sy, sx]
            keep &= (d >= d_min) & (d <= d_max)
            if permille > 0:
                for inside, ny, nx in ((sx > 0, sy, sx - 1), (sx < W - 1, sy, sx + 1), (sy > 0, sy - 1, sx), (sy < H - 1, sy + 1, sx)):
                    nb = frame[np.clip(ny, 0, H - 1), np.clip(nx, 0, W - 1)]
                    keep &= ~(inside & ((nb == 0) | (1000 * np.abs(d - nb) > permille * d)))
            z = d.astype(F)
            cx, cy = x * z, y * z
            A = poses[n]
            p = np.stack([((A[3 * a] * cx + A[3 * a + 1] * cy) + A[3 * a + 2] * z) + A[9 + a] for a in range(3)], 1).astype(F)
            keep &= np.isfinite(p).all(1)
            out[n, :, :3] = np.where(keep[:, None], p, F(0.0)).view(np.int32)
            out[n, :, 3] = np.where(keep, n, -1)
    return out.reshape(N, Hs, Ws, 4)


def depth_rays_compact(rays):
    """The valid records of ops.depth_rays / depth_rays_host, order kept -> (ends (Nr,3) float32, frame (Nr,) int32), torch tensors on the
    records' device: one boolean mask, taken once when a scene is loaded, not on the step path."""
    r = torch.as_tensor(rays).reshape(-1, 4)
    keep = r[:, 3] >= 0
    r = r[keep]
    return r[:, :3].contiguous().view(torch.float32), r[:, 3].contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# camera pose refinement (include/dbw_lens.h)
# ---------------------------------------------------------------------------------------------------------------------
def _pose_ids(ids, B, V, ids_host=None):
    """The batch's rows of delta as a contiguous int32 device tensor; a row named twice is refused (the chain kernel writes rows without
    atomics), and so is one outside the table.  Checked on ids_host -- the same ids where the caller holds them on the host too (the
    Trainer draws them there) -- or on one host copy of the B integers, which waits for the device."""
    if ids.numel() != B:
        raise ValueError(f'ids: one per view of the batch ({B}), got {ids.numel()}')
    if ids_host is not None and len(ids_host) != B:
        raise ValueError(f'ids_host: one per view of the batch ({B}), got {len(ids_host)}')
    host = [int(i) for i in (ids if ids_host is None else torch.as_tensor(ids_host)).reshape(-1).tolist()]
    if len(set(host)) != len(host):
        raise ValueError(f'pose_apply: the view ids of a batch must be distinct, got {host}')
    if host and (min(host) < 0 or max(host) >= V):
        raise ValueError(f'pose_apply: view ids outside [0, {V}): {host}')
    return ids.reshape(-1).to(torch.int32).contiguous()


class _PoseApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, R0, T0, delta, ids):
        B, V = R0.shape[0], delta.shape[0]
        R1, T1 = torch.empty_like(R0), torch.empty_like(T0)
        _lib.call('dbw_lens_pose_apply', _ptr(R0), _ptr(T0), _ptr(delta), _ptr(ids), B, V, _ptr(R1), _ptr(T1), _stream(R0))
        ctx.save_for_backward(R0, T0, delta, ids)
        return R1, T1

    @staticmethod
    def backward(ctx, g_R, g_T):
        R0, T0, delta, ids = ctx.saved_tensors
        B, V = R0.shape[0], delta.shape[0]
        g_R = torch.zeros_like(R0) if g_R is None else g_R.contiguous()
        g_T = torch.zeros_like(T0) if g_T is None else g_T.contiguous()
        g_delta = torch.zeros_like(delta)
        _lib.call('dbw_lens_pose_chain', _ptr(R0), _ptr(T0), _ptr(delta), _ptr(ids), B, V, _ptr(g_R), _ptr(g_T), _ptr(g_delta), _stream(R0))
        return None, None, g_delta, None


def pose_apply(R0, T0, delta, ids, ids_host=None):
    """dbw_lens_pose_apply / dbw_lens_pose_chain as one autograd function: R0 (B,3,3), T0 (B,3) of a batch, delta (V,6) = one (w, tau) per view
    of the scene, ids (B) = the batch's rows of delta, distinct -> (R', T') with R' = R0.E(w), T' = T0.E(w) + tau (csrc/pose_math.h).  Only
    delta receives a gradient: R0, T0 are data.  ids_host: the same ids on the host, where the caller has them (no wait for the device).
    The caller GUARANTEES that ids_host and ids hold the same integers: they are not compared (that would be the wait), and the
    distinctness that lets the chain kernel write rows without atomics is checked on ids_host alone."""
    if R0.dim() != 3 or tuple(R0.shape[1:]) != (3, 3) or tuple(T0.shape) != (R0.shape[0], 3) or delta.dim() != 2 or delta.shape[1] != 6:
        raise ValueError(f'pose_apply: R0 (B,3,3), T0 (B,3), delta (V,6); got {tuple(R0.shape)}, {tuple(T0.shape)}, {tuple(delta.shape)}')
    ids = _pose_ids(ids, R0.shape[0], delta.shape[0], ids_host)
    _lib.family('lens')
    return _PoseApply.apply(_chk(R0.detach(), torch.float32, 'R0'), _chk(T0.detach(), torch.float32, 'T0'),
                            _chk(delta, torch.float32, 'delta'), ids.to(R0.device))


# ---------------------------------------------------------------------------------------------------------------------
# intrinsics refinement (include/dbw_lens.h)
# ---------------------------------------------------------------------------------------------------------------------
class _IntrinsicsApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, K0, theta):
        K1 = torch.empty_like(K0)
        _lib.call('dbw_lens_intrinsics_apply', _ptr(K0), _ptr(theta), _ptr(K1), _stream(K0))
        ctx.save_for_backward(K0, theta)
        return K1

    @staticmethod
    def backward(ctx, g_K):
        K0, theta = ctx.saved_tensors
        g_theta = torch.empty_like(theta)
        _lib.call('dbw_lens_intrinsics_chain', _ptr(K0), _ptr(theta), _ptr(g_K.contiguous()), _ptr(g_theta), _stream(K0))
        return None, g_theta


def intrinsics_apply(K0, theta):
    """dbw_lens_intrinsics_apply / dbw_lens_intrinsics_chain as one autograd function: K0 (4,4) the pinhole matrix of the views, theta (4) =
    (a_x, a_y, c_x, c_y) -> K' = K0 with K'[0,0] = K0[0,0] exp(a_x), K'[1,1] = K0[1,1] exp(a_y), K'[0,2] = K0[0,2] + c_x, K'[1,2] = K0[1,2] +
    c_y (csrc/intrinsics_math.h; theta = 0 gives K0 bit for bit).  Only theta receives a gradient: K0 is data."""
    if tuple(K0.shape) != (4, 4) or tuple(theta.shape) != (4,):
        raise ValueError(f'intrinsics_apply: K0 (4,4), theta (4,); got {tuple(K0.shape)} and {tuple(theta.shape)}')
    _lib.family('lens')
    return _IntrinsicsApply.apply(_chk(K0.detach(), torch.float32, 'K0'), _chk(theta, torch.float32, 'theta'))


# ---------------------------------------------------------------------------------------------------------------------
# texture preparation, param -> mesh, losses, optimiser
# ---------------------------------------------------------------------------------------------------------------------
class _TexturePrep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, texture, decim):
        tex = _chk(texture.detach(), torch.float32, 'texture')
        n, h, w, _ = tex.shape
        maps = torch.empty_like(tex) if decim == 1 else torch.empty(n, h // decim, w // decim, 3, dtype=tex.dtype, device=tex.device)
        sig = torch.empty_like(tex) if decim > 1 else None
        _lib.call('dbw_texture_prep_fwd', _ptr(tex), n, h, w, int(decim), _ptr(maps), _ptr(sig), _stream(tex))
        ctx.save_for_backward(tex)
        ctx.decim = decim
        if sig is None:
            sig = maps
            ctx.alias = True
        else:
            ctx.alias = False
        return maps, sig

    @staticmethod
    def backward(ctx, g_maps, g_sig):
        (tex,) = ctx.saved_tensors
        n, h, w, _ = tex.shape
        if ctx.alias:          # maps and sig are the same tensor: autograd hands two grads for it
            g = None
            for t in (g_maps, g_sig):
                if t is not None:
                    g = t if g is None else g + t
            g_maps, g_sig = g, None
        if g_maps is None:
            d = ctx.decim
            g_maps = torch.zeros(n, h // d, w // d, 3, dtype=tex.dtype, device=tex.device)
        out = torch.empty_like(tex)
        _lib.call('dbw_texture_prep_bwd', _ptr(tex), n, h, w, int(ctx.decim), _ptr(g_maps.contiguous()),
                  _ptr(None if g_sig is None else g_sig.contiguous()), _ptr(out), _stream(tex))
        return out, None


def texture_prep(texture, decim=1):
    """(n,h,w,3) logits -> (maps sampled by the renderer: (n,h/d,w/d,3) cell means when decim > 1 -- pair them with
    `shift = log2(decim)` in the map descriptor --, undecimated sigmoid for the TV loss)."""
    maps, sig = _TexturePrep.apply(texture, int(decim))
    return maps, sig


def sq_blocks(sq_eps, S, R6, T, trig, keep, nb, ratio, scale_min, S_world, R_world, T_world, dense=True):
    """-> world verts of the blocks.  dense=True: (nb,nv,3), only the kept blocks, packed (`nb` = their number, a host int);
    dense=False: (Kb,nv,3), skipped blocks collapsed to a point (no host knowledge of `keep` needed)."""
    if dense and keep is not None and nb == 0:
        return trig.new_empty(0, trig.shape[2], 3)
    if not dense:
        nb = trig.shape[1]
    return _SqBlocks.apply(sq_eps, S, R6, T, trig, keep, nb, (float(ratio), float(scale_min), float(S_world), R_world, T_world, bool(dense)))


class _SqBlocks(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sq_eps, S, R6, T, trig, keep, nb, consts):
        ratio, scale_min, S_world, Rw, Tw, dense = consts
        args = [_chk(t.detach(), torch.float32, 'pose param') for t in (sq_eps, S, R6, T)]
        Kb, nv = trig.shape[1], trig.shape[2]
        verts = torch.empty(nb, nv, 3, dtype=torch.float32, device=trig.device)
        _lib.call('dbw_sq_blocks_fwd', *[_ptr(a) for a in args], _ptr(trig), _ptr(keep), int(dense), Kb, nv, ratio, scale_min, S_world,
                  _ptr(Rw), _ptr(Tw), _ptr(verts), _stream(trig))
        ctx.save_for_backward(*args, trig, keep if keep is not None else trig.new_empty(0), Rw)
        ctx.consts = (ratio, scale_min, S_world, keep is not None, dense)
        return verts

    @staticmethod
    def backward(ctx, g_verts):
        sq_eps, S, R6, T, trig, keep, Rw = ctx.saved_tensors
        ratio, scale_min, S_world, has_keep, dense = ctx.consts
        keep = keep if has_keep else None
        Kb, nv = trig.shape[1], trig.shape[2]
        gs = [ARENA.zeros_like(t) for t in (sq_eps, S, R6, T)]
        _lib.call('dbw_sq_blocks_bwd', _ptr(sq_eps), _ptr(S), _ptr(R6), _ptr(T), _ptr(trig), _ptr(keep), int(dense), Kb, nv, ratio, scale_min,
                  S_world, _ptr(Rw), _ptr(g_verts.contiguous()), *[_ptr(g) for g in gs], _stream(trig))
        return gs[0], gs[1], gs[2], gs[3], None, None, None, None


class _PosedMesh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, R6, T, base, S_world, Rw, Tw):
        r6, t = _chk(R6.detach(), torch.float32, 'R6'), _chk(T.detach(), torch.float32, 'T')
        nv = base.shape[0]
        verts = torch.empty(nv, 3, dtype=torch.float32, device=base.device)
        _lib.call('dbw_posed_mesh_fwd', _ptr(base), nv, _ptr(r6), _ptr(t), float(S_world), _ptr(Rw), _ptr(Tw), _ptr(verts), _stream(base))
        ctx.save_for_backward(r6, t, base, Rw)
        ctx.S_world = float(S_world)
        return verts

    @staticmethod
    def backward(ctx, g):
        r6, t, base, Rw = ctx.saved_tensors
        g6, gt = ARENA.zeros_like(r6), ARENA.zeros_like(t)
        _lib.call('dbw_posed_mesh_bwd', _ptr(base), base.shape[0], _ptr(r6), _ptr(t), ctx.S_world, _ptr(Rw), _ptr(g.contiguous()),
                  _ptr(g6), _ptr(gt), _stream(base))
        return g6, gt, None, None, None, None


def posed_mesh(R6, T, base, S_world, R_world, T_world):
    return _PosedMesh.apply(R6, T, base, S_world, R_world, T_world)


class _CompositeMSE(torch.autograd.Function):
    """loss = mean((imgs - (fg_rgb*mask + (1-mask)*env_rgb))^2) over `count` elements.  Forward: one streaming pass that only
    reduces; backward: one streaming pass that writes d/dfg and d/denv already scaled by the upstream gradient (read from
    device memory by the kernel -- no host sync, no extra elementwise multiply over the image-sized gradients)."""

    @staticmethod
    def forward(ctx, fg, env, imgs, count):
        N, _, H, W = fg.shape
        fg_c, env_c = _chk(fg.detach(), torch.float32, 'fg'), _chk(env.detach(), torch.float32, 'env')
        imgs = _chk(imgs, torch.float32, 'imgs')
        loss = torch.zeros(1, dtype=torch.float32, device=fg.device)
        _lib.call('dbw_composite_mse', _ptr(fg_c), _ptr(env_c), _ptr(imgs), N, H, W, 1.0 / count, 0, 0, _ptr(loss), 0, 0, _stream(fg))
        ctx.save_for_backward(fg_c, env_c, imgs)
        ctx.count = count
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        fg, env, imgs = ctx.saved_tensors
        N, _, H, W = fg.shape
        g_fg, g_env = torch.empty_like(fg), torch.empty_like(env)
        g = g.detach().to(torch.float32).reshape(1).contiguous()
        _lib.call('dbw_composite_mse', _ptr(fg), _ptr(env), _ptr(imgs), N, H, W, 1.0 / ctx.count, _ptr(g), 0, 0, _ptr(g_fg), _ptr(g_env),
                  _stream(fg))
        return g_fg, g_env, None, None


def composite_mse(fg, env, imgs, count=None):
    """fg (N,4,H,W), env (N,4,H,W), imgs (N,3,H,W) -> scalar MSE of the decoupled composite (dbw.py:223,366-367).
    `count` = number of elements of the GLOBAL batch (view-sharded data parallel), default this batch."""
    count = float(imgs.numel() if count is None else count)
    return _CompositeMSE.apply(fg, env, imgs, count)


def _upstream_scalar(g_value, device):
    """The gradient with respect to a composite's value as (1,) fp32 on the device; zero where nobody used the value."""
    if g_value is None:
        return torch.zeros(1, dtype=torch.float32, device=device)
    return g_value.detach().to(torch.float32).reshape(1).contiguous()


def _layer_args(fg, env, imgs, masks):
    """fg, env (N,4,H,W), imgs (N,3,H,W), masks (N,1,H,W) or None, fp32 on the GPU -> the four, contiguous."""
    fg_c, env_c, imgs_c = _chk(fg, torch.float32, 'fg'), _chk(env, torch.float32, 'env'), _chk(imgs, torch.float32, 'imgs')
    masks_c = None if masks is None else _chk(masks, torch.float32, 'masks')
    if fg_c.dim() != 4:
        raise ValueError(f'fg: (N,4,H,W), got {tuple(fg_c.shape)}')
    N, _, H, W = fg_c.shape
    if (tuple(fg_c.shape) != (N, 4, H, W) or fg_c.shape != env_c.shape or tuple(imgs_c.shape) != (N, 3, H, W)
            or (masks_c is not None and tuple(masks_c.shape) != (N, 1, H, W))):
        raise ValueError(f'fg, env (N,4,H,W), imgs (N,3,H,W), masks (N,1,H,W); got {tuple(fg_c.shape)}, {tuple(env_c.shape)}, '
                         f'{tuple(imgs_c.shape)}, {None if masks_c is None else tuple(masks_c.shape)}')
    return fg_c, env_c, imgs_c, masks_c


def _grad_args(upstream, grad_rec, fg):
    """upstream: one fp32 on the GPU, grad_rec: (N,3,H,W) for fg (N,4,H,W), or None -> the two, contiguous."""
    N, _, H, W = fg.shape
    up = _chk(upstream, torch.float32, 'upstream')
    g_rec = None if grad_rec is None else _chk(grad_rec, torch.float32, 'grad_rec')
    if up.numel() != 1 or (g_rec is not None and tuple(g_rec.shape) != (N, 3, H, W)):
        raise ValueError('upstream: one fp32, grad_rec: (N,3,H,W)')
    return up, g_rec


class _CompositeMSEMasked(torch.autograd.Function):
    """(weight * sum masks (rec - imgs)^2 / count, rec) of the decoupled composite as ONE node with two outputs: the forward is
    dbw_monitor_masked_composite (rec and the fp64 value, fixed-order reduction), the backward ONE launch of it fed by both incoming
    gradients -- the scalar's, read from device memory, and the gradient other terms send to rec (the perceptual term)."""

    @staticmethod
    def forward(ctx, fg, env, imgs, masks, scale):
        value, rec, saved = masked_composite_fwd(fg.detach(), env.detach(), imgs, masks, scale)
        ctx.set_materialize_grads(False)             # an output nobody used arrives as None, not as an image of zeros to read
        ctx.save_for_backward(*saved)
        ctx.scale = scale
        return value[0].to(torch.float32), rec

    @staticmethod
    def backward(ctx, g_value, g_rec):
        fg, env, imgs, masks = ctx.saved_tensors
        g_fg, g_env = masked_composite_bwd(fg, env, imgs, masks, ctx.scale, _upstream_scalar(g_value, fg.device),
                                           None if g_rec is None else g_rec.detach())
        return g_fg, g_env, None, None, None


def masked_composite_fwd(fg, env, imgs, masks, scale):
    """The forward of dbw_monitor_masked_composite as it stands: fg, env (N,4,H,W), imgs (N,3,H,W), masks (N,1,H,W) fp32 on the GPU,
    scale = weight / count a host number -> (value (1,) fp64 = scale * sum masks (rec - imgs)^2, rec (N,3,H,W), the four inputs as the
    kernel read them).  Two launches on the current stream, no host read."""
    lib = _monitor_lib()
    fg_c, env_c, imgs_c, masks_c = _layer_args(fg, env, imgs, masks)
    N, _, H, W = fg_c.shape
    dev = fg_c.device
    rec = torch.empty(N, 3, H, W, dtype=torch.float32, device=dev)
    value = torch.zeros(1, dtype=torch.float64, device=dev)
    if N > 0:
        ws = torch.empty(lib.dbw_monitor_masked_composite_workspace_bytes(N, H, W) // 8, dtype=torch.float64, device=dev)
        _lib.call('dbw_monitor_masked_composite', _ptr(fg_c), _ptr(env_c), _ptr(imgs_c), _ptr(masks_c), N, H, W, float(scale), _ptr(ws), _ptr(rec),
                  _ptr(value), 0, 0, 0, 0, _stream(fg_c))
    return value, rec, (fg_c, env_c, imgs_c, masks_c)


def masked_composite_bwd(fg, env, imgs, masks, scale, upstream, grad_rec=None):
    """The backward of dbw_monitor_masked_composite as it stands, ONE launch: upstream (1,) fp32 on the GPU -- the gradient with respect
    to the value --, grad_rec (N,3,H,W) or None -- the gradient with respect to rec -- -> (grad_fg, grad_env) (N,4,H,W)."""
    _monitor_lib()
    fg, env, imgs, masks = (_chk(t, torch.float32, n) for t, n in ((fg, 'fg'), (env, 'env'), (imgs, 'imgs'), (masks, 'masks')))
    N, _, H, W = fg.shape
    up, g_rec = _grad_args(upstream, grad_rec, fg)
    g_fg, g_env = torch.empty_like(fg), torch.empty_like(env)
    if N > 0:
        _lib.call('dbw_monitor_masked_composite', _ptr(fg), _ptr(env), _ptr(imgs), _ptr(masks), N, H, W, float(scale), 0, 0, 0, _ptr(up),
                  _ptr(g_rec), _ptr(g_fg), _ptr(g_env), _stream(fg))
    return g_fg, g_env


def composite_mse_masked(fg, env, imgs, masks, weight, count):
    """fg, env (N,4,H,W), imgs (N,3,H,W), masks (N,1,H,W) weights in [0, 1], count = 3 * sum(masks) of the GLOBAL batch as a host number
    -> (weight * sum masks (rec - imgs)^2 / count: a scalar, 0 for count == 0; rec (N,3,H,W): the composite).  Both outputs are
    differentiable in fg and env; one HIP launch computes the gradients of whatever was built on the two."""
    count = float(count)
    return _CompositeMSEMasked.apply(fg, env, imgs, masks, float(weight) / count if count > 0 else 0.0)


class _CompositeMSEExposure(torch.autograd.Function):
    """(weight * sum masks (rec - imgs)^2 / count, rec) with rec = exp(g) * composite + b under the per-view exposure theta
    as ONE node with two outputs: the forward is dbw_monitor_exposure_composite (rec and the fp64 value), the backward its image launch
    and its finishing launch, fed by both incoming gradients; fg, env and theta receive gradients."""

    @staticmethod
    def forward(ctx, fg, env, imgs, masks, theta, ids, scale):
        value, rec, saved = exposure_composite_fwd(fg.detach(), env.detach(), imgs, masks, theta.detach(), ids, scale)
        ctx.set_materialize_grads(False)             # an output nobody used arrives as None, not as an image of zeros to read
        ctx.has_masks = masks is not None
        ctx.save_for_backward(*[t for t in saved if t is not None])
        ctx.scale = scale
        return value[0].to(torch.float32), rec

    @staticmethod
    def backward(ctx, g_value, g_rec):
        saved = list(ctx.saved_tensors)
        fg, env, imgs = saved[:3]
        masks = saved[3] if ctx.has_masks else None
        theta, ids = saved[-2:]
        g_fg, g_env, g_theta = exposure_composite_bwd(fg, env, imgs, masks, theta, ids, ctx.scale, _upstream_scalar(g_value, fg.device),
                                                      None if g_rec is None else g_rec.detach())
        return g_fg, g_env, None, None, g_theta, None, None


def _exposure_args(fg, env, imgs, masks, theta, ids):
    fg_c, env_c, imgs_c, masks_c = _layer_args(fg, env, imgs, masks)
    theta_c, ids_c = _chk(theta, torch.float32, 'theta'), _chk(ids, torch.int32, 'ids')
    N = fg_c.shape[0]
    if theta_c.dim() != 2 or theta_c.shape[1] != 6 or theta_c.shape[0] < 1 or tuple(ids_c.shape) != (N,):
        raise ValueError(f'theta (V,6) with V >= 1, ids ({N},); got {tuple(theta_c.shape)}, {tuple(ids_c.shape)}')
    return fg_c, env_c, imgs_c, masks_c, theta_c, ids_c


def exposure_composite_fwd(fg, env, imgs, masks, theta, ids, scale):
    """The forward of dbw_monitor_exposure_composite as it stands: fg, env (N,4,H,W), imgs (N,3,H,W), masks (N,1,H,W) or None, theta (V,6)
    fp32 and ids (N,) int32 on the GPU, scale = weight / count a host number -> (value (1,) fp64 = scale * sum masks (rec - imgs)^2,
    rec (N,3,H,W) = exp(g) * composite + b, the inputs as the kernel read them).  Two launches on the current stream, no host read."""
    lib = _monitor_lib()
    fg_c, env_c, imgs_c, masks_c, theta_c, ids_c = _exposure_args(fg, env, imgs, masks, theta, ids)
    N, _, H, W = fg_c.shape
    dev = fg_c.device
    rec = torch.empty(N, 3, H, W, dtype=torch.float32, device=dev)
    value = torch.zeros(1, dtype=torch.float64, device=dev)
    if N > 0:
        ws = torch.empty(lib.dbw_monitor_exposure_composite_workspace_bytes(N, H, W) // 8, dtype=torch.float64, device=dev)
        _lib.call('dbw_monitor_exposure_composite', _ptr(fg_c), _ptr(env_c), _ptr(imgs_c), _ptr(masks_c), _ptr(theta_c), _ptr(ids_c), N, H, W,
                  theta_c.shape[0], float(scale), _ptr(ws), _ptr(rec), _ptr(value), 0, 0, 0, 0, 0, _stream(fg_c))
    return value, rec, (fg_c, env_c, imgs_c, masks_c, theta_c, ids_c)


def exposure_composite_bwd(fg, env, imgs, masks, theta, ids, scale, upstream, grad_rec=None, grad_theta=None):
    """The backward of dbw_monitor_exposure_composite as it stands, two launches: upstream (1,) fp32 on the GPU -- the gradient with
    respect to the value --, grad_rec (N,3,H,W) or None -- the gradient with respect to rec -- -> (grad_fg, grad_env (N,4,H,W), grad_theta
    (V,6)).  grad_theta given: the rows ids of it are ADDED to, the others left alone; None: a table of zeros is made."""
    lib = _monitor_lib()
    fg, env, imgs, masks, theta, ids = _exposure_args(fg, env, imgs, masks, theta, ids)
    N, _, H, W = fg.shape
    up, g_rec = _grad_args(upstream, grad_rec, fg)
    if grad_theta is None:
        grad_theta = torch.zeros_like(theta)
    elif grad_theta.shape != theta.shape or grad_theta.dtype != torch.float32 or not grad_theta.is_contiguous() or not grad_theta.is_cuda:
        raise ValueError(f'grad_theta: a contiguous fp32 table of theta\'s shape {tuple(theta.shape)} on the GPU')
    g_fg, g_env = torch.empty_like(fg), torch.empty_like(env)
    if N > 0:
        ws = torch.empty(lib.dbw_monitor_exposure_composite_workspace_bytes(N, H, W) // 8, dtype=torch.float64, device=fg.device)
        _lib.call('dbw_monitor_exposure_composite', _ptr(fg), _ptr(env), _ptr(imgs), _ptr(masks), _ptr(theta), _ptr(ids), N, H, W, theta.shape[0],
                  float(scale), _ptr(ws), 0, 0, _ptr(up), _ptr(g_rec), _ptr(g_fg), _ptr(g_env), _ptr(grad_theta), _stream(fg))
    return g_fg, g_env, grad_theta


def _exposure_ids(ids, N, V, ids_host=None):
    """The batch's rows of theta as a contiguous int32 tensor.  Where the caller holds the same ids on the host (ids_host; the Trainer
    draws them there) they are checked without a wait for the device: distinct, inside [0, V).  Without ids_host nothing is read back:
    the kernels treat an id outside the table as theta = 0 and skip its gradient row."""
    if ids.numel() != N:
        raise ValueError(f'ids: one per view of the batch ({N}), got {ids.numel()}')
    if ids_host is not None:
        host = [int(i) for i in torch.as_tensor(ids_host).reshape(-1).tolist()]
        if len(host) != N:
            raise ValueError(f'ids_host: one per view of the batch ({N}), got {len(host)}')
        if len(set(host)) != len(host):
            raise ValueError(f'composite_mse_exposure: the view ids of a batch must be distinct, got {host}')
        if host and (min(host) < 0 or max(host) >= V):
            raise ValueError(f'composite_mse_exposure: view ids outside [0, {V}): {host}')
    return ids.reshape(-1).to(torch.int32).contiguous()


def composite_mse_exposure(fg, env, imgs, masks, weight, count, theta, ids, ids_host=None):
    """fg, env (N,4,H,W), imgs (N,3,H,W), masks (N,1,H,W) weights in [0, 1] or None (= ones), count = 3 * sum(masks) -- imgs.numel() without
    masks -- of the GLOBAL batch as a host number, theta (V,6) the per-view exposures, ids (N) the batch's rows of theta,
    distinct -> (weight * sum masks (rec - imgs)^2 / count: a scalar, 0 for count == 0; rec (N,3,H,W) = exp(g) * composite + b).  Both
    outputs are differentiable in fg, env and theta; one image launch and one finishing launch compute the gradients of whatever was
    built on the two.  ids_host: the same ids on the host, where the caller has them; the caller GUARANTEES that the two are equal."""
    count = float(count)
    ids = _exposure_ids(ids, fg.shape[0], theta.shape[0], ids_host).to(fg.device)
    return _CompositeMSEExposure.apply(fg, env, imgs, masks, theta, ids, float(weight) / count if count > 0 else 0.0)


def composite(fg, env):
    """rec = fg_rgb*mask + (1-mask)*env_rgb as an image (API-compat path for predict(); HIP forward, elementwise torch
    backward -- the training path uses composite_mse)."""
    return _Composite.apply(fg, env)


class _Composite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fg, env):
        N, _, H, W = fg.shape
        fg_c, env_c = _chk(fg.detach(), torch.float32, 'fg'), _chk(env.detach(), torch.float32, 'env')
        rec = torch.empty(N, 3, H, W, dtype=torch.float32, device=fg.device)
        _lib.call('dbw_composite_mse', _ptr(fg_c), _ptr(env_c), 0, N, H, W, 0.0, 0, _ptr(rec), 0, 0, 0, _stream(fg))
        ctx.save_for_backward(fg_c, env_c)
        return rec

    @staticmethod
    def backward(ctx, g):
        fg, env = ctx.saved_tensors
        mask = fg[:, 3:4]
        g_fg = torch.cat([g * mask, (g * (fg[:, :3] - env[:, :3])).sum(1, keepdim=True)], 1)
        g_env = torch.cat([g * (1 - mask), torch.zeros_like(mask)], 1)
        return g_fg, g_env


class _TV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, maps, wrap, scale):
        m = _chk(maps.detach(), torch.float32, 'maps')
        n, h, w, _ = m.shape
        loss = torch.zeros(1, dtype=torch.float32, device=m.device)
        g = torch.empty_like(m)
        _lib.call('dbw_tv_l2sq', _ptr(m), n, h, w, int(wrap), float(scale), _ptr(loss), _ptr(g), _stream(m))
        ctx.save_for_backward(g)
        return loss[0]

    @staticmethod
    def backward(ctx, go):
        (g,) = ctx.saved_tensors
        return g * go, None, None


def tv_l2sq(maps, wrap_x=False, scale=1.0):
    """sum-over-maps l2sq total variation (dbw.py:380-386, loss.py:46), forward + gradient in one kernel."""
    return _TV.apply(maps, bool(wrap_x), float(scale))


class _Overlap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sq_eps, S, R6, T, alpha, u, consts):
        ratio, scale_min, temp, thresh = consts
        args = [_chk(t.detach(), torch.float32, 'overlap param') for t in (sq_eps, S, R6, T, alpha)]
        Kb, npts = u.shape[0], u.shape[1]
        dev = u.device
        loss = torch.zeros(1, dtype=torch.float32, device=dev)
        gs = [torch.zeros_like(t) for t in args]
        ws = torch.zeros(Kb * 18, dtype=torch.float32, device=dev)
        _lib.call('dbw_overlap_loss', _ptr(u), npts, *[_ptr(a) for a in args], Kb, ratio, scale_min, temp, thresh, 1.0, _ptr(loss),
                  *[_ptr(g) for g in gs], _ptr(ws), _stream(u))
        ctx.save_for_backward(*gs)
        return loss[0]

    @staticmethod
    def backward(ctx, go):
        gs = ctx.saved_tensors
        return gs[0] * go, gs[1] * go, gs[2] * go, gs[3] * go, gs[4] * go, None, None


def overlap_loss(sq_eps, S, R6, T, alpha, u, ratio, scale_min, temperature=0.005, n_blocks=1.95):
    """dbw.py:389-405.  u (Kb,npts,3) uniform samples in [0,1)."""
    return _Overlap.apply(sq_eps, S, R6, T, alpha, _chk(u, torch.float32, 'u'), (float(ratio), float(scale_min), float(temperature), float(n_blocks)))


class _BlockAlpha(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logit, noise, noise_scale, thresh):
        lg = _chk(logit.detach(), torch.float32, 'alpha_logit')
        Kb = lg.numel()
        alpha, alpha_full = torch.empty_like(lg), torch.empty_like(lg)
        keep = torch.empty(Kb, dtype=torch.int32, device=lg.device)
        nz = None if noise is None else _chk(noise, torch.float32, 'noise')
        _lib.call('dbw_block_alpha_fwd', _ptr(lg), _ptr(nz), float(noise_scale), float(thresh), Kb, _ptr(alpha), _ptr(alpha_full),
                  _ptr(keep), _stream(lg))
        ctx.save_for_backward(alpha, keep)
        ctx.mark_non_differentiable(keep)
        return alpha, alpha_full, keep

    @staticmethod
    def backward(ctx, g_a, g_af, _):
        alpha, keep = ctx.saved_tensors
        g = torch.empty_like(alpha)
        _lib.call('dbw_block_alpha_bwd', _ptr(alpha), _ptr(keep), _ptr(None if g_a is None else g_a.contiguous()), 1,
                  _ptr(None if g_af is None else g_af.contiguous()), alpha.numel(), _ptr(g), _stream(alpha))
        return g, None, None, None


def block_alpha(alpha_logit, noise=None, noise_scale=0.0, mask_threshold=-1.0):
    """alpha = sigmoid(alpha_logit + noise_scale*noise); keep = sigmoid(alpha_logit) > mask_threshold (all ones when
    mask_threshold < 0); alpha_full = alpha * keep  (dbw.py:297-311) -> (alpha, alpha_full, keep int32) in one launch."""
    return _BlockAlpha.apply(alpha_logit, noise, float(noise_scale), float(mask_threshold))


class _FusedLosses(torch.autograd.Function):
    """[w_rgb * MSE(composite), parsimony, tv, overlap] as one autograd node: every term is a kernel that produces its value
    and its gradient in the same pass, the weights are folded into the kernels' scale arguments and all four values land in
    one 4-float tensor -- instead of ~45 scalar-sized torch launches (fills, weight multiplications, sums and their autograd
    mirrors).  A term whose weight is None / 0 is skipped (its slot stays 0 and it sends no gradient)."""

    @staticmethod
    def forward(ctx, fg, env, imgs, alpha_full, bkg_maps, blocks_maps, ground_maps, sq_eps, S, R6, T, u, cfg):
        dev = imgs.device
        out = torch.zeros(4, dtype=torch.float32, device=dev)
        ctx.has_rgb = fg is not None        # None: the reconstruction term comes from render_decoupled_mse, only the regularisers here
        saved = []
        if ctx.has_rgb:
            fg_c, env_c = _chk(fg.detach(), torch.float32, 'fg'), _chk(env.detach(), torch.float32, 'env')
            imgs = _chk(imgs, torch.float32, 'imgs')
            N, _, H, W = fg_c.shape
            ctx.rgb_scale = cfg['rgb'] / cfg['count']
            _lib.call('dbw_composite_mse', _ptr(fg_c), _ptr(env_c), _ptr(imgs), N, H, W, ctx.rgb_scale, 0, 0, _ptr(out), 0, 0, _stream(fg_c))
            saved = [fg_c, env_c, imgs]
        ctx.n_tv = 0
        g_alpha_p = g_alpha_o = None
        if cfg.get('parsimony') and alpha_full is not None:
            a = _chk(alpha_full.detach(), torch.float32, 'alpha')
            g_alpha_p = ARENA.zeros_like(a)
            _lib.call('dbw_sqrt_mean', _ptr(a), a.numel(), 1e-6, float(cfg['parsimony']), _ptr(out) + 4, _ptr(g_alpha_p), _stream(a))
        tv_grads = []
        for maps, wrap, scale in ((bkg_maps, False, cfg.get('tv')), (blocks_maps, True, cfg.get('tv')),
                                  (ground_maps, False, (cfg.get('tv') or 0.0) * cfg.get('tv_ground_factor', 1.0))):
            if scale and maps is not None:
                m = _chk(maps.detach(), torch.float32, 'maps')
                n, h, w, _ = m.shape
                g = torch.empty_like(m)
                _lib.call('dbw_tv_l2sq', _ptr(m), n, h, w, int(wrap), float(scale), _ptr(out) + 8, _ptr(g), _stream(m))
                tv_grads.append(g)
            else:
                tv_grads.append(None)
        ov_grads = [None] * 4
        if cfg.get('overlap') and u is not None:
            ratio, scale_min, temp, thresh = cfg['overlap_consts']
            args = [_chk(t.detach(), torch.float32, 'overlap param') for t in (sq_eps, S, R6, T, alpha_full)]
            Kb, npts = u.shape[0], u.shape[1]
            gs = [ARENA.zeros_like(t) for t in args]
            ws = ARENA.zeros(Kb * 18, torch.float32, dev)
            _lib.call('dbw_overlap_loss', _ptr(u), npts, *[_ptr(a) for a in args], Kb, ratio, scale_min, temp, thresh, float(cfg['overlap']),
                      _ptr(out) + 12, *[_ptr(g) for g in gs], _ptr(ws), _stream(u))
            ov_grads, g_alpha_o = gs[:4], gs[4]
        ctx.save_for_backward(*saved)
        ctx.grads = (g_alpha_p, tv_grads, ov_grads, g_alpha_o)
        ctx.count = cfg['count']
        return out

    @staticmethod
    def backward(ctx, go):
        g_alpha_p, tv_grads, ov_grads, g_alpha_o = ctx.grads
        ctx.grads = None
        go = go.detach().to(torch.float32).contiguous()
        g_fg = g_env = None
        if ctx.has_rgb:
            fg, env, imgs = ctx.saved_tensors
            N, _, H, W = fg.shape
        if ctx.has_rgb and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            g_fg, g_env = torch.empty_like(fg), torch.empty_like(env)
            _lib.call('dbw_composite_mse', _ptr(fg), _ptr(env), _ptr(imgs), N, H, W, ctx.rgb_scale, _ptr(go), 0, 0, _ptr(g_fg), _ptr(g_env),
                      _stream(fg))
        # the saved gradients assume an upstream gradient of 1 per slot: scale each group by its slot's gradient (one
        # multi-tensor launch per group)
        tv = [g for g in tv_grads if g is not None]
        if tv:
            torch._foreach_mul_(tv, go[2])
        ov = [g for g in list(ov_grads) + [g_alpha_o] if g is not None]
        if ov:
            torch._foreach_mul_(ov, go[3])
        g_alpha = g_alpha_o
        if g_alpha_p is not None:
            g_alpha = torch.addcmul(g_alpha_o, g_alpha_p, go[1]) if g_alpha_o is not None else g_alpha_p * go[1]
        return (g_fg, g_env, None, g_alpha, tv_grads[0], tv_grads[1], tv_grads[2], ov_grads[0], ov_grads[1], ov_grads[2], ov_grads[3],
                None, None)


def fused_losses(fg, env, imgs, alpha_full, bkg_maps, blocks_maps, ground_maps, sq_eps, S, R6, T, u, cfg):
    """-> (4,) tensor [rgb, parsimony, tv, overlap], each already multiplied by its weight (dbw.py:361-408).
    cfg: {'rgb': w, 'count': elements of the global batch, 'parsimony': w|None, 'tv': w|None, 'tv_ground_factor': f,
          'overlap': w|None, 'overlap_consts': (ratio, scale_min, temperature, n_blocks)}."""
    return _FusedLosses.apply(fg, env, imgs, alpha_full, bkg_maps, blocks_maps, ground_maps, sq_eps, S, R6, T, u, cfg)


def adam_step_groups_(param, grad, exp_avg, exp_avg_sq, group_end, lrs, step, betas=(0.9, 0.999), eps=1e-8, zero=None, skip=None):
    """One launch for parameter groups that lie back to back in one flat buffer and differ in learning rate (optimizer.py:10-17).
    zero: a uint8 device tensor the same launch clears (the zero arena of the next iteration, ZeroArena.end_step).
    skip: a one-float device tensor; != 0 at launch time -> nothing is updated, only `zero` is cleared (a voided C step, c_step.py)."""
    import ctypes
    n = len(lrs)
    ends = (ctypes.c_int64 * n)(*[int(e) for e in group_end])
    lr = (ctypes.c_float * n)(*[float(x) for x in lrs])
    zb = 0 if zero is None else (zero.numel() + 15) // 16 * 16
    _lib.call('dbw_adam_step_groups', _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), ends, lr, n, float(betas[0]),
              float(betas[1]), float(eps), int(step), _ptr(zero), zb, _ptr(skip), _stream(param))


def adam_step_(param, grad, exp_avg, exp_avg_sq, lr, step, betas=(0.9, 0.999), eps=1e-8):
    """In-place fused Adam on flat fp32 buffers (torch.optim.Adam defaults; optimizer.py:6-18)."""
    _lib.call('dbw_adam_step', _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), float(lr), float(betas[0]),
              float(betas[1]), float(eps), int(step), _stream(param))


# ------------------------------------------------- what the surface and free-space terms check and allocate alike (`what`: the term in the messages)
def _term_tensors(what, tensors, rows3):
    """tensors: (tensor or None, dtype, name), each a contiguous device tensor of that dtype; rows3: (tensor, 'name (n,3)'), each (n,3)."""
    for t, dt, name in tensors:
        if t is not None:
            _chk(t, dt, name)
            if not t.is_contiguous():
                raise RuntimeError(f'{what}: {name} must be contiguous')
    if any(t.dim() != 2 or t.shape[1] != 3 for t, _ in rows3):
        raise ValueError(f'{what}: {", ".join(n for _, n in rows3)} expected, got {", ".join(str(tuple(t.shape)) for t, _ in rows3)}')


def _term_workspace(size_fn_name, what, M, F_, V, G, segment, device):
    nbytes = getattr(_lib.family('eval'), size_fn_name)(int(M), int(F_), int(V), int(G), int(segment))
    if nbytes == 0:
        raise ValueError(f'{what}: sizes M={M}, F={F_}, V={V}, G={G}, segment={segment} are refused (include/dbw_eval.h)')
    return torch.empty((nbytes + 15) // 16 * 2, dtype=torch.float64, device=device)


def _term_faces_host(what, faces_host, faces):
    if faces_host is not None and (faces_host.dtype != torch.int32 or faces_host.is_cuda or not faces_host.is_contiguous() or faces_host.shape != faces.shape):
        raise ValueError(f'{what}: faces_host is a contiguous int32 CPU copy of faces')


def _term_grads_outputs(size_fn_name, what, records_fn, M, F_, V, G, A, segment, records, workspace, grad_out, device):
    """-> (grad_verts (V,3), grad_alpha (A,) or None), empty.  The backward's partials are the last part of the workspace and grow with the
    number of segments: a workspace that the forward sized for another segment length may be too small, and the kernels do not know its size."""
    need = getattr(_lib.family('eval'), size_fn_name)(int(M), int(F_), int(V), int(G), int(segment))
    if need == 0 or workspace.numel() * workspace.element_size() < need or not workspace.is_cuda:
        raise ValueError(f'{what}: the workspace has {workspace.numel() * workspace.element_size()} bytes, segment={segment} needs {need}: '
                         f'give {records_fn} the same segment')
    if tuple(records.shape) != (M, 4) or records.dtype != torch.int32 or not records.is_contiguous():
        raise ValueError(f'{what}: records (M,4) int32 of {records_fn} expected, got {tuple(records.shape)} {records.dtype}')
    if grad_out is not None:
        _chk(grad_out, torch.float32, 'grad_out')
    return torch.empty(V, 3, dtype=torch.float32, device=device), (torch.empty(A, dtype=torch.float32, device=device) if A else None)


# ---------------------------------------------------------------------------------------------------------------- the surface term
def _surface_args(points, verts, faces, face_group, group_keep, vert_alpha, vert_group, n_points, tau, back, back_count):
    _term_tensors('surface term', ((points, torch.float32, 'points'), (verts, torch.float32, 'verts'), (faces, torch.int32, 'faces'),
                                   (face_group, torch.int32, 'face_group'), (group_keep, torch.int32, 'group_keep'),
                                   (vert_alpha, torch.float32, 'vert_alpha'), (vert_group, torch.int32, 'vert_group')),
                  ((points, 'points (N,3)'), (verts, 'verts (V,3)'), (faces, 'faces (F,3)')))
    N, V, F_, G = points.shape[0], verts.shape[0], faces.shape[0], face_group.numel() - 1
    if group_keep is not None and group_keep.numel() != G:
        raise ValueError(f'surface term: group_keep has {group_keep.numel()} entries for {G} groups')
    if vert_group is not None and vert_group.numel() != V:
        raise ValueError(f'surface term: vert_group has {vert_group.numel()} entries for {V} vertices')
    if back > 0 and (vert_alpha is None or vert_group is None):
        raise ValueError('surface term: back > 0 needs vert_alpha and vert_group')
    A = 0 if vert_alpha is None else vert_alpha.numel()
    M = int(n_points) if n_points else N
    bc = 1.0
    if back > 0:
        # the definition's n_blocks * BNV.  Without the constant it is counted: the vertices that belong to a block -- one host read, which
        # a caller inside a training step avoids by passing back_count (the model does)
        bc = float(back_count) if back_count is not None else float(int((vert_group >= 0).sum()))
        if not bc > 0:
            raise ValueError('surface term: back > 0 needs block vertices (vert_group >= 0) or a positive back_count')
    return N, V, F_, G, A, M, bc


def surface_workspace(M, F_, V, G, segment, device):
    return _term_workspace('dbw_eval_surface_workspace_bytes', 'surface term', M, F_, V, G, segment, device)


def surface_records(points, verts, faces, face_group, group_keep, vert_alpha, vert_group, *, n_points, tau, back, seed, step, back_count=None,
                    cull=True, segment=0, faces_host=None):
    """dbw_eval_surface_fwd on device tensors, arguments as in include/dbw_eval.h -> (records (M,4) int32: d2 bits, face, u bits, v bits;
    value (2,) float64: the forward mean and the back mean; the workspace, which surface_grads reads).  back_count: the constant
    n_blocks * vertices per block (default: the vertices with vert_group >= 0, counted with one host read).  faces_host: an int32 CPU copy of faces, checked against V before the launch.  Everything is
    enqueued on the current stream; nothing is read by the host."""
    N, V, F_, G, A, M, bc = _surface_args(points, verts, faces, face_group, group_keep, vert_alpha, vert_group, n_points, tau, back, back_count)
    dev = points.device
    ws = surface_workspace(M, F_, V, G, segment, dev)
    records = torch.empty(M, 4, dtype=torch.int32, device=dev)
    value = torch.empty(2, dtype=torch.float64, device=dev)
    _term_faces_host('surface term', faces_host, faces)
    with torch.cuda.device(dev):
        _lib.call('dbw_eval_surface_fwd', _ptr(points), N, int(n_points or 0), int(seed), int(step), _ptr(verts), V, _ptr(faces), _ptr(faces_host), F_,
                  _ptr(face_group), _ptr(group_keep), G, _ptr(vert_alpha), _ptr(vert_group), A, bc, float(tau), float(back), int(bool(cull)),
                  _ptr(ws), _ptr(records), _ptr(value), _stream(points))
    return records, value, ws


def surface_grads(points, verts, faces, face_group, group_keep, vert_alpha, vert_group, records, workspace, *, n_points, tau, back, seed, step,
                  weight, grad_out=None, back_count=None, segment=0):
    """dbw_eval_surface_bwd on what surface_records left (same arguments, same segment) -> (grad_verts (V,3), grad_alpha (A,) or None), fp32,
    written whole.  grad_out: a one-element fp32 device tensor that multiplies both, or None."""
    N, V, F_, G, A, M, bc = _surface_args(points, verts, faces, face_group, group_keep, vert_alpha, vert_group, n_points, tau, back, back_count)
    g_verts, g_alpha = _term_grads_outputs('dbw_eval_surface_workspace_bytes', 'surface term', 'surface_records', M, F_, V, G, A, segment, records,
                                           workspace, grad_out, points.device)
    with torch.cuda.device(points.device):
        _lib.call('dbw_eval_surface_bwd', _ptr(points), N, int(n_points or 0), int(seed), int(step), _ptr(verts), V, _ptr(faces), F_, G, _ptr(vert_alpha),
                  _ptr(vert_group), A, bc, float(tau), float(back), float(weight), _ptr(grad_out), int(segment), _ptr(records), _ptr(workspace),
                  _ptr(g_verts), _ptr(g_alpha), _stream(points))
    return g_verts, g_alpha


class _SurfaceTerm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, vert_alpha, points, faces, face_group, group_keep, vert_group, kw):
        v = verts.detach().contiguous()
        a = None if vert_alpha is None else vert_alpha.detach().contiguous()
        records, value, ws = surface_records(points, v, faces, face_group, group_keep, a, vert_group, n_points=kw['n_points'], tau=kw['tau'],
                                             back=kw['back'], seed=kw['seed'], step=kw['step'], back_count=kw['back_count'], segment=kw['segment'])
        ctx.kw = kw
        ctx.save_for_backward(v, a, points, faces, face_group, group_keep, vert_group, records, ws)
        return ((value[0] + kw['back'] * value[1]) * kw['weight']).to(torch.float32)        # (fp64 on the device, rounded once)

    @staticmethod
    def backward(ctx, g):
        v, a, points, faces, face_group, group_keep, vert_group, records, ws = ctx.saved_tensors
        kw = ctx.kw
        g_verts, g_alpha = surface_grads(points, v, faces, face_group, group_keep, a, vert_group, records, ws, n_points=kw['n_points'], tau=kw['tau'],
                                         back=kw['back'], seed=kw['seed'], step=kw['step'], weight=kw['weight'],
                                         grad_out=g.detach().reshape(1).to(torch.float32).contiguous(), back_count=kw['back_count'], segment=kw['segment'])
        return g_verts, (g_alpha if (a is not None and ctx.needs_input_grad[1]) else None), None, None, None, None, None, None


def surface_term(points, verts, faces, face_group, group_keep, vert_alpha, vert_group, *, n_points, tau, back, seed, step, weight, back_count=None,
                 segment=0):
    """The surface term of DESIGN.md 6u as ONE autograd node:
        weight * [ (1/M) sum_i rho(d2(p_i, S)) + back * (1/back_count) sum_v a_k(v) rho(|x_v - nn_P(x_v)|^2) ],   rho(d2) = min(d2, tau^2)
    -> the fp32 scalar of the fp64 value; gradients to verts (V,3) and to vert_alpha (A,).  points (N,3): the cloud; n_points draws a step
    (0: all points in order), taken inside the kernels from (seed, step); faces (F,3) int32 in the groups face_group (G+1), of which
    group_keep (G, int32 or None) drops some; vert_group (V) int32: the row of vert_alpha of a block vertex, -1 for any other vertex;
    back_count: n_blocks * vertices per block (default: the vertices with vert_group >= 0, counted with one host read).  Parts: surface_records, surface_grads."""
    if back_count is None and back > 0 and vert_group is not None:
        back_count = float(int((vert_group >= 0).sum()))
    kw = dict(n_points=int(n_points or 0), tau=float(tau), back=float(back), seed=int(seed), step=int(step), weight=float(weight),
              back_count=back_count, segment=int(segment))
    return _SurfaceTerm.apply(verts, vert_alpha, points, faces, face_group, group_keep, vert_group, kw)


# ---------------------------------------------------------------------------------------------------------------- the free-space term
FREESPACE_STREAM = 3        # csrc/freespace_math.h
FREESPACE_GRAZE = 2.0 ** -16


def _freespace_args(ends, frame, origins, verts, faces, face_group, group_keep, group_alpha, vert_alpha, n_rays):
    _term_tensors('free-space term', ((ends, torch.float32, 'ends'), (frame, torch.int32, 'frame'), (origins, torch.float32, 'origins'),
                                      (verts, torch.float32, 'verts'), (faces, torch.int32, 'faces'), (face_group, torch.int32, 'face_group'),
                                      (group_keep, torch.int32, 'group_keep'), (group_alpha, torch.int32, 'group_alpha'),
                                      (vert_alpha, torch.float32, 'vert_alpha')),
                  ((ends, 'ends (Nr,3)'), (origins, 'origins (Nf,3)'), (verts, 'verts (V,3)'), (faces, 'faces (F,3)')))
    Nr, Nf, V, F_, G = ends.shape[0], origins.shape[0], verts.shape[0], faces.shape[0], face_group.numel() - 1
    if frame.numel() != Nr:
        raise ValueError(f'free-space term: frame has {frame.numel()} entries for {Nr} rays')
    if group_keep is not None and group_keep.numel() != G:
        raise ValueError(f'free-space term: group_keep has {group_keep.numel()} entries for {G} groups')
    if group_alpha.numel() != G:
        raise ValueError(f'free-space term: group_alpha has {group_alpha.numel()} entries for {G} groups')
    A = 0 if vert_alpha is None else vert_alpha.numel()
    M = int(n_rays) if n_rays else Nr
    return Nr, Nf, V, F_, G, A, M


def freespace_workspace(M, F_, V, G, segment, device):
    return _term_workspace('dbw_eval_freespace_workspace_bytes', 'free-space term', M, F_, V, G, segment, device)


def freespace_records(ends, frame, origins, verts, faces, face_group, group_keep, group_alpha, vert_alpha, *, n_rays, tau, margin, seed, step,
                      cull=False, segment=0, faces_host=None, layout=0):
    """dbw_eval_freespace_fwd on device tensors, arguments as in include/dbw_eval.h -> (records (M,4) int32: t bits, face, u bits, v bits;
    value (1,) float64: the mean of a psi; the workspace, which freespace_grads reads).  faces_host: an int32 CPU copy of faces, checked
    against V before the launch.  cull: the slab test per group, off by default -- in the default layout it costs a few percent more than it
    saves (profiles/freespace_term.md), and without it the records hold for any mesh, not only under the condition of DESIGN.md 6v.
    layout: the forward's schedule (0: the default; 1: a workgroup per 256 rays walks every face; 2: a grid
    of ray tiles x face chunks with an integer atomic minimum) -- the same bytes.  Everything is enqueued on the current stream; nothing is
    read by the host."""
    Nr, Nf, V, F_, G, A, M = _freespace_args(ends, frame, origins, verts, faces, face_group, group_keep, group_alpha, vert_alpha, n_rays)
    dev = ends.device
    ws = freespace_workspace(M, F_, V, G, segment, dev)
    records = torch.empty(M, 4, dtype=torch.int32, device=dev)
    value = torch.empty(1, dtype=torch.float64, device=dev)
    _term_faces_host('free-space term', faces_host, faces)
    with torch.cuda.device(dev):
        _lib.call('dbw_eval_freespace_fwd', _ptr(ends), _ptr(frame), _ptr(origins), Nr, Nf, int(n_rays or 0), int(seed), int(step), _ptr(verts), V,
                  _ptr(faces), _ptr(faces_host), F_, _ptr(face_group), _ptr(group_keep), _ptr(group_alpha), G, _ptr(vert_alpha), A, float(tau),
                  float(margin), int(bool(cull)), int(layout), _ptr(ws), _ptr(records), _ptr(value), _stream(ends))
    return records, value, ws


def freespace_grads(ends, frame, origins, verts, faces, face_group, group_keep, group_alpha, vert_alpha, records, workspace, *, n_rays, tau, margin,
                    seed, step, weight, grad_out=None, segment=0):
    """dbw_eval_freespace_bwd on what freespace_records left (same arguments, same segment) -> (grad_verts (V,3), grad_alpha (A,) or None),
    fp32, written whole.  grad_out: a one-element fp32 device tensor that multiplies both, or None."""
    Nr, Nf, V, F_, G, A, M = _freespace_args(ends, frame, origins, verts, faces, face_group, group_keep, group_alpha, vert_alpha, n_rays)
    g_verts, g_alpha = _term_grads_outputs('dbw_eval_freespace_workspace_bytes', 'free-space term', 'freespace_records', M, F_, V, G, A, segment,
                                           records, workspace, grad_out, ends.device)
    with torch.cuda.device(ends.device):
        _lib.call('dbw_eval_freespace_bwd', _ptr(ends), _ptr(frame), _ptr(origins), Nr, Nf, int(n_rays or 0), int(seed), int(step), _ptr(verts), V,
                  _ptr(faces), F_, G, _ptr(vert_alpha), A, float(tau), float(margin), float(weight), _ptr(grad_out), int(segment), _ptr(records),
                  _ptr(workspace), _ptr(g_verts), _ptr(g_alpha), _stream(ends))
    return g_verts, g_alpha


class _FreespaceTerm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, vert_alpha, ends, frame, origins, faces, face_group, group_keep, group_alpha, kw):
        v = verts.detach().contiguous()
        a = None if vert_alpha is None else vert_alpha.detach().contiguous()
        records, value, ws = freespace_records(ends, frame, origins, v, faces, face_group, group_keep, group_alpha, a, n_rays=kw['n_rays'], tau=kw['tau'],
                                               margin=kw['margin'], seed=kw['seed'], step=kw['step'], segment=kw['segment'])
        ctx.kw = kw
        ctx.save_for_backward(v, a, ends, frame, origins, faces, face_group, group_keep, group_alpha, records, ws)
        return (value[0] * kw['weight']).to(torch.float32)        # (fp64 on the device, rounded once)

    @staticmethod
    def backward(ctx, g):
        v, a, ends, frame, origins, faces, face_group, group_keep, group_alpha, records, ws = ctx.saved_tensors
        kw = ctx.kw
        g_verts, g_alpha = freespace_grads(ends, frame, origins, v, faces, face_group, group_keep, group_alpha, a, records, ws, n_rays=kw['n_rays'],
                                           tau=kw['tau'], margin=kw['margin'], seed=kw['seed'], step=kw['step'], weight=kw['weight'],
                                           grad_out=g.detach().reshape(1).to(torch.float32).contiguous(), segment=kw['segment'])
        return (g_verts, (g_alpha if (a is not None and ctx.needs_input_grad[1]) else None)) + (None,) * 8


def freespace_term(ends, frame, origins, verts, faces, face_group, group_keep, group_alpha, vert_alpha, *, n_rays, tau, margin, seed, step, weight,
                   segment=0):
    """The free-space term of DESIGN.md 6v as ONE autograd node:
        weight * (1/M) sum_i a_{k(i)} psi(g_i),   g_i = (1 - t*_i) l_i - margin,   psi(g) = 0 | g^2 | tau (2 g - tau)
    -> the fp32 scalar of the fp64 value; gradients to verts (V,3) and to vert_alpha (A,).  Ray j runs from origins[frame[j]] to ends[j];
    n_rays draws a step (0: all rays in order), taken inside the kernels from (seed, step); t* is the first hit of the ray with the faces
    (F,3) int32 of the groups face_group (G+1) that group_keep (G, int32 or None) keeps; group_alpha (G) int32: a group's row of vert_alpha,
    -1 for the ground (a = 1).  Parts: freespace_records, freespace_grads."""
    kw = dict(n_rays=int(n_rays or 0), tau=float(tau), margin=float(margin), seed=int(seed), step=int(step), weight=float(weight), segment=int(segment))
    return _FreespaceTerm.apply(verts, vert_alpha, ends, frame, origins, faces, face_group, group_keep, group_alpha, kw)


def freespace_draw(seed, step, n_rays, n_total):
    """The ray indices a step draws (csrc/freespace_math.h: freespace_draw_index), on the host: word 0 of Philox4x32-10 with counter
    (i, 3, step) and key seed, mod the number of rays -> (n_rays,) int64."""
    i = np.arange(int(n_rays), dtype=np.uint64)
    c = [i, np.full_like(i, FREESPACE_STREAM), np.full_like(i, int(step) & 0xffffffff), np.full_like(i, (int(step) >> 32) & 0xffffffff)]
    k = [np.uint64(int(seed) & 0xffffffff), np.uint64((int(seed) >> 32) & 0xffffffff)]
    m32 = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k[0]) & m32, p1 & m32, ((p0 >> np.uint64(32)) ^ c[3] ^ k[1]) & m32, p0 & m32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & m32, (k[1] + np.uint64(0xBB67AE85)) & m32]
    return torch.from_numpy((c[0] % np.uint64(int(n_total))).astype(np.int64))


def freespace_first_hits(o, e, tri):
    """o, e (n,3), tri (F,3,3) -> (t (n,F), u, v, candidate (n,F) bool): Moeller-Trumbore of DESIGN.md 6v for every ray and face, in the
    tensors' dtype; t, u, v are only meaningful where candidate is set."""
    a = tri[None, :, 0]
    e1, e2 = tri[None, :, 1] - a, tri[None, :, 2] - a
    n = torch.linalg.cross(e1, e2)
    eb = e[:, None, :]
    det = -(n * eb).sum(-1)
    ok = det * det > FREESPACE_GRAZE * (n * n).sum(-1) * (eb * eb).sum(-1)
    den = torch.where(ok, det, torch.ones_like(det))
    h = torch.linalg.cross(eb.expand(-1, tri.shape[0], -1), e2.expand(e.shape[0], -1, -1))
    s = o[:, None, :] - a
    q = torch.linalg.cross(s, e1.expand_as(s))
    u, v, t = (s * h).sum(-1) / den, (eb * q).sum(-1) / den, (e2 * q).sum(-1) / den
    return t, u, v, ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < 1)


def freespace_term_torch(ends, frame, origins, verts, faces, face_group, group_keep, group_alpha, vert_alpha, *, n_rays, tau, margin, seed, step,
                         weight, chunk=1024):
    """ops.freespace_term in torch, in the dtype of verts, on any device: the readable statement of DESIGN.md 6v, the timing baseline of
    tools/freespace_bench.py and, in float64, the gradient reference of the tests.  The first hit is selected without a graph; t* of the
    selected face is then formed again from the vertices, so autograd differentiates the intersection itself."""
    dt, dev = verts.dtype, verts.device
    P, O = ends.to(device=dev, dtype=dt), origins.to(device=dev, dtype=dt)
    Nr, G = P.shape[0], face_group.numel() - 1
    idx = freespace_draw(seed, step, n_rays, Nr).to(dev) if n_rays else torch.arange(Nr, device=dev)
    counts = (face_group[1:] - face_group[:-1]).to(torch.int64)
    fgroup = torch.repeat_interleave(torch.arange(G, device=dev), counts.to(dev), output_size=faces.shape[0])
    fk = torch.ones(faces.shape[0], dtype=torch.bool, device=dev) if group_keep is None else group_keep.to(dev).to(torch.bool)[fgroup]
    fid = fk.nonzero().flatten()
    fc = faces.to(torch.int64)[fid]
    row = group_alpha.to(dev).to(torch.int64)[fgroup[fid]]
    ones = verts.new_ones(1)
    alpha = ones if vert_alpha is None else torch.cat([vert_alpha.to(dt), ones])        # (row -1: the ground's 1)
    fr = frame.to(dev).to(torch.int64)[idx]
    valid = (fr >= 0) & (fr < O.shape[0])
    idx, fr = idx[valid], fr[valid]
    total = verts.new_zeros(())
    for s0 in range(0, idx.shape[0], chunk):
        p, o = P[idx[s0:s0 + chunk]], O[fr[s0:s0 + chunk]]
        e = p - o
        with torch.no_grad():
            t, _, _, cand = freespace_first_hits(o, e, verts.detach()[fc])
            t = torch.where(cand, t, torch.full_like(t, float('inf')))
            j = t.argmin(1)
            hit = cand.any(1)
        if not bool(hit.any()):
            continue
        o, e, j = o[hit], e[hit], j[hit]
        tri = verts[fc[j]]
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        n = torch.linalg.cross(e1, e2)
        ts = (n * (tri[:, 0] - o)).sum(-1) / (n * e).sum(-1)
        g = (1 - ts) * e.norm(dim=-1) - float(margin)
        psi = torch.where(g <= 0, torch.zeros_like(g), torch.where(g <= tau, g * g, float(tau) * (2 * g - float(tau))))
        total = total + (alpha[row[j]] * psi).sum()
    M = int(n_rays) if n_rays else Nr
    return float(weight) * total / M
