/*
 * dbw_viz.h -- C ABI of the lit visualisation renders of libdbw_hip.so: the forward-only render pass with a directional light and flat
 * or Phong shading (the reference's `renderer_light`, src/model/dbw.py:139-143, and the eye_light variants of render_views /
 * render_rotated_views, src/model/renderer.py:290-380).  Python side: dbw_amd/ops.py (render_scene_lit), bound through
 * _lib.VIZ_SIGNATURES.  The arithmetic is csrc/light_math.h.
 *
 * Conventions are those of dbw_hip.h: DEVICE pointers owned by the caller, contiguous, unless said otherwise; return 0 or a negative
 * DBW_ERR_*, the text in dbw_last_error(); arguments are validated before any launch; kernels are enqueued on `stream`, no host
 * synchronisation.
 */
#ifndef DBW_VIZ_H
#define DBW_VIZ_H
#include "dbw_hip.h"

/* ABI revision of this header (dbw_viz_abi_version() returns the value the library was built with).  The scene parsing entry points
 * (dbw_viz_parse_*) were ADDED under revision 1: nothing that existed changed its meaning or its layout, so the number stays. */
#define DBW_VIZ_ABI_VERSION 1

/* Scene parsing: labels are 0 .. DBW_VIZ_MAX_LABELS - 1 (one bit of the coverage word each); DBW_VIZ_NO_LABEL marks a pixel no face covers. */
#define DBW_VIZ_MAX_LABELS 64
#define DBW_VIZ_NO_LABEL 255

#ifdef __cplusplus
extern "C" {
#endif

int dbw_viz_abi_version(void);

/* Area-weighted vertex normals (PyTorch3D's verts_normals_packed): normals[v] = normalize(sum over the (face, corner) pairs incident to v
 * of the unnormalised cross product of the face taken at that corner), norm clamped at 1e-6.  verts (V,3) fp32 world vertices, faces
 * (F,3) int32.  The adjacency is CSR: adj_start (V+1) int32 ascending with adj_start[0] == 0, adj (adj_start[V]) int32 entries
 * face * 4 + corner -- built once per topology by the caller.  The sum runs in the order of `adj` (a gather, no floating-point atomics:
 * two calls on the same input are bit-equal).  normals (V,3) fp32; a vertex without faces gets (0, 0, 0). */
int dbw_vertex_normals(const float *verts, const int32_t *faces, const int32_t *adj_start, const int32_t *adj, int V, int F, float *normals,
                       dbw_stream_t stream);

/* Bytes of workspace dbw_render_lit_fwd needs: the rasteriser's binned workspace at the RENDER size (ssaa*H x ssaa*W) and the per-(view,
 * face) light records.  0 for arguments the render call would refuse. */
size_t dbw_render_lit_workspace_bytes(int64_t F_total, int N, int F, int H, int W, int ssaa);

/* One lit render pass, forward only: per-face set-up and bins, tile rasterisation, per-pixel top-K, texture fetch, lighting, layered
 * blend -- and, with ssaa == 4, the 4x4 box filter -- in one kernel that stores nothing but the image.
 *   face_verts_c ... alpha_len: the geometry, clip tables and texture tables of dbw_render_fwd_fused (same meaning, same layout);
 *   verts_world (V,3) fp32, faces (F,3) int32: the scene the clipped faces came from (face normals are those of the ORIGINAL faces);
 *   vert_normals (V,3) fp32 from dbw_vertex_normals: Phong shading; NULL: flat shading;
 *   light_dir_world (N,3) fp32: per view, the direction FROM the surface TO the light in world space (direction @ R^T: the light is
 *     fixed to the camera), any length -- normalised here with the norm clamped at 1e-6;
 *   ambient3, diffuse3, background3: HOST pointers to 3 floats each;
 *   colour of a fragment = (ambient + diffuse * relu(n . d)) * texel, blended like dbw_render_fwd_fused blends the texel;
 *   N views, F_total = rows of face_verts_c, K = faces_per_pixel (<= DBW_MAX_FACES_PER_PIXEL), F = faces of the scene, sigma / blur_radius
 *     / perspective_correct as in dbw_render_fwd_fused;
 *   H, W: the OUTPUT size.  ssaa == 1: rendered at H x W.  ssaa == 4: rendered at 4H x 4W and every 4x4 block averaged in registers
 *     (premultiplied RGB and alpha alike); K == 1 only, DBW_ERR_UNSUPPORTED otherwise;
 *   image (N,4,H,W) fp32 out;
 *   workspace: 256-byte aligned, at least dbw_render_lit_workspace_bytes(F_total, N, F, H, W, ssaa) bytes. */
int dbw_render_lit_fwd(const float *face_verts_c, const int32_t *first_idx, const int32_t *num_faces, const int32_t *neighbor,
                       const int32_t *c2o, const int32_t *clip_code, const float *clip_w, int Fc_stride, const float *face_uvs,
                       const int32_t *face_map, const int32_t *map_desc, const float *maps, const float *faces_alpha, int alpha_len,
                       const float *verts_world, const int32_t *faces, const float *vert_normals, const float *light_dir_world,
                       const float *ambient3, const float *diffuse3, int N, int64_t F_total, int H, int W, int K, int F, float sigma,
                       float blur_radius, int perspective_correct, const float *background3, int ssaa, float *image, void *workspace,
                       size_t workspace_bytes, dbw_stream_t stream);

/* Bytes of workspace dbw_viz_parse_fwd needs: the rasteriser's binned workspace at H x W and one label per clipped face.  0 for arguments
 * the call would refuse. */
size_t dbw_viz_parse_workspace_bytes(int64_t F_total, int N, int F, int H, int W);

/* Scene parsing maps, one forward-only pass: which labelled part of the scene every pixel SEES, how far away it is, and every label that
 * COVERS the pixel, occluded or not (amodal masks).  Hard rasterisation (sigma = 0, blur_radius = 0), no culling; the inside test, the depth
 * and the order of the faces are the rasteriser's own ((pz, face index), dbw_rasterize_fwd with K = 1 and clipped barycentrics).
 *   face_verts_c ... c2o, Fc_stride, N, F_total, H, W, F, perspective_correct: as in dbw_render_lit_fwd (c2o NULL: an unclipped table of
 *     N * F faces); N, H, W > 0;
 *   face_label (F) int32: one label in [0, DBW_VIZ_MAX_LABELS) per ORIGINAL face; clipped face f has the label of face c2o[f];
 *   face_label_host: NULL, or a HOST copy of face_label.  The labels are validated on that copy, before any launch (an entry outside
 *     [0, 64): DBW_ERR_INVALID); the device table is never read back.  With NULL the caller vouches for the table (ops.parse_scene always
 *     passes the copy it built the device table from); an unchecked label is taken modulo 64 and nothing is accessed out of bounds;
 *   label  (N,H,W) uint8 out: label of the nearest face, DBW_VIZ_NO_LABEL where no face passes;
 *   depth  (N,H,W) fp32 out: view-space z of the nearest face -- what zbuf[..., 0] of dbw_rasterize_fwd holds -- or -1;
 *   cover  (N,H,W) int64 out: bit l = some face with label l passes the inside test at the pixel (bit 63 is the sign bit);
 *   counts (N,DBW_VIZ_MAX_LABELS,2) int32 out: per view and label [pixels covered (amodal area), pixels where it is the nearest (visible
 *     area)].  Zeroed on `stream` by the call, summed with integer atomics: two calls are bit-equal;
 *   workspace: 256-byte aligned, at least dbw_viz_parse_workspace_bytes(F_total, N, F, H, W) bytes. */
int dbw_viz_parse_fwd(const float *face_verts_c, const int32_t *first_idx, const int32_t *num_faces, const int32_t *neighbor,
                      const int32_t *c2o, int Fc_stride, int N, int64_t F_total, int H, int W, int F, int perspective_correct,
                      const int32_t *face_label, const int32_t *face_label_host, uint8_t *label, float *depth, int64_t *cover,
                      int32_t *counts, void *workspace, size_t workspace_bytes, dbw_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
