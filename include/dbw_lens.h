/*
 * dbw_lens.h -- C ABI of the camera of a custom capture in libdbw_hip.so: its lens and its pose.
 * Lens: raw 8-bit frames, resident on the device, resampled from the distorted image of an OpenCV radial-tangential lens (the k1..k4, p1,
 * p2 of a Nerfstudio transforms.json) into the pinhole frame the renderer assumes, before the image ingest (dbw_ingest.h) resizes them.
 * Pose: the gradient of a render with respect to each view's R and T, and the per-view 6-vector that refines a pose during training.
 * A capture whose frames have a camera each, or a fisheye lens, is rectified frame by frame into one pinhole (dbw_lens_rectify_u8).
 * Intrinsics: the gradient of a render with respect to the pinhole matrix the views share, and the 4-vector that refines it.
 * Python side: dbw_amd/ops.py (undistort_u8, lens_valid_u8, rectify_u8, rectify_valid_u8, project_clip_bwd_cam, pose_apply,
 * project_clip_bwd_k, intrinsics_apply), bound through _lib.LENS_SIGNATURES and
 * _lib.LENS_OTHER_SIGNATURES.  The arithmetic is csrc/lens_math.h, csrc/pose_math.h and csrc/intrinsics_math.h.
 *
 * Conventions are those of dbw_hip.h: DEVICE pointers owned by the caller, contiguous, unless said otherwise; return 0 or a negative
 * DBW_ERR_*, the text in dbw_last_error(); arguments are validated before any launch; kernels are enqueued on `stream`, no host
 * synchronisation.
 */
#ifndef DBW_LENS_H
#define DBW_LENS_H
#include "dbw_hip.h"

/* ABI revision of this header (dbw_lens_abi_version() returns the value the library was built with). */
#define DBW_LENS_ABI_VERSION 1

/* Number of floats of the `lens` array. */
#define DBW_LENS_N_PARAMS 12

#ifdef __cplusplus
extern "C" {
#endif

int dbw_lens_abi_version(void);

/* src (N,H,W,3) uint8 -> out (N,H,W,3) uint8, both on the DEVICE; they must not overlap (DBW_ERR_INVALID).  N >= 1, H >= 2, W >= 2.
 * lens: a HOST array of DBW_LENS_N_PARAMS floats [fx, fy, cx, cy, inv_zfx, inv_zfy, k1, k2, k3, k4, p1, p2], read before the call
 * returns: focal lengths and principal point of the source frames in pixels (pixel centres at +0.5), the reciprocals 1 / (zoom * fx) and
 * 1 / (zoom * fy) of the output's focal lengths, and the distortion coefficients.  Output pixel (i, j) is the bilinear sample of its
 * frame at
 *   x = (j + 0.5 - cx) * inv_zfx, y = (i + 0.5 - cy) * inv_zfy, r2 = x*x + y*y, d = 1 + r2*(k1 + r2*(k2 + r2*(k3 + r2*k4))),
 *   u = (x*d + 2*p1*x*y + p2*(r2 + 2*x*x)) * fx + cx - 0.5,  v = (y*d + 2*p2*x*y + p1*(r2 + 2*y*y)) * fy + cy - 0.5,
 * clamped to the frame, in fp32 and rounded half up (csrc/lens_math.h has the order of the operations).  The same map serves all N
 * frames.  Output rows leave as dwords where their addresses allow it and byte by byte at their ends: any alignment of src and out and
 * any W give the same bytes. */
int dbw_images_undistort_u8(const uint8_t *src, int N, int H, int W, const float *lens, uint8_t *out, dbw_stream_t stream);

/* The validity map of a rectified frame, added under revision 1 of this header.  out (H,W) uint8 on the DEVICE: 255 where output pixel
 * (i, j) reads inside the source frame -- 0 <= u <= W - 1 and 0 <= v <= H - 1 for the (u, v) above, NOT clamped --, 0 elsewhere and for
 * a NaN coordinate.  lens: the HOST array of dbw_images_undistort_u8.  One map serves every frame of a scene: with it as a mask of the
 * loss the frames need no zoom that crops the border away.  H >= 1, W >= 1. */
int dbw_lens_valid_u8(int H, int W, const float *lens, uint8_t *out, dbw_stream_t stream);

/* Frames with a camera each, rectified to one pinhole: added under revision 1 of this header.  Number of floats of a row of `cams`. */
#define DBW_LENS_RECT_N_PARAMS 16

/* src (N,H,W,3) uint8 -> out (N,H,W,3) uint8, both on the DEVICE; they must not overlap (DBW_ERR_INVALID).  N >= 1, H >= 2, W >= 2.
 * cams: a HOST array of N * DBW_LENS_RECT_N_PARAMS floats, one row per frame of the chunk in the chunk's order:
 * [model, fx, fy, cx, cy, k1, k2, k3, k4, p1, p2, 0, 0, 0, 0, 0] -- model 0: OpenCV's radial-tangential lens (the one of
 * dbw_images_undistort_u8; a pinhole where the coefficients are 0), model 1: OpenCV's fisheye lens (k1..k4; p1, p2 are not read) --, focal
 * lengths and principal point of THAT frame in pixels (pixel centres at +0.5).  target: a HOST array of 4 floats [cx0, cy0, 1/fx0, 1/fy0],
 * the pinhole camera every frame is resampled into, the reciprocals rounded once from fp64.  Both arrays are read before the call returns.
 * Output pixel (i, j) of frame n is the bilinear sample of that frame at
 *   x = (j + 0.5 - cx0) / fx0, y = (i + 0.5 - cy0) / fy0, r2 = x*x + y*y,
 *   model 0: (u, v) of dbw_images_undistort_u8 from (x, y, r2) on, with the frame's own coefficients, focal lengths and principal point
 *            (with cx0 = cx, cy0 = cy, 1/fx0 = inv_zfx, 1/fy0 = inv_zfy: the bytes of dbw_images_undistort_u8),
 *   model 1: r = sqrt(r2), th = atan(r), td = th*(1 + k1 th^2 + k2 th^4 + k3 th^6 + k4 th^8), s = td / r (1 where r2 == 0),
 *            u = x*s*fx + cx - 0.5, v = y*s*fy + cy - 0.5,
 * clamped to the frame, in fp32 and rounded half up; csrc/lens_math.h has the order of the operations and the arctangent, which is
 * written there from + - * / sqrt so that a host build gives the same bytes.  Refused before any launch (DBW_ERR_INVALID): a value of cams
 * (its padding too) or of target that is not finite, a model id other than 0 and 1, a focal length or a reciprocal that is not > 0.
 * The table travels in the arguments of the launches, 32 frames to a launch: no allocation, no copy, no synchronisation.  Any alignment
 * of src and out and any W give the same bytes. */
int dbw_lens_rectify_u8(const uint8_t *src, int N, int H, int W, const float *cams, const float *target, uint8_t *out, dbw_stream_t stream);

/* The validity maps of the frames dbw_lens_rectify_u8 makes from the same cams and target: out (N,H,W) uint8 on the DEVICE, 255 where
 * output pixel (i, j) of frame n reads inside its source frame -- 0 <= u <= W - 1 and 0 <= v <= H - 1, NOT clamped --, 0 elsewhere and
 * for a NaN coordinate.  The per-frame form of dbw_lens_valid_u8: what one source frame cannot fill of the common target is masked in
 * that frame alone.  N >= 1, H >= 1, W >= 1. */
int dbw_lens_rectify_valid_u8(int N, int H, int W, const float *cams, const float *target, uint8_t *out, dbw_stream_t stream);

/* Camera pose refinement, added under revision 1 of this header.  Conventions of the camera transform (dbw_project_clip_fwd): row vectors,
 * v = X.R + T, R (B,3,3) row-major, T (B,3).
 *
 * dbw_lens_pose_grad: the gradient of the clipped faces of B views with respect to each view's camera.  The arguments up to
 * grad_face_verts_c (B,2F,3,3) are those of dbw_project_clip_bwd, which sums the same per-slot gradient over the views into the vertices;
 * this call sums it over the slots j < num_faces[b] of view b into grad_R (B,3,3) and grad_T (B,3).  What grad_face_verts_c holds in the
 * other slots reaches nothing.  accumulate != 0: the sums are added to what grad_R, grad_T hold (a second pass over the same views), else
 * they replace it.  workspace: dbw_lens_pose_grad_workspace_bytes(B, F) bytes on the DEVICE, 4-byte aligned, contents irrelevant.  The
 * sums have a fixed order (no atomics): two calls give the same bits.  B >= 0 (B == 0: nothing is done), V > 0, F > 0, B <= 65535. */
size_t dbw_lens_pose_grad_workspace_bytes(int B, int F);
int dbw_lens_pose_grad(const float *verts_world, const int32_t *faces, const float *R, const float *T, const float *Kmat, int B, int V, int F,
                       float eps, float z_clip, int perspective_correct, const int32_t *num_faces, const int32_t *c2o,
                       const int32_t *clip_code, const float *clip_w, const float *grad_face_verts_c, void *workspace,
                       size_t workspace_bytes, float *grad_R, float *grad_T, int accumulate, dbw_stream_t stream);

/* The refined poses of a batch.  delta (V,6): one row (w, tau) per view of the scene; ids (B) int32: the row of each view of the batch.
 * R_out[b] = R0[b].E(w), T_out[b] = T0[b].E(w) + tau with E = exp([w]x) (csrc/pose_math.h has the sign convention and the series near
 * w = 0: a zero row gives R0[b], T0[b] bit for bit).  An id outside [0, V) leaves the pose as it is.  B >= 0, V > 0. */
int dbw_lens_pose_apply(const float *R0, const float *T0, const float *delta, const int32_t *ids, int B, int V, float *R_out, float *T_out,
                        dbw_stream_t stream);

/* Backward of dbw_lens_pose_apply with respect to delta: grad_R (B,3,3), grad_T (B,3) of the refined poses -> row ids[b] of grad_delta
 * (V,6), WRITTEN, not added: the caller zeroes the rows beforehand and passes ids that are distinct within the batch.  R0, T0 are data
 * and receive no gradient. */
int dbw_lens_pose_chain(const float *R0, const float *T0, const float *delta, const int32_t *ids, int B, int V, const float *grad_R,
                        const float *grad_T, float *grad_delta, dbw_stream_t stream);

/* Intrinsics refinement, added under revision 1 of this header (csrc/camera_grad.hip, arithmetic: csrc/intrinsics_math.h).  Kmat (4,4)
 * row-major is the pinhole matrix the views share: px, py, pw of a view-space point come from its rows 0, 1 and 3, row 2 is never read.
 *
 * dbw_lens_intrinsics_grad: the gradient of the clipped faces of B views with respect to Kmat.  The arguments up to workspace_bytes are
 * those of dbw_lens_pose_grad; the per-slot gradient is summed over the slots j < num_faces[b] of every view into grad_K (4,4), the full
 * gradient of the matrix (what autograd gives for it), row 2 zero.  What grad_face_verts_c holds in the other slots reaches nothing.
 * accumulate != 0: the sum is added to what grad_K holds (a second pass), else it replaces it.  workspace:
 * dbw_lens_intrinsics_grad_workspace_bytes(B, F) bytes on the DEVICE, 4-byte aligned, contents irrelevant.  The sum has a fixed order --
 * slots of a chunk of 256, then view-major over the chunks in fp64 -- and no atomics: two calls give the same bits.  B >= 0 (B == 0:
 * nothing is done), V > 0, F > 0, B <= 65535. */
size_t dbw_lens_intrinsics_grad_workspace_bytes(int B, int F);
int dbw_lens_intrinsics_grad(const float *verts_world, const int32_t *faces, const float *R, const float *T, const float *Kmat, int B, int V,
                             int F, float eps, float z_clip, int perspective_correct, const int32_t *num_faces, const int32_t *c2o,
                             const int32_t *clip_code, const float *clip_w, const float *grad_face_verts_c, void *workspace,
                             size_t workspace_bytes, float *grad_K, int accumulate, dbw_stream_t stream);

/* The refined matrix.  theta: 4 floats (a_x, a_y, c_x, c_y) on the DEVICE.  K_out = K0 except K_out[0] = K0[0] exp(a_x),
 * K_out[5] = K0[5] exp(a_y), K_out[2] = K0[2] + c_x, K_out[6] = K0[6] + c_y: a scale of each focal length and an offset of the principal
 * point in NDC units.  theta = 0 gives K0 bit for bit. */
int dbw_lens_intrinsics_apply(const float *K0, const float *theta, float *K_out, dbw_stream_t stream);

/* Backward of dbw_lens_intrinsics_apply with respect to theta: grad_K (4,4) of the refined matrix -> grad_theta (4), WRITTEN:
 * (grad_K[0] K_out[0], grad_K[5] K_out[5], grad_K[2], grad_K[6]).  K0 is data and receives no gradient. */
int dbw_lens_intrinsics_chain(const float *K0, const float *theta, const float *grad_K, float *grad_theta, dbw_stream_t stream);

/* The point cloud of a capture's depth maps, added under revision 1 of this header (csrc/depth_cloud.hip, arithmetic: csrc/depth_math.h).
 * depth (N,H,W) uint16 on the DEVICE, at any 2-byte alignment: one depth map per frame, at the maps' own resolution.  cams (N rows of
 * DBW_LENS_RECT_N_PARAMS floats) and target (4 floats) are the HOST arrays of dbw_lens_rectify_u8, with the intrinsics at the depth maps'
 * resolution; poses: a HOST array of N * 12 floats, a row [A (3x3 row-major), t] per frame, camera (x right, y down, z forward, in depth
 * units) to world: the caller folds the axis flip of its convention and the depth unit into A.  box: a HOST array of 4 floats
 * [lo_x, lo_y, lo_z, inv_step], inv_step = G * 1024 / (hi - lo) rounded once from fp64.  The four arrays are read before the call returns
 * and travel in the arguments of the launches, 16 frames to a launch: no allocation, no copy, no synchronisation.
 * Target pixel (i, j) with i % stride == 0 and j % stride == 0 of frame n reads its lens map (u, v) as dbw_lens_rectify_u8 forms it and
 * takes the NEAREST source pixel (floor(v + 0.5), floor(u + 0.5)); it is dropped where that is not finite or outside the frame, where the
 * depth d is outside [d_min, d_max] (0 is "no measurement"), and, with edge_permille > 0, where an in-frame 4-neighbour d_nb of the source
 * pixel is 0 or has 1000 * |d - d_nb| > edge_permille * d.  The camera point (x*z, y*z, z), z = (float)d, goes to p = A.c + t, each axis
 * is quantised to q = floor((p - lo) * inv_step), the sample is dropped (and counted in info[2]) unless 0 <= q < G * 1024 on all axes, and
 * its cell is ((qx >> 10) * G + (qy >> 10)) * G + (qz >> 10).  A cell adds up integers only (a 32-bit count, three 64-bit sums of q), so
 * the result does not depend on the order of arrival: two calls give the same bytes.  Outputs on the DEVICE: points (capacity,3) fp32 and
 * counts (capacity,) int32, one row per cell with count >= min_count in ascending cell order, point = lo + ((sum + 0.5 count) / count) /
 * inv_step in fp64, rounded once; rows from M on are not written.  info: 3 int64 [M, samples accumulated, samples outside the box].
 * workspace: dbw_lens_depth_cloud_workspace_bytes(G) bytes on the DEVICE, 16-byte aligned, contents irrelevant (the call clears it); the
 * size is 0 for a G outside [1, 256], else a multiple of 16.
 * Refused before any launch (DBW_ERR_INVALID): a null pointer; a misaligned one (workspace 16 bytes, points and counts 4, info 8, depth 2);
 * N, H, W, stride or min_count below 1; G outside [1, 256]; d_min outside [1, d_max] or d_max above 65535; edge_permille outside
 * [0, 1000]; N * ceil(H / stride) * ceil(W / stride) of 2^31 or more; capacity below the smaller of G^3 and that product; a value of cams,
 * target, poses or box that is not finite, an inv_step that is not > 0, and the cameras dbw_lens_rectify_u8 refuses. */
size_t dbw_lens_depth_cloud_workspace_bytes(int G);
int dbw_lens_depth_cloud(const uint16_t *depth, int N, int H, int W, const float *cams, const float *target, const float *poses,
                         const float *box, int G, int d_min, int d_max, int stride, int edge_permille, int min_count, void *workspace,
                         float *points, int32_t *counts, int64_t capacity, int64_t *info, dbw_stream_t stream);

/* The depth rays of a capture, added under revision 1 of this header (csrc/depth_cloud.hip, arithmetic: csrc/depth_math.h depth_ray_end): the
 * arguments of dbw_lens_depth_cloud without the grid and the cube.  rays on the DEVICE, 16-byte aligned: a dense array
 * (N, ceil(H / stride), ceil(W / stride)) of 16-byte records [px, py, pz fp32, frame int32], one per target pixel (i, j) with i % stride == 0
 * and j % stride == 0 of every frame, every record written.  (px, py, pz) is the world point p = A.c + t exactly as dbw_lens_depth_cloud
 * forms it (the same operations in the same order, the same lens map, the nearest source pixel) and frame is n; where
 * dbw_lens_depth_cloud drops the sample before the cube (lens, range, edge rule) or a coordinate of p is not finite, the record is
 * [0, 0, 0, -1].  The cube is not applied.  Refused before any launch (DBW_ERR_INVALID): a null pointer; a misaligned one (rays 16 bytes,
 * depth 2); N, H, W or stride below 1; d_min outside [1, d_max] or d_max above 65535; edge_permille outside [0, 1000];
 * N * ceil(H / stride) * ceil(W / stride) of 2^31 or more; a value of cams, target or poses that is not finite, and the cameras
 * dbw_lens_rectify_u8 refuses. */
int dbw_lens_depth_rays(const uint16_t *depth, int N, int H, int W, const float *cams, const float *target, const float *poses, int d_min,
                        int d_max, int stride, int edge_permille, void *rays, dbw_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
