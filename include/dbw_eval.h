/*
 * dbw_eval.h -- C ABI of the 3D evaluation entry points of libdbw_hip.so: exact nearest neighbours (the Chamfer distance of
 * utils/chamfer.py, PyTorch3D's knn_points with K = 1) and the kernels of the official DTU protocol (utils/dtu_eval.py: the dense
 * triangle lattice and the greedy radius downsample).  Python side: dbw_amd/eval3d.py, bound through _lib.EVAL_SIGNATURES.
 *
 * Conventions are those of dbw_hip.h: DEVICE pointers owned by the caller, contiguous; return 0 or a negative DBW_ERR_*, the text in
 * dbw_last_error(); arguments are validated before any launch; kernels are enqueued on `stream`, no host synchronisation.
 */
#ifndef DBW_EVAL_H
#define DBW_EVAL_H
#include "dbw_hip.h"

/* ABI revision of this header (dbw_eval_abi_version() returns the value the library was built with). */
#define DBW_EVAL_ABI_VERSION 1

#ifdef __cplusplus
extern "C" {
#endif

int dbw_eval_abi_version(void);

/* Exact 1-nearest neighbour of every x[n, i] among y[n, 0 .. y_lengths[n]), fp32:
 *   dist2 = ((dx*dx + dy*dy) + dz*dz) with d = x - y, one rounding per operation; ties go to the lowest index.
 *   x (N,P1,3), y (N,P2,3) fp32; x_lengths / y_lengths (N,) int64 or NULL (= P1 / P2); keys (N*P1) uint64 workspace;
 *   dist2 (N,P1) fp32, idx (N,P1) int64.  A query at or past x_lengths[n] gets idx -1, dist2 0; a batch with y_lengths[n] == 0 gets
 *   idx -1, dist2 +inf.  splits: number of y ranges per batch searched by separate workgroups and merged with a 64-bit atomic min on
 *   (dist2 bits << 32 | idx), 0 = chosen from the sizes; the result does not depend on it.  P1, P2 < 2^31. */
int dbw_nn_points(const float *x, const float *y, const int64_t *x_lengths, const int64_t *y_lengths, int N, int P1, int P2, int splits,
                  void *keys, float *dist2, int64_t *idx, dbw_stream_t stream);

/* DTU dense lattice (dtu_eval.py:21-30,56-78), fp64 in numpy's order of operations.  tri (F,3,3): the three vertices of every face.
 * counts (F) int64: lattice points of each face (0 for a face of zero area). */
int dbw_dtu_lattice_counts(const double *tri, int64_t F, int64_t *counts, dbw_stream_t stream);
/* points (n_out,3) fp64: the lattice of face f at rows offsets[f] .. offsets[f] + counts[f], in np.mgrid row-major order.  A face whose
 * range does not fit in n_out writes nothing. */
int dbw_dtu_lattice_points(const double *tri, int64_t F, const int64_t *counts, const int64_t *offsets, int64_t n_out, double *points,
                           dbw_stream_t stream);

/* One round of the greedy radius downsample (dtu_eval.py:82-96) as a parallel maximal independent set.  points (n,3) fp64 sorted by
 * cell_keys (n) int64 ascending, key = (cx * ny + cy) * nz + cz of a uniform grid of cell size >= radius whose cell coordinates start at 1
 * (a border of empty cells on every side); rank (n) int64: each point's position in the processing order.  status_in / status_out (n)
 * int32: 0 undecided, 1 kept, 2 removed.  An undecided point with an earlier kept point within radius (distance <= radius) is removed; one
 * with no earlier undecided or kept point within radius is kept; the others stay undecided.  Repeat (swapping the two) until no point is
 * undecided: the kept set is that of the sequential loop. */
int dbw_radius_downsample_round(const double *points, const int64_t *cell_keys, const int64_t *rank, int64_t n, int64_t ny, int64_t nz,
                                double radius, const int32_t *status_in, int32_t *status_out, dbw_stream_t stream);

/* Plane RANSAC on a point cloud (csrc/plane_fit.hip, arithmetic csrc/plane_math.h; reference src/utils/ransac.py and the ground filter of
 * src/dtu_3d_process.py:36-41), added under revision 1 of this header.  points (N,3) fp32; H hypotheses, each the plane through three
 * points: the rows of triples (H,3) int32, or (NULL) those drawn by Philox4x32-10 from `seed` (its 64 bits; the type is int64_t for the
 * sake of plain-C bindings) and the hypothesis index.  A plane is (n, d), the residual of p is ((n.x*p.x + n.y*p.y) + n.z*p.z) - d, p is an
 * inlier iff residual^2 < thresh2.
 *   mode DBW_EVAL_PLANE_ORTHOGONAL: n is the unit normal (turned to n.up >= 0 when up (3) is given), thresh2 = tau^2.  Priors: with up, a
 *     hypothesis needs n.up >= cos_tilt; with cams (M,3), at least min_cams camera centres with residual > tau.
 *   mode DBW_EVAL_PLANE_VERTICAL: the reference's regression z = p0 + p1 x + p2 y as the plane n = (-p1, -p2, 1), d = p0; thresh2 is the
 *     reference's `thresh`.  up, cams and refine are not used.
 * A triple with a repeated index, (nearly) collinear points or, in the vertical mode, a vertical triangle is degenerate.  The best
 * hypothesis has the most inliers, the lowest index on ties.  refine (0..8) rounds, orthogonal mode only: the plane is refitted to its
 * inliers among all N points (smallest eigenvector of their fp64 covariance), stopping early below 3 inliers.
 * Outputs: plane (4) fp64 = n, d (zero if no hypothesis is admissible: the call still returns 0); info (4) int32 = best hypothesis or -1,
 * its count, the inlier count of the final plane, refinement rounds done; counts (H) int32 or NULL, -1 for a degenerate or inadmissible
 * hypothesis; triples_out (H,3) int32 or NULL; mask (N) uint8 or NULL, the inliers of the final plane (rounded to fp32).
 * 1 <= H <= 4096, 3 <= N < 2^31, M <= 65536.  workspace: dbw_eval_plane_workspace_bytes(N, H) bytes (0: sizes refused), 16-byte aligned. */
#define DBW_EVAL_PLANE_ORTHOGONAL 0
#define DBW_EVAL_PLANE_VERTICAL 1
size_t dbw_eval_plane_workspace_bytes(int64_t N, int H);
int dbw_eval_plane_fit(const float *points, int64_t N, int H, int mode, float thresh2, int64_t seed, const int32_t *triples, const float *up,
                       float cos_tilt, const float *cams, int M, float tau, int min_cams, int refine, void *workspace, double *plane,
                       int32_t *info, int32_t *counts, int32_t *triples_out, uint8_t *mask, dbw_stream_t stream);

/* k-means with a PCA of every cluster (csrc/cluster_fit.hip, arithmetic csrc/cluster_math.h), added under revision 1 of this header: where the
 * blocks of a custom scene start (dbw_amd/worldfit.py: blocks_from_points).  points (N,3) fp32, K centres.
 *   distance    dist2 = ((dx*dx + dy*dy) + dz*dz), d = p - c, fp32, as in dbw_nn_points.  The label of a point is the k of the smallest dist2,
 *               the lowest k on ties; a point with a non-finite coordinate gets -1 and enters no sum.
 *   seeding     init (K,3) fp32, or (NULL) farthest-point seeding: centre 0 is the point nearest the fp32-rounded mean of the finite points,
 *               centre j the point whose smallest dist2 to the centres 0 .. j-1 is largest, the lowest index on ties.  With fewer than K
 *               distinct points later centres repeat earlier ones and stay empty; without a finite point every centre is zero.
 *   rounds      n_iter Lloyd rounds, no early stop: every point is assigned and the fp64 moments of each cluster about its current centre
 *               (count, sum d, sum d d^T) are added in a fixed order (no floating-point atomics: the same call gives the same bytes); the
 *               centre becomes the fp64 mean rounded to fp32, an empty cluster keeps its centre.  One more pass against the final centres
 *               gives every output.
 * Outputs: centres (K,3) fp32, the centres the labels belong to; labels (N) int32 or NULL; counts (K) int32; mean (K,3) fp64 or NULL;
 * cov (K,6) fp64 or NULL (xx xy xz yy yz zz about the mean; zero below two points); evals (K,3) fp64 or NULL, descending; axes (K,3,3) fp64
 * or NULL: row i the unit eigenvector of evals[i], the largest-magnitude component of rows 0 and 1 positive (lowest index on ties), row 2 =
 * row 0 x row 1 (identity below two points); info (4) int32 = rounds done, labels that changed in the last pass (N when it is the only
 * one), non-empty clusters, 0.
 * 1 <= K <= 256, K <= N < 2^31, 0 <= n_iter <= 64.  workspace: dbw_eval_cluster_workspace_bytes(N, K) bytes (0: sizes refused), 16-byte
 * aligned. */
size_t dbw_eval_cluster_workspace_bytes(int64_t N, int K);
int dbw_eval_cluster_fit(const float *points, int64_t N, int K, const float *init, int n_iter, void *workspace, float *centres,
                         int32_t *labels, int32_t *counts, double *mean, double *cov, double *evals, double *axes, int32_t *info,
                         dbw_stream_t stream);

/* The surface term (csrc/surface_term.hip, arithmetic csrc/surface_math.h), added under revision 1 of this header: a capture's
 * point cloud against the posed meshes, in the frame of both.
 *   value[0] = (1/M) sum_i rho(d2(p_i, S)),  value[1] = (1/back_count) sum_v a_{k(v)} rho(|x_v - nn(x_v)|^2),  rho(d2) = min(d2, tau^2), fp64.
 *   points (N,3) fp32, the cloud.  n_points > 0: M = n_points draws, draw i is cloud index step_random(seed, step, stream 2, i).x mod N
 *     (csrc/rng_math.h), taken inside the kernels; n_points == 0: M = N, all points in order.
 *   verts (V,3) fp32, faces (F,3) int32 into them, in G groups of consecutive faces: face_group (G+1) int32, ascending from 0 to F -- the
 *     caller's contract, like faces < V when faces_host (a HOST copy of faces, or NULL) is not offered: the kernels clamp both, so nothing
 *     outside the arrays is read, but the result then belongs to another mesh.  group_keep (G) int32 or NULL: a group with 0 is no part of S.
 *   d2(p, S) = |p - c|^2, c the closest point of S: per face the projection onto its plane where that lies inside, else the nearest of the
 *     clamped projections onto its sides; a face of zero area is its sides, of zero length its point.  Of equal d2 the lowest face wins.
 *   records (M) of 16 bytes, 16-byte aligned: d2 fp32, face int32, u, v fp32 with c = (1-u-v) v0 + u v1 + v v2.  A point without any kept
 *     face: face -1, d2 NaN (counted as tau^2).
 *   back > 0: x_v are the vertices with 0 <= vert_group[v] < A, a = vert_alpha (A) fp32, nn the exact nearest cloud point (dbw_nn_points'
 *     search); back_count the constant n_blocks * vertices per block.  back == 0: value[1] = 0, vert_alpha / vert_group may be NULL.
 *   cull (0 | 1): skip a group whose box is farther than every running best of a wave; records and value do not depend on it.
 *   A face index outside [0, V) is read as vertex 0 by both calls (faces_host refuses it before any launch).
 * dbw_eval_surface_bwd, on the records and the workspace that dbw_eval_surface_fwd left for the same arguments: with
 *   L = weight * (value[0] + back * value[1]),  grad_verts (V,3) fp32 = grad_out[0] * dL/dverts (-2 b_m (p - c) / M per record inside tau;
 *   2 a_k (x_v - nn) back / back_count per block vertex inside tau), grad_alpha (A) fp32 or NULL = grad_out[0] * dL/da (the sum of the block's
 *   rho).  grad_out: one fp32 on the device, or NULL (= 1).  Both outputs are written whole.  No floating-point atomics: records are walked in
 *   segments of `segment` (0: DBW_EVAL_SURFACE_SEGMENT; else in [64, 2^20]) in index order, the segments added in order.
 * 1 <= N < 2^31, 1 <= M <= 2^24, 1 <= F <= 2^20, 1 <= V <= 2^21, 1 <= G <= 4096, 0 <= A <= V, tau > 0, back >= 0.  workspace:
 * dbw_eval_surface_workspace_bytes(M, F, V, G, segment) bytes (0: sizes refused), 16-byte aligned, kept untouched between the two calls;
 * `segment` is the one dbw_eval_surface_bwd will be given: its partials, one row per segment, are the last part of the workspace, and
 * the entry points do not know the workspace's size (ops.surface_grads checks it). */
#define DBW_EVAL_SURFACE_SEGMENT 1024
size_t dbw_eval_surface_workspace_bytes(int64_t M, int F, int V, int G, int segment);
int dbw_eval_surface_fwd(const float *points, int64_t N, int64_t n_points, int64_t seed, int64_t step, const float *verts, int V,
                         const int32_t *faces, const int32_t *faces_host, int F, const int32_t *face_group, const int32_t *group_keep, int G,
                         const float *vert_alpha, const int32_t *vert_group, int A, double back_count, float tau, float back, int cull,
                         void *workspace, void *records, double *value, dbw_stream_t stream);
int dbw_eval_surface_bwd(const float *points, int64_t N, int64_t n_points, int64_t seed, int64_t step, const float *verts, int V,
                         const int32_t *faces, int F, int G, const float *vert_alpha, const int32_t *vert_group, int A, double back_count,
                         float tau, float back, float weight, const float *grad_out, int segment, const void *records, void *workspace,
                         float *grad_verts, float *grad_alpha, dbw_stream_t stream);

/* The free-space term (csrc/freespace_term.hip, arithmetic csrc/freespace_math.h), added under revision 1 of this header: a
 * capture's depth rays against the posed meshes, in the frame of both.
 *   value[0] = (1/M) sum_i a_{k(i)} psi(g_i), fp64.  Ray j runs from origins[frame[j]] to ends[j]: ends (Nr,3) fp32, frame (Nr) int32 (a
 *     frame outside [0, Nf) is a ray without a hit), origins (Nf,3) fp32.  n_rays > 0: M = n_rays draws, draw i is ray
 *     step_random(seed, step, stream 3, i).x mod Nr (csrc/rng_math.h), taken inside the kernels; n_rays == 0: M = Nr, all rays in order.
 *   verts, faces, faces_host, face_group, group_keep: as for dbw_eval_surface_fwd.  group_alpha (G) int32: a group's row of vert_alpha (A)
 *     fp32, or -1 (the ground: a = 1).  A == 0: vert_alpha may be NULL and every a is 1.
 *   With o the origin, e = end - o, l = |e| and, per face (a, b, c), e1 = b - a, e2 = c - a, n = e1 x e2, h = e x e2, s = o - a, q = s x e1,
 *     det = -(n . e), u = (s . h)/det, v = (e . q)/det, t = (e2 . q)/det: a face is a candidate when det^2 > 2^-16 (n . n)(e . e), u >= 0,
 *     v >= 0, u + v <= 1 and 0 < t < 1 (two-sided).  The first hit is the smallest t, the lowest face on equal t.
 *     g = (1 - t) l - margin;  psi(g) = 0 for g <= 0, g^2 for g <= tau, tau (2 g - tau) beyond.
 *   records (M) of 16 bytes, 16-byte aligned: t fp32, face int32, u, v fp32.  A ray without a candidate: face -1, t NaN; it adds 0.
 *   cull (0 | 1): skip a group whose slackened box no segment t in (0, best t) of a wave reaches.  Records and value do not depend on it for
 *     meshes whose faces have sin(e1, e2) >= 2^-4 (DESIGN.md 6v has the derivation; thinner faces met at the grazing limit are outside it).
 *   layout (0 | 1 | 2): the forward's schedule; records and value are the same bytes.  1: one workgroup per 256 rays walks every face.
 *     2, and 0 (the default): a grid of (256 rays x 128 faces), the first hit taken with a 64-bit integer atomic minimum of the key
 *     (bits(t) << 32) | face, its (t, u, v) formed again for the winner.
 *   A face index outside [0, V) is read as vertex 0 by both calls (faces_host refuses it before any launch).
 * dbw_eval_freespace_bwd, on the records and the workspace that dbw_eval_freespace_fwd left for the same arguments: with L = weight * value[0],
 *   grad_verts (V,3) fp32 = grad_out[0] * dL/dverts (-(weight/M) a psi'(g) l wts_m n / (n . e) per record, wts = (1-u-v, u, v),
 *   psi'(g) = 2 min(g, tau)), grad_alpha (A) fp32 or NULL when A == 0 = grad_out[0] * (weight/M) * the sum of psi over the records that hit
 *   the block.  grad_out: one fp32 on the device, or NULL (= 1).  Both outputs are written whole.  No floating-point atomics: records are
 *   walked in segments of `segment` (0: DBW_EVAL_FREESPACE_SEGMENT; else in [64, 2^20]) in index order, the segments added in order.
 * 1 <= Nr < 2^31, 1 <= Nf <= 2^20, 1 <= M <= 2^24, 1 <= F <= 2^20, 1 <= V <= 2^21, 1 <= G <= 4096, 0 <= A <= V, tau > 0, margin >= 0.
 * workspace: dbw_eval_freespace_workspace_bytes(M, F, V, G, segment) bytes (0: sizes refused), 16-byte aligned, kept untouched between the
 * two calls; `segment` is the one dbw_eval_freespace_bwd will be given (its partials are the last part of the workspace). */
#define DBW_EVAL_FREESPACE_SEGMENT 1024
size_t dbw_eval_freespace_workspace_bytes(int64_t M, int F, int V, int G, int segment);
int dbw_eval_freespace_fwd(const float *ends, const int32_t *frame, const float *origins, int64_t Nr, int Nf, int64_t n_rays, int64_t seed,
                           int64_t step, const float *verts, int V, const int32_t *faces, const int32_t *faces_host, int F,
                           const int32_t *face_group, const int32_t *group_keep, const int32_t *group_alpha, int G, const float *vert_alpha,
                           int A, float tau, float margin, int cull, int layout, void *workspace, void *records, double *value,
                           dbw_stream_t stream);
int dbw_eval_freespace_bwd(const float *ends, const int32_t *frame, const float *origins, int64_t Nr, int Nf, int64_t n_rays, int64_t seed,
                           int64_t step, const float *verts, int V, const int32_t *faces, int F, int G, const float *vert_alpha, int A,
                           float tau, float margin, float weight, const float *grad_out, int segment, const void *records, void *workspace,
                           float *grad_verts, float *grad_alpha, dbw_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
