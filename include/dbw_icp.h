/*
 * dbw_icp.h -- C ABI of the gradient ICP of libdbw_hip.so: the alignment loop of the reference's ICP-aligned mesh scores
 * (src/utils/icp.py:11-78, the per-instance branch: Chamfer forward, backward, Adam, keep-best every 10 iterations) behind ONE call.
 * Python side: dbw_amd/eval3d.py (icp_run, gradient_icp), bound through _lib.ICP_SIGNATURES.  The arithmetic is csrc/icp_math.h, the two
 * nearest-neighbour searches of an iteration are the kernel of dbw_nn_points (include/dbw_eval.h).
 *
 * Conventions are those of dbw_hip.h: DEVICE pointers owned by the caller, contiguous; return 0 or a negative DBW_ERR_*, the text in
 * dbw_last_error(); arguments are validated before any launch; kernels are enqueued on `stream`, no host synchronisation and no host read.
 */
#ifndef DBW_ICP_H
#define DBW_ICP_H
#include "dbw_hip.h"

/* ABI revision of this header (dbw_icp_abi_version() returns the value the library was built with).
 *   1: dbw_icp_workspace_bytes, dbw_icp_run. */
#define DBW_ICP_ABI_VERSION 1

#define DBW_ICP_TRACE_PER_INSTANCE 15 /* R (9, row-major), T (3), s (3) */

#ifdef __cplusplus
extern "C" {
#endif

int dbw_icp_abi_version(void);

/* Bytes of `workspace` that dbw_icp_run needs for these sizes; 0 for sizes it refuses.  (n_iter does not enter today: the trace is the
 * caller's buffer.) */
size_t dbw_icp_workspace_bytes(int N, int P1, int P2, int n_iter);

/* pred (N,P1,3), gt (N,P2,3) fp32.  Minimises over R6 (6D rotation, R = rotation_6d_to_matrix(R6)), T and s, per instance,
 *   L = (1/N) sum_n [ (1/P1) sum_i |q_i - g_nn(i)|^2 + (1/P2) sum_j |q_nn(j) - g_j|^2 ],   q_i = (s * p_i) @ R + T  (row vectors),
 * with torch's Adam (betas 0.9 / 0.999, eps 1e-8, learning rate lr) for n_iter iterations from R = I, T = 0, s = 1.
 *   estimate_scale = 0: s stays 1.  anisotropic_scale = 0: one scale per instance (s[0] == s[1] == s[2]).
 *   splits: as in dbw_nn_points (0 = chosen from the sizes); the result does not depend on it.
 * Per iteration: q from the current parameters, the two exact searches, the 2 x 13 sums (loss, dL/dT, dL/dM with M = diag(s) R) of the
 * chosen pairs with residuals taken in fp64, summed per workgroup and then in index order (no atomics: two runs give the same bits), the
 * chain to the parameters and the Adam step in fp32.  Keep-best (icp.py:27-28,65-74): the batch-mean loss is averaged since the last
 * check; at every iteration with it % 10 == 0 the average is compared with the smallest kept so far (1e6 at the start), the parameters
 * AFTER that iteration's step are kept when it is smaller, and the average restarts.
 * Outputs: out_cloud (N,P1,3) fp32: pred under the kept parameters; out_R (N,9), out_T (N,3), out_s (N,3) fp32: the kept parameters
 * (the identity when no check was passed); out_best (2) fp64: the kept loss average (1e6 when none) and its iteration (-1 when none).
 * trace, when not NULL: (n_iter, 1 + 15 N) fp64: the batch-mean loss of the iteration, then every instance's R, T, s after its step.
 * workspace: dbw_icp_workspace_bytes(...) bytes, 16-byte aligned. */
int dbw_icp_run(const float *pred, const float *gt, int N, int P1, int P2, int estimate_scale, int anisotropic_scale, double lr, int n_iter,
                int splits, void *workspace, float *out_cloud, float *out_R, float *out_T, float *out_s, double *out_best, double *trace,
                dbw_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
