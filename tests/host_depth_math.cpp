// Host build (g++) of csrc/depth_math.h for tests/test_host_depth_math.py, tests/test_depth_cloud_host.py and tests/test_gpu_depth_cloud.py:
// the same inline functions the kernels of csrc/depth_cloud.hip compile, driven by the plain loop over frames and selected pixels, with the
// integer accumulation and the emit in cell order written out.
#include "../differentiable-blocksworld_amd/csrc/depth_math.h"

using namespace dbw;

extern "C" {

// every selected pixel of every frame: cell (N,Hs,Ws) int32 (>= 0, or DEPTH_DROPPED / DEPTH_OUTSIDE) and q (N,Hs,Ws,3) int32 (0 where dropped)
int host_depth_samples(const uint16_t *depth, int N, int H, int W, const float *cams, const float *target, const float *poses, const float *box,
                       int G, int d_min, int d_max, int stride, int edge_permille, int32_t *cell, int32_t *q) {
    const DepthRule D = {H, W, G, d_min, d_max, edge_permille};
    const LensTarget T = lens_target(target);
    long long k = 0;
    for (long long n = 0; n < N; ++n) {
        const LensCam C = lens_cam(cams + n * LENS_RECT_N_PARAMS);
        for (int i = 0; i < H; i += stride)
            for (int j = 0; j < W; j += stride, ++k) {
                int qq[3] = {0, 0, 0};
                cell[k] = depth_sample(depth + n * H * W, D, C, T, poses + n * DEPTH_POSE_N, box, i, j, qq);
                for (int a = 0; a < 3; ++a) q[3 * k + a] = cell[k] >= 0 ? qq[a] : 0;
            }
    }
    return 0;
}

// dbw_lens_depth_cloud on the host.  cell_count (G^3) uint32 and cell_sum (G^3,3) uint64 are the caller's, zeroed; points (G^3,3), counts
// (G^3), info (3) int64 -> M.
long long host_depth_cloud(const uint16_t *depth, int N, int H, int W, const float *cams, const float *target, const float *poses, const float *box,
                           int G, int d_min, int d_max, int stride, int edge_permille, int min_count, uint32_t *cell_count,
                           unsigned long long *cell_sum, float *points, int32_t *counts, int64_t *info) {
    const DepthRule D = {H, W, G, d_min, d_max, edge_permille};
    const LensTarget T = lens_target(target);
    int64_t in = 0, outside = 0;
    for (long long n = 0; n < N; ++n) {
        const LensCam C = lens_cam(cams + n * LENS_RECT_N_PARAMS);
        for (int i = 0; i < H; i += stride)
            for (int j = 0; j < W; j += stride) {
                int q[3];
                const int cell = depth_sample(depth + n * H * W, D, C, T, poses + n * DEPTH_POSE_N, box, i, j, q);
                if (cell == DEPTH_OUTSIDE) ++outside;
                if (cell < 0) continue;
                ++in;
                ++cell_count[cell];
                for (int a = 0; a < 3; ++a) cell_sum[3LL * cell + a] += (unsigned long long)q[a];
            }
    }
    long long M = 0;
    for (long long c = 0; c < (long long)G * G * G; ++c) {
        if (cell_count[c] < (uint32_t)min_count) continue;
        for (int a = 0; a < 3; ++a) points[3 * M + a] = depth_point(cell_sum[3 * c + a], cell_count[c], box[a], box[3]);
        counts[M++] = (int32_t)cell_count[c];
    }
    info[0] = M; info[1] = in; info[2] = outside;
    return M;
}

}
