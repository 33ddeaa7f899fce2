// Host build (g++) of depth_ray_end of csrc/depth_math.h for tests/test_freespace_host.py and tests/test_gpu_depth_rays.py: the plain loop
// over frames and selected pixels that csrc/depth_cloud.hip's depth_rays_kernel runs, the records as it writes them -- and, beside them,
// depth_sample's verdict on the same pixel against a cube, so that a test can hold the two functions to each other.
#include <string.h>

#include "../differentiable-blocksworld_amd/csrc/depth_math.h"

using namespace dbw;

extern "C" {

// rays (N,Hs,Ws,4) as 32-bit words: px, py, pz, frame (-1 after three zeros: no measurement).  cell (N,Hs,Ws) int32 or NULL: depth_sample's
// result for the pixel with the cube `box` of G cells.
int host_depth_rays(const uint16_t *depth, int N, int H, int W, const float *cams, const float *target, const float *poses, int d_min, int d_max,
                    int stride, int edge_permille, uint32_t *rays, const float *box, int G, int32_t *cell) {
    const DepthRule D = {H, W, G, d_min, d_max, edge_permille};
    const LensTarget T = lens_target(target);
    long long k = 0;
    for (long long n = 0; n < N; ++n) {
        const LensCam C = lens_cam(cams + n * LENS_RECT_N_PARAMS);
        for (int i = 0; i < H; i += stride)
            for (int j = 0; j < W; j += stride, ++k) {
                float p[3] = {0.0f, 0.0f, 0.0f};
                const bool ok = depth_ray_end(depth + n * H * W, D, C, T, poses + n * DEPTH_POSE_N, i, j, p);
                if (!ok) p[0] = p[1] = p[2] = 0.0f;
                memcpy(rays + 4 * k, p, 12);
                rays[4 * k + 3] = ok ? (uint32_t)n : 0xffffffffu;
                if (cell) {
                    int q[3];
                    cell[k] = depth_sample(depth + n * H * W, D, C, T, poses + n * DEPTH_POSE_N, box, i, j, q);
                }
            }
    }
    return 0;
}

}
