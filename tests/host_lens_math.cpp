// Host build (g++) of csrc/lens_math.h for tests/test_host_lens_math.py, tests/test_custom_scene_host.py and tests/test_gpu_lens.py: the same
// inline functions the rectification kernel compiles, driven by the plain loop over frames, rows, pixels and channels.
#include "../differentiable-blocksworld_amd/csrc/lens_math.h"

using namespace dbw;

extern "C" {

// the source index coordinates of every output pixel, not clamped: u, v (H, W) fp32
int host_lens_source(int H, int W, const float *lens, float *u, float *v) {
    const LensParams L = lens_params(lens);
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) lens_source(L, i, j, u + (long long)i * W + j, v + (long long)i * W + j);
    return 0;
}

// dbw_images_undistort_u8 on the host: src (N,H,W,3) uint8 -> out (N,H,W,3) uint8
int host_images_undistort_u8(const uint8_t *src, int N, int H, int W, const float *lens, uint8_t *out) {
    if (!src || !lens || !out || N < 1 || H < 2 || W < 2) return -1;
    const LensParams L = lens_params(lens);
    for (long long n = 0; n < N; ++n) {
        const uint8_t *s = src + n * H * W * 3;
        for (int i = 0; i < H; ++i)
            for (int j = 0; j < W; ++j) {
                const LensTap t = lens_tap(L, i, j, H, W);
                const uint8_t *c0 = s + ((long long)t.y0 * W + t.x0) * 3, *c1 = c0 + (long long)W * 3;
                for (int c = 0; c < 3; ++c) out[((n * H + i) * W + j) * 3 + c] = lens_blend(c0[c], c0[3 + c], c1[c], c1[3 + c], t.wx, t.wy);
            }
    }
    return 0;
}

}
