// Host build (g++) of csrc/frame_math.h for tests/test_host_frame_math.py and tests/test_gpu_export.py: the same inline functions
// frames_u8_kernel compiles, driven by the loop that kernel runs (one thread per 4 pixels there, one iteration per pixel here).
#include "../differentiable-blocksworld_amd/csrc/frame_math.h"

using namespace dbw;

extern "C" {

// dbw_frames_u8 on the host: same arguments (every pointer a host pointer), same bytes
int host_frames_u8(const float *src, int N, int C, int H, int W, int flags, const float *bkg3, const float *bkg_img, const float *mask,
                   const float *edge3, const float *edge_img, uint8_t *out) {
    const long long P = (long long)H * W;
    const bool has_bkg = bkg3 || bkg_img;
    for (long long n = 0; n < N; ++n)
        for (long long q = 0; q < P; ++q) {
            float p[4] = {0.f, 0.f, 0.f, 1.f}, b[3] = {0.f, 0.f, 0.f}, e[3] = {0.f, 0.f, 0.f}, m = 0.f;
            if (flags & FRAME_HWC) {
                for (int c = 0; c < 3; ++c) p[c] = src[(n * P + q) * 3 + c];
            } else {
                for (int c = 0; c < C; ++c) p[c] = src[(n * C + c) * P + q];
            }
            for (int c = 0; c < 3; ++c) {
                if (bkg3) b[c] = bkg3[c];
                if (bkg_img) b[c] = bkg_img[c * P + q];
                if (edge3) e[c] = edge3[c];
                if (edge_img) e[c] = edge_img[(n * 3 + c) * P + q];
            }
            if (mask) m = mask[n * P + q];
            frame_pixel(p, has_bkg, b, mask != nullptr, m, e, flags, out + (n * P + q) * 3);
        }
    return 0;
}

// the two blends alone, element-wise over n floats: what torch evaluates as rgb * alpha + (1 - alpha) * bkg and img * (1 - mask) + mask * colour
int host_composite(const float *rgb, const float *alpha, const float *bkg, long long n, float *out) {
    for (long long i = 0; i < n; ++i) out[i] = frame_composite(rgb[i], alpha[i], bkg[i]);
    return 0;
}

int host_edge_blend(const float *img, const float *mask, const float *colour, long long n, float *out) {
    for (long long i = 0; i < n; ++i) out[i] = frame_edge_blend(img[i], mask[i], colour[i]);
    return 0;
}

}
