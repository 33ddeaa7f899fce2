// Host build (g++) of csrc/score_math.h for tests/test_host_score_math.py and tests/test_gpu_monitor.py: the same inline functions
// image_scores_kernel compiles, driven plane by plane (the kernel walks 16 x 32 tiles; every output sees the same operations in the same
// order).  With -DSCORE_MATH_MAIN the file is a program of its own, for a run under the sanitizers.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../differentiable-blocksworld_amd/csrc/score_math.h"

using namespace dbw;

extern "C" {

int host_ssim_window(float *w) {
    const SsimWindow win = ssim_window();
    for (int k = 0; k < SSIM_TAPS; ++k) w[k] = win.w[k];
    return 0;
}

// dbw_image_scores on the host: same arguments without the workspace (every pointer a host pointer); the sums of out are added pixel by
// pixel in index order.  -1 where the entry point refuses.
int host_image_scores(const float *a, const float *b, int N, int H, int W, int padding, float *map, double *out) {
    if (!a || !b || !out || N < 0 || H <= 0 || W <= 0 || (padding != 0 && padding != 1)) return -1;
    if (!padding && (H < SSIM_TAPS || W < SSIM_TAPS)) return -1;
    const SsimWindow win = ssim_window();
    const int off = padding ? SSIM_HALO / 2 : 0;
    const int Hp = padding ? H : H - SSIM_HALO, Wp = padding ? W : W - SSIM_HALO;
    std::vector<float> rows((size_t)5 * H * Wp);                   // the five statistics, filtered along the rows
    for (int n = 0; n < N; ++n) {
        double se = 0.0, ss = 0.0;
        for (int ch = 0; ch < 3; ++ch) {
            const float *pa = a + ((size_t)n * 3 + ch) * H * W, *pb = b + ((size_t)n * 3 + ch) * H * W;
            for (size_t i = 0; i < (size_t)H * W; ++i) se += sq_err(pa[i], pb[i]);
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < Wp; ++x) {
                    float t[5][SSIM_TAPS];
                    for (int k = 0; k < SSIM_TAPS; ++k) {
                        const int xi = x - off + k;
                        const bool in = xi >= 0 && xi < W;
                        float s[5];
                        ssim_stats(in ? pa[(size_t)y * W + xi] : 0.f, in ? pb[(size_t)y * W + xi] : 0.f, s);
                        for (int j = 0; j < 5; ++j) t[j][k] = s[j];
                    }
                    for (int j = 0; j < 5; ++j) rows[((size_t)j * H + y) * Wp + x] = ssim_filter(win.w, t[j]);
                }
            for (int y = 0; y < Hp; ++y)
                for (int x = 0; x < Wp; ++x) {
                    float m[5];
                    for (int j = 0; j < 5; ++j) {
                        float t[SSIM_TAPS];
                        for (int k = 0; k < SSIM_TAPS; ++k) {
                            const int yi = y - off + k;
                            t[k] = yi >= 0 && yi < H ? rows[((size_t)j * H + yi) * Wp + x] : 0.f;
                        }
                        m[j] = ssim_filter(win.w, t);
                    }
                    const float v = ssim_pixel(m);
                    if (map) map[(((size_t)n * 3 + ch) * Hp + y) * Wp + x] = v;
                    ss += (double)v;
                }
        }
        out[2 * n] = se;
        out[2 * n + 1] = ss;
    }
    return 0;
}

}

#ifdef SCORE_MATH_MAIN
// Every shape of the tests, both paddings, exactly sized heap buffers: a read or write outside them is the sanitizer's to report.
int main() {
    const int shapes[][2] = {{11, 11}, {12, 16}, {23, 37}, {37, 70}, {48, 64}, {40, 52}};
    uint32_t seed = 12345u;
    for (const auto &hw : shapes)
        for (int padding = 0; padding < 2; ++padding) {
            const int N = 2, H = hw[0], W = hw[1], Hp = padding ? H : H - SSIM_HALO, Wp = padding ? W : W - SSIM_HALO;
            std::vector<float> a((size_t)N * 3 * H * W), b(a.size()), map((size_t)N * 3 * Hp * Wp);
            for (size_t i = 0; i < a.size(); ++i) {
                seed = seed * 1664525u + 1013904223u; a[i] = (float)(seed >> 8) / 16777216.f;
                seed = seed * 1664525u + 1013904223u; b[i] = (float)(seed >> 8) / 16777216.f;
            }
            std::vector<double> out(2 * N);
            if (host_image_scores(a.data(), b.data(), N, H, W, padding, map.data(), out.data()) != 0) return 1;
            for (float v : map)
                if (!(v >= -1.0001f && v <= 1.0001f)) { printf("SSIM out of range: %g\n", v); return 1; }
            if (host_image_scores(a.data(), a.data(), N, H, W, padding, map.data(), out.data()) != 0 || out[0] != 0.0) return 1;
            printf("%dx%d padding %d: ok\n", H, W, padding);
        }
    std::vector<float> t((size_t)3 * 10 * 16);
    double o[2];
    if (host_image_scores(t.data(), t.data(), 1, 10, 16, 0, nullptr, o) != -1) return 1;
    return 0;
}
#endif
