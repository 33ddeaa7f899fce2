// Host build (g++) of the SSIM term's arithmetic (csrc/score_math.h: ssim_stats, ssim_filter, ssim_deriv, ssim_loss_pixel, ssim_grad_pixel) for
// tests/test_host_ssim_term.py and tests/test_gpu_ssim_term.py: the same inline functions ssim_term_kernel compiles, driven plane by
// plane (the kernel walks 16 x 32 tiles; every window and every gradient element sees the same operations in the same order, so the
// gradient is the kernel's bit for bit; the value is added pixel by pixel in index order here, per workgroup there).  With
// -DSSIM_TERM_MAIN the file is a program of its own, for a run under the sanitizers.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../differentiable-blocksworld_amd/csrc/score_math.h"

using namespace dbw;

namespace {

// x (H,W) -> out (H,W): the zero-padded 11-tap filter along the rows (axis = 0) or the columns (axis = 1)
void blur_axis(const SsimWindow &win, const float *x, int H, int W, int axis, float *out) {
    for (int y = 0; y < H; ++y)
        for (int xx = 0; xx < W; ++xx) {
            float t[SSIM_TAPS];
            for (int k = 0; k < SSIM_TAPS; ++k) {
                const int yi = axis ? y - SSIM_TAPS / 2 + k : y, xi = axis ? xx : xx - SSIM_TAPS / 2 + k;
                t[k] = yi >= 0 && yi < H && xi >= 0 && xi < W ? x[(size_t)yi * W + xi] : 0.f;
            }
            out[(size_t)y * W + xx] = ssim_filter(win.w, t);
        }
}

}  // namespace

extern "C" {

// dbw_monitor_ssim_term on the host: same arguments without the workspace and the stream (every pointer a host pointer).  map, when not
// NULL: (N,3,H,W), receives the SSIM map.  -1 where the entry point refuses.
int host_ssim_term(const float *a, const float *b, int N, int H, int W, float *grad, float *map, double *value) {
    if (!a || !b || !value || N < 0 || H <= 0 || W <= 0) return -1;
    if (N == 0) return 0;
    const SsimWindow win = ssim_window();
    const size_t P = (size_t)H * W;
    const double M = (double)N * 3.0 * (double)H * (double)W, scale = -1.0 / M;
    std::vector<float> stat(P), rows(P), m5(5 * P), d(3 * P), f(3 * P);
    double sum = 0.0;
    for (int plane = 0; plane < N * 3; ++plane) {
        const float *pa = a + plane * P, *pb = b + plane * P;
        for (int j = 0; j < 5; ++j) {
            for (size_t i = 0; i < P; ++i) {
                float s[5];
                ssim_stats(pa[i], pb[i], s);
                stat[i] = s[j];
            }
            blur_axis(win, stat.data(), H, W, 0, rows.data());
            blur_axis(win, rows.data(), H, W, 1, m5.data() + j * P);
        }
        for (size_t i = 0; i < P; ++i) {
            const float m[5] = {m5[i], m5[P + i], m5[2 * P + i], m5[3 * P + i], m5[4 * P + i]};
            const SsimDeriv r = ssim_deriv(m);
            d[i] = r.A; d[P + i] = r.B; d[2 * P + i] = r.C;
            if (map) map[plane * P + i] = r.S;
            sum += ssim_loss_pixel(m);
        }
        if (!grad) continue;
        for (int j = 0; j < 3; ++j) {
            blur_axis(win, d.data() + j * P, H, W, 0, rows.data());
            blur_axis(win, rows.data(), H, W, 1, f.data() + j * P);
        }
        for (size_t i = 0; i < P; ++i) grad[plane * P + i] = ssim_grad_pixel(f[i], f[P + i], f[2 * P + i], pa[i], pb[i], scale);
    }
    value[0] = sum / M;
    return 0;
}

// S of ssim_deriv against ssim_pixel on the same statistics: 1 where the bits agree
int host_ssim_deriv_matches_pixel(const float *m) { return f2u(ssim_deriv(m).S) == f2u(ssim_pixel(m)); }

}

#ifdef SSIM_TERM_MAIN
// Every shape of the tests, exactly sized heap buffers: a read or write outside them is the sanitizer's to report.
int main() {
    const int shapes[][3] = {{1, 5, 7}, {2, 16, 32}, {1, 17, 33}, {2, 19, 37}, {1, 48, 96}};
    uint32_t seed = 12345u;
    for (const auto &s : shapes) {
        const int N = s[0], H = s[1], W = s[2];
        std::vector<float> a((size_t)N * 3 * H * W), b(a.size()), g(a.size());
        for (size_t i = 0; i < a.size(); ++i) {
            seed = seed * 1664525u + 1013904223u; a[i] = (float)(seed >> 8) / 16777216.f;
            seed = seed * 1664525u + 1013904223u; b[i] = (float)(seed >> 8) / 16777216.f;
        }
        double v = -1.0, v0 = -1.0;
        if (host_ssim_term(a.data(), b.data(), N, H, W, g.data(), nullptr, &v) != 0 || !(v > 0.0 && v < 2.0)) return 1;
        if (host_ssim_term(a.data(), b.data(), N, H, W, nullptr, nullptr, &v0) != 0 || v0 != v) return 1;
        if (host_ssim_term(a.data(), a.data(), N, H, W, g.data(), nullptr, &v) != 0 || v != 0.0) return 1;
        printf("%dx3x%dx%d: ok\n", N, H, W);
    }
    double v;
    return host_ssim_term(nullptr, nullptr, 1, 4, 4, nullptr, nullptr, &v) == -1 ? 0 : 1;
}
#endif
