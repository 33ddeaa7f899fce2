// Host build (g++) of the SSIM term's arithmetic (csrc/score_math.h: ssim_stats, ssim_filter, ssim_deriv, ssim_loss_pixel, ssim_grad_pixel) for
// tests/test_host_ssim_term.py and tests/test_gpu_ssim_term.py: the same inline functions ssim_term_kernel compiles, driven plane by
// plane by tests/host_ssim_model.h (every window and every gradient element sees the kernel's operations in the kernel's order, so the
// gradient is the kernel's bit for bit; the value is added pixel by pixel in index order here, per workgroup there).  With
// -DSSIM_TERM_MAIN the file is a program of its own, for a run under the sanitizers.
#include <stdio.h>
#include <stdlib.h>

#include "host_ssim_model.h"

using namespace dbw;

extern "C" {

// dbw_monitor_ssim_term on the host: same arguments without the workspace and the stream (every pointer a host pointer).  map, when not
// NULL: (N,3,H,W), receives the SSIM map.  -1 where the entry point refuses.
int host_ssim_term(const float *a, const float *b, int N, int H, int W, float *grad, float *map, double *value) {
    if (!a || !b || !value || N < 0 || H <= 0 || W <= 0) return -1;
    if (N == 0) return 0;
    const double M = (double)N * 3.0 * (double)H * (double)W;
    value[0] = host_ssim_planes<false>(a, b, nullptr, N, H, W, -1.0 / M, grad, map) / M;
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
