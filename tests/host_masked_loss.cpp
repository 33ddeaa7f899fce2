// Host build (g++) of the arithmetic of the masked image terms (csrc/masked_loss.hip, csrc/ssim_term.hip) and of dbw_lens_valid_u8 for
// tests/test_host_masked_loss.py and the GPU tests: the inline functions the kernels compile (csrc/loss_math.h: masked_composite_pixel;
// csrc/score_math.h: ssim_stats, ssim_filter, ssim_deriv, ssim_loss_pixel, ssim_grad_pixel; csrc/lens_math.h: lens_valid), driven plane by
// plane (tests/host_ssim_model.h) and pixel by pixel.  Every window and every gradient element sees the kernel's operations in the
// kernel's order, so rec and the gradients are the kernels' bit for bit; the values are added in index order here, per lane and
// workgroup there.  With -DMASKED_LOSS_MAIN the file is a program of its own, for a run under the sanitizers.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../differentiable-blocksworld_amd/csrc/lens_math.h"
#include "../differentiable-blocksworld_amd/csrc/loss_math.h"
#include "host_ssim_model.h"

using namespace dbw;

extern "C" {

// dbw_monitor_masked_ssim_term on the host: same arguments without the workspace and the stream (every pointer a host pointer).
// -1 where the entry point refuses.
int host_masked_ssim_term(const float *a, const float *b, const float *msk, int N, int H, int W, double count, float *grad, double *value) {
    if (!a || !b || !msk || !value || N < 0 || H <= 0 || W <= 0 || !(count >= 0.0)) return -1;
    if (N == 0) return 0;
    const double sum = host_ssim_planes<true>(a, b, msk, N, H, W, count > 0.0 ? -1.0 / count : 0.0, grad, nullptr);
    value[0] = count > 0.0 ? sum / count : 0.0;
    return 0;
}

// dbw_monitor_masked_composite on the host, both directions in one call: rec (N,3,H,W) and value[0] = scale * sum m (rec - img)^2, and --
// where grad_fg is given -- grad_fg, grad_env (N,4,H,W) for the upstream scalar `upstream` and the optional grad_rec (N,3,H,W).
int host_masked_composite(const float *fg, const float *env, const float *imgs, const float *msk, int N, int H, int W, double scale, float *rec,
                          double *value, float upstream, const float *grad_rec, float *grad_fg, float *grad_env) {
    if (!fg || !env || !imgs || !msk || N < 0 || H <= 0 || W <= 0 || (grad_fg == nullptr) != (grad_env == nullptr)) return -1;
    const size_t P = (size_t)H * W;
    const float two_scale = grad_fg ? (float)((2.0 * scale) * (double)upstream) : 0.f;
    double sum = 0.0;
    for (size_t n = 0; n < (size_t)N; ++n)
        for (size_t p = 0; p < P; ++p) {
            const float *f = fg + n * 4 * P + p, *e = env + n * 4 * P + p, *t = imgs + n * 3 * P + p;
            const float f3[3] = {f[0], f[P], f[2 * P]}, e3[3] = {e[0], e[P], e[2 * P]}, t3[3] = {t[0], t[P], t[2 * P]};
            float x3[3] = {0.f, 0.f, 0.f};
            const bool has_extra = grad_fg && grad_rec;
            if (has_extra)
                for (int c = 0; c < 3; ++c) x3[c] = grad_rec[n * 3 * P + c * P + p];
            float r3[3], gf3[3], ge3[3], gmask;
            sum += (double)masked_composite_pixel(f3, f[3 * P], e3, t3, msk[n * P + p], two_scale, r3, gf3, ge3, gmask, x3, has_extra);
            for (int c = 0; c < 3; ++c) {
                if (rec) rec[n * 3 * P + c * P + p] = r3[c];
                if (grad_fg) { grad_fg[n * 4 * P + c * P + p] = gf3[c]; grad_env[n * 4 * P + c * P + p] = ge3[c]; }
            }
            if (grad_fg) { grad_fg[n * 4 * P + 3 * P + p] = gmask; grad_env[n * 4 * P + 3 * P + p] = 0.f; }
        }
    if (value) value[0] = sum * scale;
    return 0;
}

// dbw_lens_valid_u8 on the host: out (H,W) uint8
int host_lens_valid_u8(int H, int W, const float *lens, uint8_t *out) {
    if (!lens || !out || H < 1 || W < 1) return -1;
    const LensParams L = lens_params(lens);
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) out[(size_t)i * W + j] = lens_valid(L, i, j, H, W) ? 255 : 0;
    return 0;
}

}

#ifdef MASKED_LOSS_MAIN
// Every shape of the tests, exactly sized heap buffers: a read or write outside them is the sanitizer's to report.
int main() {
    const int shapes[][3] = {{1, 5, 7}, {2, 16, 32}, {1, 17, 33}, {2, 19, 37}, {1, 48, 96}};
    uint32_t seed = 12345u;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) / 16777216.f; };
    for (const auto &s : shapes) {
        const int N = s[0], H = s[1], W = s[2];
        const size_t P = (size_t)H * W;
        std::vector<float> a(N * 3 * P), b(a.size()), g(a.size()), m(N * P), zero(N * P, 0.f);
        std::vector<float> fg(N * 4 * P), env(fg.size()), gfg(fg.size()), genv(fg.size()), rec(a.size());
        for (auto &v : a) v = rnd();
        for (auto &v : b) v = rnd();
        for (auto &v : fg) v = rnd();
        for (auto &v : env) v = rnd();
        double cnt = 0.0;
        for (auto &v : m) { v = rnd() < 0.3f ? 0.f : 1.f; cnt += 3.0 * v; }
        double v = -1.0, v0 = -1.0;
        if (host_masked_ssim_term(a.data(), b.data(), m.data(), N, H, W, cnt, g.data(), &v) != 0 || !(v > 0.0 && v < 2.0)) return 1;
        if (host_masked_ssim_term(a.data(), b.data(), m.data(), N, H, W, cnt, nullptr, &v0) != 0 || v0 != v) return 1;
        if (host_masked_ssim_term(a.data(), a.data(), m.data(), N, H, W, cnt, g.data(), &v) != 0 || v != 0.0) return 1;
        if (host_masked_ssim_term(a.data(), b.data(), zero.data(), N, H, W, 0.0, g.data(), &v) != 0 || v != 0.0) return 1;
        for (const float x : g)
            if (x != 0.f) return 1;
        if (host_masked_composite(fg.data(), env.data(), a.data(), m.data(), N, H, W, 1.0 / cnt, rec.data(), &v, 1.f, g.data(), gfg.data(),
                                  genv.data()) != 0 || !(v > 0.0)) return 1;
        if (host_masked_composite(fg.data(), env.data(), a.data(), m.data(), N, H, W, 1.0 / cnt, rec.data(), &v0, 0.f, nullptr, nullptr, nullptr) != 0
            || v0 != v) return 1;
        printf("%dx3x%dx%d: ok\n", N, H, W);
    }
    const float lens[12] = {28.8f, 29.44f, 16.32f, 11.52f, 1.f / 28.8f, 1.f / 29.44f, 0.12f, 0.02f, 0.f, 0.f, 0.003f, -0.002f};
    std::vector<uint8_t> valid(24 * 32);
    if (host_lens_valid_u8(24, 32, lens, valid.data()) != 0) return 1;
    double v;
    return host_masked_ssim_term(nullptr, nullptr, nullptr, 1, 4, 4, 1.0, nullptr, &v) == -1 ? 0 : 1;
}
#endif
