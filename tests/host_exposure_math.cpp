// Host build (g++) of csrc/exposure_math.h for tests/test_host_exposure_math.py: the inline functions the kernels of
// csrc/exposure_loss.hip compile, driven pixel by pixel over planar images as the kernels lay them out.
#include <stddef.h>

#include "../differentiable-blocksworld_amd/csrc/exposure_math.h"

using namespace dbw;

extern "C" {

// dbw_monitor_exposure_composite on the host, both directions in one call.  fg, env (N,4,H,W), imgs (N,3,H,W), masks (N,1,H,W) or NULL,
// theta (V,6), ids (N).  rec (N,3,H,W) and value[0] = scale * sum m (rec - img)^2 where given; where grad_fg is given: grad_fg, grad_env
// (N,4,H,W) written and the six sums of every view ADDED to row ids[n] of grad_theta (V,6) as doubles, for the upstream scalar and the
// optional grad_rec (N,3,H,W).  An id outside [0, V) reads as theta = 0 and its row is skipped.  -1 where the entry point refuses.
int host_exposure_composite(const float *fg, const float *env, const float *imgs, const float *msk, const float *theta, const int *ids, int N,
                            int H, int W, int V, double scale, float *rec, double *value, float upstream, const float *grad_rec, float *grad_fg,
                            float *grad_env, double *grad_theta) {
    if (!fg || !env || !imgs || !theta || !ids || N < 0 || H <= 0 || W <= 0 || V <= 0) return -1;
    if ((grad_fg == nullptr) != (grad_env == nullptr) || (grad_fg == nullptr) != (grad_theta == nullptr)) return -1;
    const size_t P = (size_t)H * W;
    const float two_scale = grad_fg ? (float)((2.0 * scale) * (double)upstream) : 0.f;
    double sum = 0.0;
    for (size_t n = 0; n < (size_t)N; ++n) {
        const bool inside = ids[n] >= 0 && ids[n] < V;
        float th[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (inside)
            for (int k = 0; k < 6; ++k) th[k] = theta[(size_t)ids[n] * 6 + k];
        float gain[3];
        exposure_gains(th, gain);
        const float bias[3] = {th[3], th[4], th[5]};
        double s6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (size_t p = 0; p < P; ++p) {
            const float *f = fg + n * 4 * P + p, *e = env + n * 4 * P + p, *t = imgs + n * 3 * P + p;
            const float f3[3] = {f[0], f[P], f[2 * P]}, e3[3] = {e[0], e[P], e[2 * P]}, t3[3] = {t[0], t[P], t[2 * P]};
            const float m = msk ? msk[n * P + p] : 1.f;
            float r3[3];
            sum += (double)exposure_forward_pixel(f3, f[3 * P], e3, t3, m, gain, bias, r3);
            if (rec)
                for (int c = 0; c < 3; ++c) rec[n * 3 * P + c * P + p] = r3[c];
            if (!grad_fg) continue;
            float x3[3] = {0.f, 0.f, 0.f};
            if (grad_rec)
                for (int c = 0; c < 3; ++c) x3[c] = grad_rec[n * 3 * P + c * P + p];
            float gf3[3], ge3[3], galpha, q6[6];
            exposure_backward_pixel(f3, f[3 * P], e3, t3, m, gain, bias, two_scale, x3, grad_rec != nullptr, gf3, ge3, galpha, q6);
            for (int c = 0; c < 3; ++c) { grad_fg[n * 4 * P + c * P + p] = gf3[c]; grad_env[n * 4 * P + c * P + p] = ge3[c]; }
            grad_fg[n * 4 * P + 3 * P + p] = galpha;
            grad_env[n * 4 * P + 3 * P + p] = 0.f;
            for (int k = 0; k < 6; ++k) s6[k] += (double)q6[k];
        }
        if (grad_fg && inside)
            for (int k = 0; k < 6; ++k) grad_theta[(size_t)ids[n] * 6 + k] += s6[k];
    }
    if (value) value[0] = sum * scale;
    return 0;
}

}
