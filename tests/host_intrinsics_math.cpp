// Checker-side build of the intrinsics refinement arithmetic (differentiable-blocksworld_amd/csrc/intrinsics_math.h, the header
// camera_grad.hip compiles) for the host.  tests/test_host_intrinsics_math.py holds the gradient of K to autograd of the oracle and to the
// vertex backward's own intermediate quantities, and apply / chain to a float64 restatement, without a GPU; tests/test_gpu_intrinsics.py holds
// the kernels to this build.  With -DINTRINSICS_MATH_MAIN the file is a program of its own (its main walks the same cases on exactly sized
// heap buffers) for -fsanitize=address,undefined.  Test infrastructure only.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../differentiable-blocksworld_amd/csrc/intrinsics_math.h"
#include "host_slot_loop.h"

using namespace dbw;

extern "C" {

// dbw_lens_intrinsics_grad for B views, slot by slot in fp32, the views' sums added in view order: gK (4,4) written.  gK_view (B,12) or null:
// the twelve accumulators of each view alone.  abs_terms (B,12) or null, with it n_terms (B), and gv (B,2F,3,3) or null: the bookkeeping of
// host_slot_loop.h, per view.
int host_intrinsics_grad(const float *verts, const int *faces, const float *R, const float *T, const float *Kmat, int B, int F, float eps, float zc,
                         int persp, const int *num_faces, const int *c2o, const int *code, const float *cw, const float *g, float *gK, float *gK_view,
                         double *abs_terms, int *n_terms, float *gv_out) {
    double total[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < B; ++b) {
        Cam cam;
        load_cam(R, T, Kmat, b, cam);
        float acc[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        host_view_slots<KGradSink>(verts, faces, cam, b, F, eps, zc, persp, num_faces[b], c2o, code, cw, g, acc, abs_terms ? abs_terms + b * 12 : nullptr,
                                   n_terms ? n_terms + b : nullptr, gv_out);
        for (int c = 0; c < 12; ++c) {
            total[c] += (double)acc[c];
            if (gK_view) gK_view[b * 12 + c] = acc[c];
        }
    }
    for (int i = 0; i < 16; ++i) gK[i] = 0.f;
    for (int c = 0; c < 12; ++c) gK[c < 8 ? c : c + 4] = (float)total[c];
    return 0;
}

int host_intrinsics_apply(const float *K0, const float *theta, float *K1) { intrinsics_apply(K0, theta, K1); return 0; }
int host_intrinsics_chain(const float *K0, const float *theta, const float *gK, float *gtheta) { intrinsics_chain(K0, theta, gK, gtheta); return 0; }

}  // extern "C"

#ifdef INTRINSICS_MATH_MAIN
// The cases of the tests on exactly sized heap buffers: a read or write outside them is the sanitizer's to report.
int main() {
    uint32_t seed = 2024u;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) / 16777216.f - 0.5f; };
    // apply and chain at the values of the tests
    const double thetas[] = {0.0, 1e-6, -1e-6, 1e-2, -1e-2, 0.5, -0.5};
    for (double th : thetas) {
        std::vector<float> K0 = {2.1f, 0, 0.05f, 0, 0, 2.3f, -0.03f, 0, 0, 0, 0, 1, 0, 0, 1, 0}, theta(4, (float)th), K1(16), gK(16), gt(4);
        for (auto &x : gK) x = rnd();
        host_intrinsics_apply(K0.data(), theta.data(), K1.data());
        host_intrinsics_chain(K0.data(), theta.data(), gK.data(), gt.data());
        double s = 0.0;
        for (float x : K1) s += x;
        for (float x : gt) s += x;
        bool same = true;
        for (int i = 0; i < 16; ++i) same = same && K1[i] == K0[i];
        if (!(s - s == 0.0) || (th == 0.0 && !same)) { std::printf("theta %g: not finite, or K(0) is not K0\n", th); return 1; }
        std::printf("theta %g: ok\n", th);
    }
    // gradient of K: a fan of triangles across the near plane of two cameras, so that untouched, dropped and clipped faces all occur
    for (int persp = 0; persp < 2; ++persp) {
        const int V = 40, F = 60, B = 2;
        const float zc = 0.25f, eps = 1e-8f;
        std::vector<float> verts((size_t)V * 3), R = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.8f, 0, -0.6f, 0, 1, 0, 0.6f, 0, 0.8f}, T = {0, 0, 0.3f, 0.1f, -0.1f, 0.2f},
                           K = {2.1f, 0, 0.05f, 0, 0, 2.1f, -0.03f, 0, 0, 0, 0, 1, 0, 0, 1, 0};
        std::vector<int> faces((size_t)F * 3);
        for (auto &x : verts) x = 2.f * rnd();
        for (int f = 0; f < F; ++f) { faces[f * 3] = f % V; faces[f * 3 + 1] = (f * 7 + 1) % V; faces[f * 3 + 2] = (f * 11 + 2) % V; }
        std::vector<int> num(B), c2o((size_t)B * 2 * F), code((size_t)B * 2 * F);
        std::vector<float> cw((size_t)B * 2 * F * 2), g((size_t)B * 2 * F * 9), gK(16), gKv((size_t)B * 12), gv((size_t)B * 2 * F * 9);
        std::vector<double> abs_terms((size_t)B * 12, 0.0);
        std::vector<int> n_terms((size_t)B, 0);
        int kinds[4] = {0, 0, 0, 0};
        for (int b = 0; b < B; ++b) {
            Cam cam;
            load_cam(R.data(), T.data(), K.data(), b, cam);
            int n = 0;
            for (int f = 0; f < F; ++f) {
                f3 p[3];
                for (int i = 0; i < 3; ++i) p[i] = project(verts.data() + (size_t)faces[f * 3 + i] * 3, cam, eps).ndc;
                ClippedFace cf;
                clip_face(p, 1, zc, persp, cf);
                for (int t = 0; t < cf.emit; ++t) {
                    const size_t o = (size_t)b * 2 * F + n + t;
                    c2o[o] = f; code[o] = t == 0 ? cf.code0 : cf.code1; cw[o * 2] = cf.w2; cw[o * 2 + 1] = cf.w3;
                    ++kinds[code[o] < 0 ? 3 : code[o] >> 2];
                }
                n += cf.emit;
            }
            num[b] = n;
        }
        for (auto &x : g) x = rnd();
        host_intrinsics_grad(verts.data(), faces.data(), R.data(), T.data(), K.data(), B, F, eps, zc, persp, num.data(), c2o.data(), code.data(), cw.data(),
                             g.data(), gK.data(), gKv.data(), abs_terms.data(), n_terms.data(), gv.data());
        double s = 0.0;
        for (float x : gK) s += x;
        const bool row2 = gK[8] == 0.f && gK[9] == 0.f && gK[10] == 0.f && gK[11] == 0.f;
        if (!(s - s == 0.0) || !row2 || !kinds[0] || !kinds[1] || !kinds[2] || !kinds[3]) {
            std::printf("gradient of K persp=%d: sum %g, row 2 zero %d, kinds %d %d %d, untouched %d\n", persp, s, (int)row2, kinds[0], kinds[1], kinds[2], kinds[3]);
            return 1;
        }
        std::printf("gradient of K persp=%d: ok\n", persp);
    }
    return 0;
}
#endif
