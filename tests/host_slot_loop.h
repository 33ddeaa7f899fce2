// The slot loop of one view that the checker-side builds of the camera gradients share (tests/host_pose_math.cpp, tests/host_intrinsics_math.cpp):
// every clipped-face slot j < n of view b walked through camera_math.h::clip_slot_walk -- the walk the device compiles -- into a sink of type
// Sink (pose_math.h::CamGradSink, intrinsics_math.h::KGradSink), slot by slot in fp32 into acc, with the bookkeeping the tests ask for.
// Test infrastructure only.
#pragma once
#include <cmath>

#include "../differentiable-blocksworld_amd/csrc/camera_math.h"

// abs_terms (12) or null: per component the sum of the |terms| of the sum (a term = what one vertex of one slot adds), for the bound of an
// fp32 sum in the tests; with it n_terms or null: the number of terms (vertices whose gradient is not all zero: the others add nothing).
// gv_out (B,2F,3,3) or null: the ndc gradients of the three ORIGINAL vertices of every slot j < n, what the walk hands to the sink (zero
// where it hands nothing; other slots are not written).
template <class Sink>
void host_view_slots(const float *verts, const int *faces, const dbw::Cam &cam, int b, int F, float eps, float zc, int persp, int n, const int *c2o,
                     const int *code, const float *cw, const float *g, float (&acc)[12], double *abs_terms, int *n_terms, float *gv_out) {
    for (int j = 0; j < n; ++j) {
        const long long o = (long long)b * 2 * F + j;
        float g9[9];
        bool any = false;
        for (int i = 0; i < 9; ++i) { g9[i] = g[o * 9 + i]; any |= (g9[i] != 0.f); }
        if (gv_out)
            for (int i = 0; i < 9; ++i) gv_out[o * 9 + i] = 0.f;
        if (!any) continue;
        const int f = c2o[o];
        dbw::clip_slot_walk(verts, faces[f * 3], faces[f * 3 + 1], faces[f * 3 + 2], cam, eps, zc, persp, code[o], cw + o * 2, g9, [&](int i, int vi, dbw::f3 gv) {
            Sink{verts, cam, eps, acc}(i, vi, gv);
            if (gv_out) { gv_out[o * 9 + i * 3] = gv.x; gv_out[o * 9 + i * 3 + 1] = gv.y; gv_out[o * 9 + i * 3 + 2] = gv.z; }
            if (!abs_terms) return;
            if (n_terms) ++*n_terms;
            float one[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            Sink{verts, cam, eps, one}(i, vi, gv);
            for (int c = 0; c < 12; ++c) abs_terms[c] += std::fabs((double)one[c]);
        });
    }
}
