// Intrinsics refinement arithmetic shared by the device kernels (hipcc, camera_grad.hip) and the host (g++: tests/host_intrinsics_math.cpp,
// held by tests/test_host_intrinsics_math.py to autograd of the oracle and to a float64 restatement).  DESIGN.md 6t.
//
// Conventions are those of camera_math.h::project: K (4,4) row-major, shared by the views,
//   px = vx K[0] + vy K[1] + vz K[2] + K[3],  py from row 1 (K[4..7]),  pw from row 3 (K[12..15]);  row 2 (K[8..11]) is never read.
//
// Gradient of K.  With gpx, gpy, gpw the gradients of the three projected rows of a vertex (what camera_math.h::project_bwd forms from
// the ndc gradient g; gpw = 0 where |pw| < eps, the clamp of the denominator), the vertex adds gpx (vx, vy, vz, 1) to g_K[0..3],
// gpy (vx, vy, vz, 1) to g_K[4..7] and gpw (vx, vy, vz, 1) to g_K[12..15]: twelve accumulators acc[0..3], acc[4..7], acc[8..11], the full
// gradient of the matrix (row 2 is 0).  The depth component g.z reaches the view depth alone, which K does not touch.  KGradSink does that
// for every vertex camera_math.h::clip_slot_walk hands it: the three vertices of one clipped-face slot, through the one clipping case analysis.
//
// Refinement.  theta = (a_x, a_y, c_x, c_y): K' = K0 except K'[0] = K0[0] exp(a_x), K'[5] = K0[5] exp(a_y), K'[2] = K0[2] + c_x,
// K'[6] = K0[6] + c_y -- a scale of each focal length, an offset of the principal point in NDC units (half the shorter image side).
// theta = 0 returns K0 bit for bit: x + 0.f == x for every x, and the scale is refine_scale(a), which returns 1 for a == 0 WITHOUT calling
// expf.  IEEE 754 only recommends exp(0) == 1, and neither of the two libraries that serve this header (the device's OCML, the host's
// libm) states it for expf, so the identity rests on the branch and not on them.
#pragma once
#include "camera_math.h"

namespace dbw {

// ---- gradient of K --------------------------------------------------------------------------------------------------------------------
// one vertex: acc[0..3] += gpx (vx, vy, vz, 1), acc[4..7] += gpy (..), acc[8..11] += gpw (..)
DBW_HD void vertex_k_grad(const float *verts, int vi, const Cam &c, float eps, f3 g, float (&acc)[12]) {
    if (all_zero(g)) return;
    const ProjGrad p = project_bwd(verts + (long long)vi * 3, c, eps, g);
    const Proj &pr = p.pr;
    acc[0] += p.gpx * pr.vx; acc[1] += p.gpx * pr.vy; acc[2] += p.gpx * pr.vz; acc[3] += p.gpx;
    acc[4] += p.gpy * pr.vx; acc[5] += p.gpy * pr.vy; acc[6] += p.gpy * pr.vz; acc[7] += p.gpy;
    acc[8] += p.gpw * pr.vx; acc[9] += p.gpw * pr.vy; acc[10] += p.gpw * pr.vz; acc[11] += p.gpw;
}

// the sink of camera_math.h::clip_slot_walk that sums the gradient of K over the vertices it is handed
struct KGradSink {
    const float *verts;
    const Cam &c;
    float eps;
    float (&acc)[12];
    DBW_HD void operator()(int, int vi, f3 g) const { vertex_k_grad(verts, vi, c, eps, g, acc); }
};

// one clipped-face slot of one view: g = the nine gradient components of its three vertices, vi0..vi2 = the mesh face's vertex indices
DBW_HD void slot_k_grad(const float *verts, int vi0, int vi1, int vi2, const Cam &c, float eps, float zc, int persp, int cd, float w2, float w3,
                        const float (&g)[9], float (&acc)[12]) {
    const float cw2[2] = {w2, w3};
    clip_slot_walk(verts, vi0, vi1, vi2, c, eps, zc, persp, cd, cw2, g, KGradSink{verts, c, eps, acc});
}

// ---- refinement -----------------------------------------------------------------------------------------------------------------------
// exp(a), with 1 for a == 0 by a branch (see the head of the file)
DBW_HD float refine_scale(float a) { return a == 0.f ? 1.f : expf(a); }

// K' (16) from K0 (16) and theta = (a_x, a_y, c_x, c_y)
DBW_HD void intrinsics_apply(const float *K0, const float *theta, float *K1) {
#pragma unroll
    for (int i = 0; i < 16; ++i) K1[i] = K0[i];
    K1[0] = K0[0] * refine_scale(theta[0]);
    K1[5] = K0[5] * refine_scale(theta[1]);
    K1[2] = K0[2] + theta[2];
    K1[6] = K0[6] + theta[3];
}

// g_K' (16) -> g_theta (4): K0 is data and receives nothing
DBW_HD void intrinsics_chain(const float *K0, const float *theta, const float *gK, float *gtheta) {
    gtheta[0] = gK[0] * (K0[0] * refine_scale(theta[0]));
    gtheta[1] = gK[5] * (K0[5] * refine_scale(theta[1]));
    gtheta[2] = gK[2];
    gtheta[3] = gK[6];
}

}  // namespace dbw
