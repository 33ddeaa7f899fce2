// Camera pose refinement arithmetic shared by the device kernels (hipcc, camera_grad.hip) and the host (g++: tests/host_pose_math.cpp, held
// by tests/test_host_pose_math.py to autograd of the oracle and to a float64 restatement).  DESIGN.md 6o.
//
// Conventions are those of camera_math.h::project: row vectors, v = X.R + T, R row-major, v_c = sum_r X_r R[3r + c] + T_c.
//
// Gradient of a view's camera.  With gview the view-space gradient of a vertex (camera_math.h::view_grad), the vertex adds gview to g_T
// and X_r * gview_c to g_R[3r + c].  CamGradSink does that for every vertex camera_math.h::clip_slot_walk hands it: the three vertices of one
// clipped-face slot, through the one clipping case analysis.
//
// Refinement.  A view's 6-vector delta = (w, tau) perturbs the camera in its own frame: v' = v.E(w) + tau, hence R' = R.E, T' = T.E + tau.
// E = I + a K + b K^2 with th = |w|, a = sin th / th, b = (1 - cos th) / th^2 and
//        (  0  -wz   wy )
//   K =  (  wz   0  -wx )        K x = w x x for a COLUMN x, E = exp(K).  The row-vector product v.E is (E^T v^T)^T: the view-space point is
//        ( -wy   wx   0 )        turned by -w about the camera centre.  dE/dw_i at 0 is the generator G_i = dK/dw_i.
// Below th^2 < POSE_SERIES_T the four coefficients come from their series in t = th^2 (four terms: the first one left out is below 1e-10
// relative there), so w = 0 gives E = I exactly and a finite, correct gradient.
#pragma once
#include "camera_math.h"

namespace dbw {

constexpr float POSE_SERIES_T = 0.0625f;     // th < 0.25

// ---- gradient of a view's camera ------------------------------------------------------------------------------------------------------
// one vertex: acc[0..8] += X_r * gview_c (g_R, row-major), acc[9..11] += gview (g_T)
DBW_HD void vertex_cam_grad(const float *verts, int vi, const Cam &c, float eps, f3 g, float (&acc)[12]) {
    if (all_zero(g)) return;
    const float *X = verts + (long long)vi * 3;
    const f3 gv = view_grad(project_bwd(X, c, eps, g), c, g);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        acc[r * 3] += X[r] * gv.x; acc[r * 3 + 1] += X[r] * gv.y; acc[r * 3 + 2] += X[r] * gv.z;
    }
    acc[9] += gv.x; acc[10] += gv.y; acc[11] += gv.z;
}

// the sink of camera_math.h::clip_slot_walk that sums a view's camera gradient over the vertices it is handed
struct CamGradSink {
    const float *verts;
    const Cam &c;
    float eps;
    float (&acc)[12];
    DBW_HD void operator()(int, int vi, f3 g) const { vertex_cam_grad(verts, vi, c, eps, g, acc); }
};

// one clipped-face slot of one view: g = the nine gradient components of its three vertices, vi0..vi2 = the mesh face's vertex indices
DBW_HD void slot_cam_grad(const float *verts, int vi0, int vi1, int vi2, const Cam &c, float eps, float zc, int persp, int cd, float w2, float w3,
                          const float (&g)[9], float (&acc)[12]) {
    const float cw2[2] = {w2, w3};
    clip_slot_walk(verts, vi0, vi1, vi2, c, eps, zc, persp, cd, cw2, g, CamGradSink{verts, c, eps, acc});
}

// ---- refinement -----------------------------------------------------------------------------------------------------------------------
struct RodCoef {
    float a, b;       // sin th / th, (1 - cos th) / th^2
    float c1, c2;     // (da/dth) / th = (th cos th - sin th) / th^3, (db/dth) / th = (th sin th - 2 (1 - cos th)) / th^4
};

DBW_HD RodCoef rodrigues_coef(const float *w) {
    const float t = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    RodCoef k;
    if (t < POSE_SERIES_T) {
        k.a = 1.f + t * (-1.f / 6.f + t * (1.f / 120.f + t * (-1.f / 5040.f)));
        k.b = 0.5f + t * (-1.f / 24.f + t * (1.f / 720.f + t * (-1.f / 40320.f)));
        k.c1 = -1.f / 3.f + t * (1.f / 30.f + t * (-1.f / 840.f + t * (1.f / 45360.f)));
        k.c2 = -1.f / 12.f + t * (1.f / 180.f + t * (-1.f / 6720.f + t * (1.f / 453600.f)));
    } else {
        const float th = sqrtf(t), s = sinf(th), c = cosf(th);
        k.a = s / th;
        k.b = (1.f - c) / t;
        k.c1 = (th * c - s) / (t * th);
        k.c2 = (th * s - 2.f * (1.f - c)) / (t * t);
    }
    return k;
}

// E (3,3) row-major = exp([w]x)
DBW_HD void rodrigues(const float *w, float *E) {
    const RodCoef k = rodrigues_coef(w);
    const float x = w[0], y = w[1], z = w[2], t = x * x + y * y + z * z;
    E[0] = 1.f + k.b * (x * x - t); E[1] = k.a * -z + k.b * (x * y);    E[2] = k.a * y + k.b * (x * z);
    E[3] = k.a * z + k.b * (y * x); E[4] = 1.f + k.b * (y * y - t);     E[5] = k.a * -x + k.b * (y * z);
    E[6] = k.a * -y + k.b * (z * x); E[7] = k.a * x + k.b * (z * y);    E[8] = 1.f + k.b * (z * z - t);
}

// gw[i] = sum_jk gE[3j + k] dE[3j + k] / dw_i
DBW_HD void rodrigues_bwd(const float *w, const float *gE, float *gw) {
    const RodCoef k = rodrigues_coef(w);
    const float x = w[0], y = w[1], z = w[2], t = x * x + y * y + z * z;
    // <gE, K>, <gE, K^2> (K^2 = w w^T - t I), trace
    const float gK = (gE[7] - gE[5]) * x + (gE[2] - gE[6]) * y + (gE[3] - gE[1]) * z;
    const float tr = gE[0] + gE[4] + gE[8];
    const float gKK = gE[0] * (x * x) + gE[4] * (y * y) + gE[8] * (z * z) + (gE[1] + gE[3]) * (x * y) + (gE[2] + gE[6]) * (x * z) + (gE[5] + gE[7]) * (y * z)
                      - t * tr;
    const float radial = k.c1 * gK + k.c2 * gKK;
    // <gE, G_i> and <gE, d(K^2)/dw_i> = sum_k (gE[i][k] + gE[k][i]) w_k - 2 w_i tr
    const float sx = (gE[0] + gE[0]) * x + (gE[1] + gE[3]) * y + (gE[2] + gE[6]) * z - 2.f * x * tr;
    const float sy = (gE[3] + gE[1]) * x + (gE[4] + gE[4]) * y + (gE[5] + gE[7]) * z - 2.f * y * tr;
    const float sz = (gE[6] + gE[2]) * x + (gE[7] + gE[5]) * y + (gE[8] + gE[8]) * z - 2.f * z * tr;
    gw[0] = x * radial + k.a * (gE[7] - gE[5]) + k.b * sx;
    gw[1] = y * radial + k.a * (gE[2] - gE[6]) + k.b * sy;
    gw[2] = z * radial + k.a * (gE[3] - gE[1]) + k.b * sz;
}

// R' = R0.E(w), T' = T0.E(w) + tau for delta = (w, tau); R0, R' (3,3) row-major
DBW_HD void pose_apply(const float *R0, const float *T0, const float *delta, float *R1, float *T1) {
    float E[9];
    rodrigues(delta, E);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R1[r * 3 + c] = R0[r * 3] * E[c] + R0[r * 3 + 1] * E[3 + c] + R0[r * 3 + 2] * E[6 + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) T1[c] = T0[0] * E[c] + T0[1] * E[3 + c] + T0[2] * E[6 + c] + delta[3 + c];
}

// (g_R', g_T') -> g_delta (6): R0, T0 are data and receive nothing
DBW_HD void pose_chain(const float *R0, const float *T0, const float *delta, const float *gR, const float *gT, float *gdelta) {
    float gE[9];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) gE[k * 3 + c] = R0[k] * gR[c] + R0[3 + k] * gR[3 + c] + R0[6 + k] * gR[6 + c] + T0[k] * gT[c];
    rodrigues_bwd(delta, gE, gdelta);
    gdelta[3] = gT[0]; gdelta[4] = gT[1]; gdelta[5] = gT[2];
}

}  // namespace dbw
