// Arithmetic of the gradient ICP (include/dbw_icp.h; reference src/utils/icp.py:11-78), written once for the device (hipcc, icp_align.hip) and
// for the host (g++, tests/test_host_icp_math.py builds tests/host_icp_math.cpp and compares it with torch without a GPU).  Both sides are
// built with -ffp-contract=off: one rounding per operation, in the order written here (an fmaf is one operation).
//
//  * transform:   q = (s * p) @ R + T as q_c = ((p0 * M0c + p1 * M1c) + p2 * M2c) + T_c with M_ac = s_a * R_ac, fp32.  The 12 floats
//                 M (row-major) | T are one instance's "block".
//  * moments:     the 13 sums of one direction -- |r|^2, r (3), p^T r (9) over its pairs, r = q - g in fp64 from the fp32 coordinates.
//  * chain:       dL/dT and dL/dM from the 2 x 13 sums (weights 2 / (N P1), 2 / (N P2)), then dR_ac = s_a dM_ac, ds_a = sum_c R_ac dM_ac
//                 (summed over a as well for an isotropic scale), dR6 = rot6d_bwd(dR).
//  * Adam:        torch.optim.Adam's single-tensor update (betas 0.9 / 0.999, eps 1e-8), parameters and moments in fp32, the step's scalars
//                 computed in fp64 on the host like Python computes them.
//  * keep-best:   icp.py:27-28,65-74 with its quirks.
#pragma once
#include <math.h>
#include <stdint.h>

#include "model_math.h"       // DBW_HD, Rot6, rot6d_fwd, rot6d_bwd

#pragma clang fp contract(off)

namespace dbw {

constexpr int ICP_NSUM = 13;          // sums per direction: loss, dT (3), dM (9)
constexpr int ICP_NPARAM = 12;        // R6 (6) | T (3) | s (3)
constexpr int ICP_NRTS = 15;          // R (9) | T (3) | s (3)
constexpr int ICP_CHECK_EVERY = 10;
constexpr double ICP_LOSS_MIN0 = 1e6;

// ---- transform ------------------------------------------------------------------------------------------------------------------------
DBW_HD void icp_block(const float *R, const float *T, const float *s, float *blk) {
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) blk[a * 3 + c] = s[a] * R[a * 3 + c];
    for (int c = 0; c < 3; ++c) blk[9 + c] = T[c];
}

DBW_HD void icp_transform(const float *blk, float p0, float p1, float p2, float *q) {
    for (int c = 0; c < 3; ++c) q[c] = ((p0 * blk[c] + p1 * blk[3 + c]) + p2 * blk[6 + c]) + blk[9 + c];
}

DBW_HD void icp_rotation(const float *R6, Rot6 &rot, float *R) {
    rot6d_fwd(R6, rot);
    for (int c = 0; c < 3; ++c) { R[c] = rot.b1[c]; R[3 + c] = rot.b2[c]; R[6 + c] = rot.b3[c]; }
}

// ---- moments of one pair: q the transformed pred point, g its ground-truth partner, p the untransformed pred point ---------------------
DBW_HD void icp_pair_moments(const float *q, const float *g, const float *p, double *acc) {
    const double r0 = (double)q[0] - (double)g[0], r1 = (double)q[1] - (double)g[1], r2 = (double)q[2] - (double)g[2];
    acc[0] += (r0 * r0 + r1 * r1) + r2 * r2;
    acc[1] += r0; acc[2] += r1; acc[3] += r2;
    const double p0 = p[0], p1 = p[1], p2 = p[2];
    acc[4] += p0 * r0; acc[5] += p0 * r1; acc[6] += p0 * r2;
    acc[7] += p1 * r0; acc[8] += p1 * r1; acc[9] += p1 * r2;
    acc[10] += p2 * r0; acc[11] += p2 * r1; acc[12] += p2 * r2;
}

// ---- from the 2 x 13 sums of an instance (direction 0: pred -> gt, P1 pairs; direction 1: gt -> pred, P2 pairs) -------------------------
DBW_HD double icp_instance_loss(const double *sums, int P1, int P2) { return sums[0] / (double)P1 + sums[ICP_NSUM] / (double)P2; }

DBW_HD void icp_grad_MT(const double *sums, int N, int P1, int P2, float *dM, float *dT) {
    const double w1 = 2.0 / ((double)N * (double)P1), w2 = 2.0 / ((double)N * (double)P2);
    for (int c = 0; c < 3; ++c) dT[c] = (float)(w1 * sums[1 + c] + w2 * sums[ICP_NSUM + 1 + c]);
    for (int k = 0; k < 9; ++k) dM[k] = (float)(w1 * sums[4 + k] + w2 * sums[ICP_NSUM + 4 + k]);
}

// dM -> gradients of R6 (6) and s (3; isotropic: gs[0] is the gradient of the one scale, gs[1] = gs[2] = 0)
DBW_HD void icp_chain(const Rot6 &rot, const float *R, const float *s, const float *dM, int anisotropic, float *gR6, float *gs) {
    float dR[9];
    for (int a = 0; a < 3; ++a) {
        for (int c = 0; c < 3; ++c) dR[a * 3 + c] = s[a] * dM[a * 3 + c];
        gs[a] = (R[a * 3] * dM[a * 3] + R[a * 3 + 1] * dM[a * 3 + 1]) + R[a * 3 + 2] * dM[a * 3 + 2];
    }
    if (!anisotropic) { gs[0] = (gs[0] + gs[1]) + gs[2]; gs[1] = gs[2] = 0.f; }
    rot6d_bwd(rot, dR, gR6);
}

// ---- Adam -----------------------------------------------------------------------------------------------------------------------------
// torch/optim/adam.py, _single_tensor_adam, on fp32 tensors (ATen's CPU kernels, which the device repeats operation by operation):
//   exp_avg.lerp_(grad, 1 - beta1)                        m + w * (g - m), ONE fused multiply-add (Lerp.h, weight < 0.5)
//   exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)  v * beta2 + ((1 - beta2) * g) * g, the last product and the sum ONE fused
//                                                         multiply-add (torch's vectorised CPU kernel contracts them; held bit for bit by the test)
//   denom = (exp_avg_sq.sqrt() / bias_correction2 ** 0.5).add_(eps)
//   param.addcdiv_(exp_avg, denom, value=-lr / bias_correction1)      p + ((-step_size) * m) / denom
// The scalars are Python floats (fp64), rounded to fp32 where they meet the tensor.
struct IcpAdam {
    float step_size;          // (float)(lr / (1 - 0.9 ** step))
    float bc2_sqrt;           // (float)((1 - 0.999 ** step) ** 0.5)
};

inline IcpAdam icp_adam_scalars(double lr, int step) {      // host only: the launch passes the result to the kernel
    IcpAdam a;
    a.step_size = (float)(lr / (1.0 - pow(0.9, (double)step)));
    a.bc2_sqrt = (float)pow(1.0 - pow(0.999, (double)step), 0.5);
    return a;
}

DBW_HD void icp_adam_update(float &p, float &m, float &v, float g, IcpAdam a) {
    const float w1 = (float)(1.0 - 0.9), w2 = (float)(1.0 - 0.999);
    m = fmaf(w1, g - m, m);
    v = fmaf(w2 * g, g, v * 0.999f);
    const float denom = sqrtf(v) / a.bc2_sqrt + 1e-8f;
    p = p + ((-a.step_size) * m) / denom;
}

// One instance's iteration behind the sums: gradients, Adam on R6 | T | s, the parameters after the step as R | T | s (rts, 15) and as the
// next block (blk, 12).  param / m / v: 12 floats each, R6 | T | s; with an isotropic scale param[9] is the parameter and [10], [11] copy it.
DBW_HD void icp_step(float *param, float *m, float *v, const double *sums, int N, int P1, int P2, int estimate_scale, int anisotropic,
                     IcpAdam a, float *blk, float *rts) {
    Rot6 rot;
    float R[9], dM[9], dT[3], g[ICP_NPARAM];
    icp_rotation(param, rot, R);
    icp_grad_MT(sums, N, P1, P2, dM, dT);
    icp_chain(rot, R, param + 9, dM, anisotropic, g, g + 9);
    for (int c = 0; c < 3; ++c) g[6 + c] = dT[c];
    const int n_adam = estimate_scale ? (anisotropic ? 12 : 10) : 9;
    for (int k = 0; k < n_adam; ++k) icp_adam_update(param[k], m[k], v[k], g[k], a);
    if (estimate_scale && !anisotropic) param[10] = param[11] = param[9];
    icp_rotation(param, rot, rts);
    for (int c = 0; c < 3; ++c) { rts[9 + c] = param[6 + c]; rts[12 + c] = param[9 + c]; }
    icp_block(rts, rts + 9, rts + 12, blk);
}

DBW_HD void icp_identity(float *param, float *rts, float *blk) {
    for (int k = 0; k < ICP_NPARAM; ++k) param[k] = (k == 0 || k == 4 || k >= 9) ? 1.f : 0.f;
    for (int k = 0; k < ICP_NRTS; ++k) rts[k] = (k == 0 || k == 4 || k == 8 || k >= 12) ? 1.f : 0.f;
    icp_block(rts, rts + 9, rts + 12, blk);
}

// ---- keep-best (icp.py:27-28,65-74) -----------------------------------------------------------------------------------------------------
// loss_min starts at 1e6; the meter (utils/metrics.py:17-35, updated with N = the batch size) averages the batch-mean loss since its last
// reset; it is looked at when it % 10 == 0 and reset at every look.  What the caller keeps on `true` are the parameters AFTER iteration
// it's Adam step, paired with an average of losses taken before those steps.  best_iter stays -1 while nothing beat 1e6: the caller's kept
// parameters are then still the identity it started from.
struct IcpMeter {
    double sum, count, loss_min, best_iter;
};

DBW_HD void icp_meter_init(IcpMeter &m) { m.sum = 0.0; m.count = 0.0; m.loss_min = ICP_LOSS_MIN0; m.best_iter = -1.0; }

DBW_HD bool icp_keep_best(IcpMeter &m, double loss, int N, int it) {
    m.sum += loss * (double)N;
    m.count += (double)N;
    if (it % ICP_CHECK_EVERY != 0) return false;
    const double avg = m.count != 0.0 ? m.sum / m.count : 0.0;
    const bool keep = avg < m.loss_min;
    if (keep) { m.loss_min = avg; m.best_iter = (double)it; }
    m.sum = 0.0;
    m.count = 0.0;
    return keep;
}

}  // namespace dbw
