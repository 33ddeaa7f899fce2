// Arithmetic of the image scores (run_monitor.hip), written once for the device (hipcc) and for the host (g++:
// tests/test_host_score_math.py builds it into a checker-side shared object and compares it, without a GPU, with tests/golden/ssim.npz --
// the reference's own SSIMLoss -- and with the 2-D 11x11 definition evaluated in fp64; tests/test_gpu_monitor.py holds the kernel's map
// to the host build's bit for bit).
//
// SSIM as dbw_amd/metrics.py pins it against the reference (src/model/loss.py:124-156): an 11-tap Gaussian window, sigma 1.5, whose
// weights are computed in fp64, normalised and rounded to fp32 once; the five statistics a, b, a*a, b*b, a*b filtered along the rows first,
// then along the columns; C1 = 0.01^2, C2 = 0.03^2.  All fp32, one rounding per operation (-ffp-contract=off), in ONE fixed order, so that
// the host build and the device agree per pixel.  A filter is a compensated dot product over the taps k = 0 .. 10 (ssim_filter below): the
// variance E[x^2] - mu^2 of a flat region is the difference of two filtered values over C2 = 9e-4, and a plain left-to-right sum rounds
// eleven times at their full magnitude where this rounds once.
#pragma once
#include <math.h>
#include <stdint.h>

#include "raster_math.h"      // DBW_HD

namespace dbw {

constexpr int SSIM_TAPS = 11, SSIM_HALO = SSIM_TAPS - 1;

struct SsimWindow { float w[SSIM_TAPS]; };

// the window, on the host (both builds take it from here; the kernel receives it as an argument): exp(-x^2 / (2 sigma^2)) / sum in fp64,
// then one rounding to fp32 -- metrics.gaussian_window
inline SsimWindow ssim_window() {
    double g[SSIM_TAPS], s = 0.0;
    for (int k = 0; k < SSIM_TAPS; ++k) {
        const double x = (double)(k - SSIM_TAPS / 2);
        g[k] = exp(-x * x / (2.0 * 1.5 * 1.5));
        s += g[k];
    }
    SsimWindow win;
    for (int k = 0; k < SSIM_TAPS; ++k) win.w[k] = (float)(g[k] / s);
    return win;
}

// the five statistics of one pixel pair, in the order they are kept everywhere: a, b, a*a, b*b, a*b
DBW_HD void ssim_stats(float a, float b, float s[5]) {
    s[0] = a; s[1] = b; s[2] = a * a; s[3] = b * b; s[4] = a * b;
}

// one 11-tap filter: x[0 .. 10] under the window, as a compensated dot product (Ogita, Rump, Oishi 2005, Dot2): every product and every
// partial sum keeps its rounding error (fmaf and the branch-free two-sum give it exactly), the errors are added up on the side and join
// the sum at the end -- the result is the dot product as if evaluated in twice the precision, rounded once.
DBW_HD float ssim_filter(const float w[SSIM_TAPS], const float x[SSIM_TAPS]) {
    float s = 0.f, c = 0.f;
    for (int k = 0; k < SSIM_TAPS; ++k) {
        const float p = w[k] * x[k];
        const float ep = fmaf(w[k], x[k], -p);
        const float t = s + p;
        const float bb = t - s;
        const float es = (s - (t - bb)) + (p - bb);
        s = t;
        c = c + (es + ep);
    }
    return s + c;
}

// the filtered statistics mu1, mu2, E[a^2], E[b^2], E[ab] of one window -> its SSIM
DBW_HD float ssim_pixel(const float m[5]) {
    const float c1 = (float)(0.01 * 0.01), c2 = (float)(0.03 * 0.03);
    const float mu1_sq = m[0] * m[0], mu2_sq = m[1] * m[1], mu12 = m[0] * m[1];
    const float s11 = m[2] - mu1_sq, s22 = m[3] - mu2_sq, s12 = m[4] - mu12;
    const float n1 = 2.f * mu12 + c1, n2 = 2.f * s12 + c2;
    const float d1 = mu1_sq + mu2_sq + c1, d2 = s11 + s22 + c2;
    const float num = n1 * n2, den = d1 * d2;
    return num / den;
}

// ---- SSIM as a loss term (ssim_term.hip): L = mean over n, c, y, x of (1 - SSIM(a, b)), zero padding, and dL/db ------------------------
// With m = (mu1, mu2, Eaa, Ebb, Eab) the filtered statistics of the window at p and S = n1 n2 / (d1 d2) as ssim_pixel forms it, only
// mu2, Ebb and Eab depend on b, each linearly through the window:
//   A = dS/dmu2 = 2 [mu1 (n2 - n1) + mu2 S (d1 - d2)] / (d1 d2),     B = dS/dEbb = -S / d2,     C = dS/dEab = 2 n1 / (d1 d2)
//   dL/db_q = -(1/M) [blur(A)_q + 2 b_q blur(B)_q + a_q blur(C)_q]                    (the window is symmetric: blur is its own adjoint)
// A is written over the common denominator, without a division by n1 or n2 (n2 passes through 0 where the images are anticorrelated).
// Identical windows have n1 == d1, n2 == d2, mu1 == mu2 and S == 1 as floats; the forms below then give A == 0 and C == -2 B exactly
// (C as 2 (n1 / d1) / d2: the quotient is 1), so that blur(C) == -2 blur(B) and the gradient of rec == target is exactly 0, as it is at
// the minimum of the term.
// The three backward filters are ssim_filter too, the compensated dot product: in a flat region d2 comes down to C2 = 9e-4, so A, B and C
// are of the order 1 / C2 ~ 1e3 while their combination -- the gradient -- is of the order 1 or less (0 where rec == target): what the
// filters round at the magnitude of the maps stays in the gradient at full size.  A plain 11-term sum rounds eleven times at that
// magnitude per pass, the compensated one once.  The last combination is one expression in fp64 for the same reason (ssim_grad_pixel).
struct SsimDeriv { float S, A, B, C; };

DBW_HD SsimDeriv ssim_deriv(const float m[5]) {
    const float c1 = (float)(0.01 * 0.01), c2 = (float)(0.03 * 0.03);
    const float mu1_sq = m[0] * m[0], mu2_sq = m[1] * m[1], mu12 = m[0] * m[1];
    const float s11 = m[2] - mu1_sq, s22 = m[3] - mu2_sq, s12 = m[4] - mu12;
    const float n1 = 2.f * mu12 + c1, n2 = 2.f * s12 + c2;
    const float d1 = mu1_sq + mu2_sq + c1, d2 = s11 + s22 + c2;
    const float num = n1 * n2, den = d1 * d2;
    SsimDeriv r;
    r.S = num / den;                                         // (the operations of ssim_pixel, in its order: the same bits)
    const float t0 = m[0] * (n2 - n1), t1 = (m[1] * r.S) * (d1 - d2);
    r.A = (2.f * (t0 + t1)) / den;
    r.B = -(r.S / d2);
    r.C = (2.f * (n1 / d1)) / d2;
    return r;
}

// one element of the value: 1 - S of one window, every operation in fp64 on the fp32 statistics.  The value is a mean of 1 - S, and S as
// an fp32 number near 1 resolves 6e-8 of it: on a nearly black or a nearly perfect reconstruction, where 1 - S is 1e-3 or less, that is
// 1e-4 of the term and more.  Formed in fp64, what is left is the rounding of the five statistics, which scales with them.  Identical
// windows give exactly 0.
DBW_HD double ssim_loss_pixel(const float m[5]) {
    const double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;
    const double mu1 = (double)m[0], mu2 = (double)m[1];
    const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const double s11 = (double)m[2] - mu1_sq, s22 = (double)m[3] - mu2_sq, s12 = (double)m[4] - mu12;
    const double n1 = 2.0 * mu12 + c1, n2 = 2.0 * s12 + c2;
    const double d1 = mu1_sq + mu2_sq + c1, d2 = s11 + s22 + c2;
    return 1.0 - (n1 * n2) / (d1 * d2);
}

// one element of the gradient: fa, fb, fc = blur(A), blur(B), blur(C) at q, a / b the two images there, scale = -1 / M in fp64
DBW_HD float ssim_grad_pixel(float fa, float fb, float fc, float a, float b, double scale) {
    const double t = (double)fa + (2.0 * (double)b) * (double)fb + (double)a * (double)fc;
    return (float)(t * scale);
}

// one element of the squared-error sum: difference and square in fp64
DBW_HD double sq_err(float a, float b) {
    const double d = (double)a - (double)b;
    return d * d;
}

// one add of the loss meter: the value widened, times the weight, rounded, then added
DBW_HD double meter_add(double sum, float v, double weight) {
    const double p = (double)v * weight;
    return sum + p;
}

DBW_HD bool meter_finite(float v) { return (f2u(v) & 0x7f800000u) != 0x7f800000u; }

}  // namespace dbw
