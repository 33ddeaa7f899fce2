// Per-view exposure compensation (exposure_loss.hip), host + device: the arithmetic of one pixel, compiled by hipcc for the
// kernels and by g++ for tests/test_host_exposure_math.py.  A view carries theta = (g_r, g_g, g_b, b_r, b_g, b_b); with the decoupled
// composite comp_c = fg_c * alpha + (1 - alpha) * env_c (loss_math.h) the compensated image is
//   rec_c = exp(g_c) * comp_c + b_c                                  (no clamp; theta = 0: rec == comp bit for bit, 1 * x + 0 == x)
// and the reconstruction term scale * sum m (rec - img)^2 with the validity weight m of the pixel (1 without masks).
#pragma once
#include <math.h>

#include "raster_math.h"      // DBW_HD

namespace dbw {

// theta[0..2] -> the three gains exp(g_c): once per view, not per pixel
DBW_HD void exposure_gains(const float theta[6], float gain[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) gain[c] = expf(theta[c]);
}

// forward of one pixel: rec[3], returns m * sum_c (rec_c - target_c)^2
DBW_HD float exposure_forward_pixel(const float fc[3], float alpha, const float ec[3], const float target[3], float m, const float gain[3],
                                    const float bias[3], float rec[3]) {
    float part = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float comp = fc[c] * alpha + (1.f - alpha) * ec[c];
        rec[c] = gain[c] * comp + bias[c];
        const float d = rec[c] - target[c];
        part += d * d;
    }
    return m * part;
}

// backward of one pixel.  rec is formed again; per channel d'_c = (two_scale * m) * (rec_c - target_c) + extra_c is the gradient that
// arrives at rec -- two_scale = 2 * scale * (the upstream scalar), extra the perceptual term's d/d rec (has_extra: a flag next to the
// values, as in loss_math.h) -- and d_c = exp(g_c) * d'_c what goes on through the composite:
//   gf = d * alpha, ge = d * (1 - alpha), galpha = sum_c d_c (fc_c - ec_c).
// sums[c] = d'_c * exp(g_c) * comp_c and sums[3 + c] = d'_c: the pixel's contribution to d loss / d (g_c, b_c) of its view.
DBW_HD void exposure_backward_pixel(const float fc[3], float alpha, const float ec[3], const float target[3], float m, const float gain[3],
                                    const float bias[3], float two_scale, const float extra[3], bool has_extra, float gf[3], float ge[3],
                                    float &galpha, float sums[6]) {
    const float wm = two_scale * m;
    galpha = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float comp = fc[c] * alpha + (1.f - alpha) * ec[c];
        const float lit = gain[c] * comp;
        const float d = (lit + bias[c]) - target[c];
        const float dp = has_extra ? wm * d + extra[c] : wm * d;
        const float dc = gain[c] * dp;
        gf[c] = dc * alpha;
        ge[c] = dc * (1.f - alpha);
        galpha += dc * (fc[c] - ec[c]);
        sums[c] = dp * lit;
        sums[3 + c] = dp;
    }
}

}  // namespace dbw
