// Arithmetic of the lens rectification (lens_undistort.hip), written once for the device (hipcc) and for the host (g++:
// tests/test_host_lens_math.py builds it into a checker-side shared object and holds it, without a GPU, to an fp64 restatement).
//
// A frame taken through a lens with OpenCV's radial-tangential distortion (the coefficient set k1..k4, p1, p2 of a Nerfstudio
// transforms.json) is resampled into the pinhole frame of the same size whose focal lengths are zoom * (fx, fy): output pixel (i, j) of an
// H x W frame reads the source at the INDEX coordinates (u, v),
//   x  = (j + 0.5 - cx) * inv_zfx            y  = (i + 0.5 - cy) * inv_zfy            (inv_zf* = 1 / (zoom * f*), rounded from fp64 by the host)
//   r2 = x*x + y*y
//   d  = 1 + r2*(k1 + r2*(k2 + r2*(k3 + r2*k4)))
//   xd = x*d + 2*p1*x*y + p2*(r2 + 2*x*x)    yd = y*d + 2*p2*x*y + p1*(r2 + 2*y*y)
//   u  = xd*fx + cx - 0.5                    v  = yd*fy + cy - 0.5
// with pixel centres at +0.5, the convention cx, cy of a transforms.json are given in.  All fp32, one rounding per operation in the order
// written below (both builds run with -ffp-contract=off), no division.  (u, v) is clamped to the frame, split into the corner
// (x0, y0) = (min((int)u, W - 2), min((int)v, H - 2)) and the weights (u - x0, v - y0), and each channel is blended in the order
//   a = p00 + (p01 - p00)*wx,  b = p10 + (p11 - p10)*wx,  val = a + (b - a)*wy,  byte = (int)(val + 0.5f).
// The clamps are written so that a NaN coordinate lands on 0: no lens value can send a read outside the frame.
#pragma once
#include <stdint.h>

#include "raster_math.h"      // DBW_HD

namespace dbw {

constexpr int LENS_N_PARAMS = 12;     // the `lens` array of dbw_images_undistort_u8, in the order of the struct below

struct LensParams {
    float fx, fy, cx, cy, inv_zfx, inv_zfy, k1, k2, k3, k4, p1, p2;
};

inline LensParams lens_params(const float *lens) {
    LensParams L;
    L.fx = lens[0]; L.fy = lens[1]; L.cx = lens[2]; L.cy = lens[3]; L.inv_zfx = lens[4]; L.inv_zfy = lens[5];
    L.k1 = lens[6]; L.k2 = lens[7]; L.k3 = lens[8]; L.k4 = lens[9]; L.p1 = lens[10]; L.p2 = lens[11];
    return L;
}

// The source index coordinates of output pixel (i, j), not clamped.
DBW_HD void lens_source(const LensParams &L, int i, int j, float *u, float *v) {
    const float x = ((float)j + 0.5f - L.cx) * L.inv_zfx, y = ((float)i + 0.5f - L.cy) * L.inv_zfy;
    const float xx = x * x, yy = y * y, xy = x * y;
    const float r2 = xx + yy;
    const float d = 1.0f + r2 * (L.k1 + r2 * (L.k2 + r2 * (L.k3 + r2 * L.k4)));
    const float xd = x * d + (2.0f * L.p1) * xy + L.p2 * (r2 + 2.0f * xx);
    const float yd = y * d + (2.0f * L.p2) * xy + L.p1 * (r2 + 2.0f * yy);
    *u = xd * L.fx + L.cx - 0.5f;
    *v = yd * L.fy + L.cy - 0.5f;
}

// Whether output pixel (i, j) reads inside the source frame: 0 <= u <= W - 1 and 0 <= v <= H - 1 of lens_source, not clamped (false for
// a NaN).  The validity mask of a frame rectified without a crop (dbw_lens_valid_u8).
DBW_HD bool lens_valid(const LensParams &L, int i, int j, int H, int W) {
    float u, v;
    lens_source(L, i, j, &u, &v);
    return u >= 0.0f && u <= (float)(W - 1) && v >= 0.0f && v <= (float)(H - 1);
}

// One axis of a sample: the coordinate clamped to [0, size - 1], the lower corner (at most size - 2) and the weight of the upper one.
DBW_HD int lens_split(float t, int size, float *w) {
    t = t > 0.0f ? t : 0.0f;                                  // (false for a NaN: 0)
    t = t > (float)(size - 1) ? (float)(size - 1) : t;
    int t0 = (int)t;
    t0 = t0 < size - 2 ? t0 : size - 2;
    *w = t - (float)t0;
    return t0;
}

// The bilinear sample of one output pixel: corner (x0, y0) with 0 <= x0 <= W - 2, 0 <= y0 <= H - 2, weights in [0, 1].
struct LensTap {
    int x0, y0;
    float wx, wy;
};
DBW_HD LensTap lens_tap(const LensParams &L, int i, int j, int H, int W) {
    float u, v;
    lens_source(L, i, j, &u, &v);
    LensTap t;
    t.x0 = lens_split(u, W, &t.wx);
    t.y0 = lens_split(v, H, &t.wy);
    return t;
}

// One channel: the four corners blended, rounded half up to a byte (val lies in [0, 255]).
DBW_HD uint8_t lens_blend(uint8_t p00, uint8_t p01, uint8_t p10, uint8_t p11, float wx, float wy) {
    const float f00 = (float)p00, f10 = (float)p10;
    const float a = f00 + ((float)p01 - f00) * wx;
    const float b = f10 + ((float)p11 - f10) * wx;
    const float val = a + (b - a) * wy;
    return (uint8_t)(int)(val + 0.5f);
}

}  // namespace dbw
