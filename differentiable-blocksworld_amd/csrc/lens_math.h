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

// ---- per-frame cameras rectified to one pinhole (lens_rectify.hip) -------------------------------------------------------------
// Every frame of a chunk has a source camera of its own -- a model id (0: the radial-tangential model above, 1: OpenCV's fisheye), fx, fy,
// cx, cy, k1..k4, p1, p2 -- and all of them are resampled into ONE target pinhole (cx0, cy0, 1/fx0, 1/fy0; the reciprocals rounded from
// fp64 by the host like inv_zf* above).  Output pixel (i, j) reads its frame at
//   x  = (j + 0.5 - cx0) * inv_fx0          y  = (i + 0.5 - cy0) * inv_fy0          r2 = x*x + y*y
//   model 0:  d, xd, yd, u, v as above with the source's k*, p*, fx, fy, cx, cy: where cx0 = cx, cy0 = cy, inv_f*0 = inv_zf* this is
//             lens_source operation for operation
//   model 1:  r  = sqrt(r2)                 th = atan(r)                            t2 = th*th
//             td = th*(1 + t2*(k1 + t2*(k2 + t2*(k3 + t2*k4))))
//             s  = td / r   (1 where r2 == 0: the principal point on a pixel centre)
//             u  = (x*s)*fx + cx - 0.5      v  = (y*s)*fy + cy - 0.5               (p1, p2 are not read)
// The arctangent is written here (lens_atan), from + - * and the IEEE division and square root both builds round correctly (hipcc's default,
// build.py; g++ -O2 has no fast-math): a library atanf differs between the device and the host, and the tests of this family compare bytes.
// It is the Cephes single-precision reduction for t >= 0,
//   t > tan(3 pi/8):  y0 = pi/2, a = -(1 / t)      t > tan(pi/8):  y0 = pi/4, a = (t - 1) / (t + 1)      else  y0 = 0, a = t
//   z = a*a,  q = ((A3*z + A2)*z + A1)*z + A0,  atan(t) = y0 + ((q*z)*a + a)
// one rounding per operation in this order.  Its relative error stays below 8 * 2^-24 (the account: tests/test_host_rectify_math.py, which
// measures 3.3 * 2^-24 at the worst of its arguments); the chain from r2 to (u, v) adds a rounding per
// operation, each relative to a value of at most the largest coordinate (tests/test_host_rectify_math.py holds the whole map to
// 64 * 2^-23 * max(H, W) px against fp64, the bound of the shared map).  A NaN fails every comparison, takes the last branch and stays a NaN
// up to the clamps of lens_split, which land it on 0.
constexpr int LENS_RECT_N_PARAMS = 16;    // a row of the `cams` table of dbw_lens_rectify_u8: the struct below and 5 floats of padding (64 bytes)
constexpr int LENS_RECT_PINHOLE = 0, LENS_RECT_FISHEYE = 1;     // (0: radial-tangential, a pinhole where every coefficient is 0)

struct LensCam {
    float model, fx, fy, cx, cy, k1, k2, k3, k4, p1, p2;
};
struct LensTarget {
    float cx0, cy0, inv_fx0, inv_fy0;
};

DBW_HD LensCam lens_cam(const float *row) {
    LensCam C;
    C.model = row[0]; C.fx = row[1]; C.fy = row[2]; C.cx = row[3]; C.cy = row[4];
    C.k1 = row[5]; C.k2 = row[6]; C.k3 = row[7]; C.k4 = row[8]; C.p1 = row[9]; C.p2 = row[10];
    return C;
}

DBW_HD LensTarget lens_target(const float *target) {
    LensTarget T;
    T.cx0 = target[0]; T.cy0 = target[1]; T.inv_fx0 = target[2]; T.inv_fy0 = target[3];
    return T;
}

// atan(t) for t >= 0 (the order of the operations: the comment above).
DBW_HD float lens_atan(float t) {
    float y0, a;
    if (t > 2.414213562373095f) {                               // tan(3 pi / 8)
        y0 = 1.5707963267948966f;
        a = -(1.0f / t);
    } else if (t > 0.4142135623730950f) {                       // tan(pi / 8)
        y0 = 0.7853981633974483f;
        a = (t - 1.0f) / (t + 1.0f);
    } else {
        y0 = 0.0f;
        a = t;
    }
    const float z = a * a;
    const float q = ((8.05374449538e-2f * z - 1.38776856032e-1f) * z + 1.99777106478e-1f) * z - 3.33329491539e-1f;
    return y0 + ((q * z) * a + a);
}

// The source index coordinates of output pixel (i, j) of the target in the frame of camera C, not clamped.
DBW_HD void lens_rect_source(const LensCam &C, const LensTarget &T, int i, int j, float *u, float *v) {
    const float x = ((float)j + 0.5f - T.cx0) * T.inv_fx0, y = ((float)i + 0.5f - T.cy0) * T.inv_fy0;
    const float xx = x * x, yy = y * y, xy = x * y;
    const float r2 = xx + yy;
    if (C.model == (float)LENS_RECT_FISHEYE) {
        const float r = __builtin_sqrtf(r2);
        const float th = lens_atan(r);
        const float t2 = th * th;
        const float td = th * (1.0f + t2 * (C.k1 + t2 * (C.k2 + t2 * (C.k3 + t2 * C.k4))));
        const float s = r2 == 0.0f ? 1.0f : td / r;
        *u = (x * s) * C.fx + C.cx - 0.5f;
        *v = (y * s) * C.fy + C.cy - 0.5f;
        return;
    }
    const float d = 1.0f + r2 * (C.k1 + r2 * (C.k2 + r2 * (C.k3 + r2 * C.k4)));
    const float xd = x * d + (2.0f * C.p1) * xy + C.p2 * (r2 + 2.0f * xx);
    const float yd = y * d + (2.0f * C.p2) * xy + C.p1 * (r2 + 2.0f * yy);
    *u = xd * C.fx + C.cx - 0.5f;
    *v = yd * C.fy + C.cy - 0.5f;
}

// lens_valid and lens_tap of a frame with a camera of its own.
DBW_HD bool lens_rect_valid(const LensCam &C, const LensTarget &T, int i, int j, int H, int W) {
    float u, v;
    lens_rect_source(C, T, i, j, &u, &v);
    return u >= 0.0f && u <= (float)(W - 1) && v >= 0.0f && v <= (float)(H - 1);
}
DBW_HD LensTap lens_rect_tap(const LensCam &C, const LensTarget &T, int i, int j, int H, int W) {
    float u, v;
    lens_rect_source(C, T, i, j, &u, &v);
    LensTap t;
    t.x0 = lens_split(u, W, &t.wx);
    t.y0 = lens_split(v, H, &t.wy);
    return t;
}

}  // namespace dbw
