// Arithmetic of the image ingest (image_ingest.hip), written once for the device (hipcc) and for the host (g++:
// tests/test_host_resample_math.py builds it into a checker-side shared object and compares it, without a GPU, with the bytes Pillow makes).
//
// The reference's datasets make their targets with Compose([Resize(img_size), ToTensor()]) on a PIL image (src/dataset/dtu.py:70-72,
// bmvs.py:61-63): Pillow's antialiased BILINEAR resample of an 8-bit image, then uint8 / 255 in fp32.  Pillow's resample is integer
// arithmetic behind a double-precision coefficient table, so it is restated here bit for bit:
//  * per axis (`in` input samples, `out` output samples), in double: scale = in / out, support = max(scale, 1); output sample xx has its
//    centre at (xx + 0.5) * scale and takes the input samples [xmin, xmax) = [max((int)(centre - support + 0.5), 0),
//    min((int)(centre + support + 0.5), in)); sample x weighs max(0, 1 - |x - centre + 0.5| / support), the weights are divided by
//    their sum and rounded to 22 fractional bits, k = (int)(w * 2^22 + 0.5) (half away from zero; they are never negative);
//  * per output sample and channel, in int32: acc = 2^21 + sum pixel[xmin + x] * k[x], result = clamp(acc >> 22, 0, 255);
//  * the horizontal pass runs first and rounds to 8 bits, the vertical pass runs on that intermediate;
//  * ToTensor: float(u8) / 255.0f, one IEEE fp32 division.
// A table row is [xmin, n, k_0 .. k_{ksize-1}] (zero padded), ksize = (int)ceil(support) * 2 + 1.
#pragma once
#include <math.h>
#include <stdint.h>

#include "raster_math.h"      // DBW_HD

namespace dbw {

constexpr int RESAMPLE_BITS = 22;                           // Pillow's PRECISION_BITS for 8-bit pixels: 32 - 8 - 2
constexpr int32_t RESAMPLE_HALF = 1 << (RESAMPLE_BITS - 1); // the rounding constant every accumulator starts from
constexpr int32_t RESAMPLE_ONE = 1 << RESAMPLE_BITS;        // the weight of an axis that keeps its size (one tap)

inline double resample_support(int in, int out) {
    const double scale = (double)in / (double)out;
    return scale < 1.0 ? 1.0 : scale;
}

// Width of a table row's weights.
inline int resample_ksize(int in, int out) { return (int)ceil(resample_support(in, out)) * 2 + 1; }

// The input samples output sample xx reads: [*xmin, *xmin + n), n returned.
inline int resample_bounds(int in, int out, int xx, int *xmin) {
    const double scale = (double)in / (double)out, support = resample_support(in, out);
    const double center = (xx + 0.5) * scale;
    int lo = (int)(center - support + 0.5), hi = (int)(center + support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > in) hi = in;
    *xmin = lo;
    return hi - lo;
}

// One table row: row[0] = xmin, row[1] = n, row[2 .. 2 + ksize) the fixed-point weights.
inline void resample_table_row(int in, int out, int xx, int ksize, int32_t *row) {
    const double scale = (double)in / (double)out, support = resample_support(in, out), ss = 1.0 / support;
    const double center = (xx + 0.5) * scale;
    int xmin;
    const int n = resample_bounds(in, out, xx, &xmin);
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
        double t = (x + xmin - center + 0.5) * ss;
        if (t < 0.0) t = -t;
        ww += t < 1.0 ? 1.0 - t : 0.0;
    }
    row[0] = xmin;
    row[1] = n;
    for (int x = 0; x < ksize; ++x) {
        double w = 0.0;
        if (x < n) {
            double t = (x + xmin - center + 0.5) * ss;
            if (t < 0.0) t = -t;
            w = t < 1.0 ? 1.0 - t : 0.0;
            if (ww != 0.0) w /= ww;
        }
        row[2 + x] = w < 0.0 ? (int32_t)(-0.5 + w * (double)RESAMPLE_ONE) : (int32_t)(0.5 + w * (double)RESAMPLE_ONE);
    }
}

// acc >> 22 clamped to a byte.  The accumulator cannot overflow: the n weights of a row are each rounded up by at most 0.5 / 2^22, so
// their sum is at most 2^22 + n / 2, and acc <= 2^21 + 255 * (2^22 + n / 2) < 2^31 for every n below 2^23 -- more taps than an image
// axis has samples.
DBW_HD uint8_t resample_clip8(int32_t acc) {
    const int32_t v = acc >> RESAMPLE_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// One output sample of one pass: n taps `stride` bytes apart.
DBW_HD uint8_t resample_dot(const uint8_t *px, long long stride, const int32_t *k, int n) {
    int32_t acc = RESAMPLE_HALF;
    for (int x = 0; x < n; ++x) acc += (int32_t)px[x * stride] * k[x];
    return resample_clip8(acc);
}

// ToTensor
DBW_HD float resample_to_float(uint8_t v) { return (float)v / 255.0f; }

}  // namespace dbw
