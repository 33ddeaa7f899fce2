// Arithmetic of the depth cloud (depth_cloud.hip), written once for the device (hipcc) and for the host (g++:
// tests/host_depth_math.cpp builds it into a checker-side shared object, tests/test_host_depth_math.py holds it to an fp64 restatement).
//
// A capture ships one 16-bit depth map per frame.  Every depth sample of every frame goes through that frame's own lens and pose into the
// normalised world frame, and the samples are reduced on a voxel grid of G^3 cells to one point per occupied cell.  Per frame: an H x W
// grid of uint16 depths, a LensCam row and the LensTarget of lens_math.h (at the depth maps' resolution), and a pose row of 12 floats
// [A (3x3 row-major), t] -- the host folds the OpenGL flip and depth unit x normalisation scale into A.  For target pixel (i, j):
//   x = (j + 0.5 - cx0) * inv_fx0,  y = (i + 0.5 - cy0) * inv_fy0          as lens_rect_source forms them
//   (u, v) = lens_rect_source(...)                                         the frame's own lens
//   (sy, sx) = (floor(v + 0.5), floor(u + 0.5))                            the NEAREST source pixel: depth is never blended across an edge
//   dropped: a coordinate that is not finite or a pixel outside the frame; a depth d outside [d_min, d_max] (d_min >= 1: 0 is "no
//            measurement"); with edge_permille > 0, an in-frame 4-neighbour d_nb that is 0 or has 1000 * |d - d_nb| > edge_permille * d
//            (integers: the mixed pixels a depth sensor produces at a discontinuity)
//   c = (x*z, y*z, z),  z = (float)d
//   p_a = ((A[a][0]*c.x + A[a][1]*c.y) + A[a][2]*c.z) + t[a]
//   f_a = floorf((p_a - lo_a) * inv_step)                                  inv_step = G * 1024 / (hi - lo), rounded once from fp64 by the host
//   dropped (outside the box) unless 0 <= f_a < G * 1024 on all three axes; written so that a NaN drops, and the cast comes after it
//   q_a = (int)f_a,  cell = ((qx >> 10) * G + (qy >> 10)) * G + (qz >> 10)
// All fp32, one rounding per operation in the order written below (both builds run with -ffp-contract=off).  A cell accumulates integers
// only -- a uint32 count and three uint64 sums of q_a --, so any arrival order gives the same words.  Its point is formed in fp64 from
// + * / alone and rounded to fp32 once:  point_a = lo_a + ((sum_a + 0.5 * count) / count) / inv_step.
#pragma once
#include <stdint.h>

#include "lens_math.h"

namespace dbw {

constexpr int DEPTH_POSE_N = 12;          // floats of a pose row: A (3x3 row-major), t
constexpr int DEPTH_SUB_BITS = 10;        // a cell is 1024 quantisation steps wide
constexpr int DEPTH_MAX_GRID = 256;       // G^3 cells, G in [1, DEPTH_MAX_GRID]
constexpr int DEPTH_DROPPED = -1;         // depth_sample: no measurement here (lens, range, edge)
constexpr int DEPTH_OUTSIDE = -2;         // depth_sample: a measurement outside the box

struct DepthRule {
    int H, W, G, d_min, d_max, edge_permille;
};

// |d - nb| of an in-frame neighbour is a jump (nb == 0: no measurement next to this one)
DBW_HD bool depth_jump(int d, int nb, int edge_permille) {
    const int diff = d > nb ? d - nb : nb - d;
    return nb == 0 || 1000 * diff > edge_permille * d;
}

// The sample of target pixel (i, j) of one frame: its cell (>= 0) with q[3] filled, or DEPTH_DROPPED / DEPTH_OUTSIDE.
DBW_HD int depth_sample(const uint16_t *frame, const DepthRule &D, const LensCam &C, const LensTarget &T, const float *pose, const float *box,
                        int i, int j, int *q) {
    float u, v;
    lens_rect_source(C, T, i, j, &u, &v);
    const float fu = __builtin_floorf(u + 0.5f), fv = __builtin_floorf(v + 0.5f);
    if (!(fu >= 0.0f && fu <= (float)(D.W - 1) && fv >= 0.0f && fv <= (float)(D.H - 1))) return DEPTH_DROPPED;     // (a NaN, an infinity)
    const int sx = (int)fu, sy = (int)fv;
    const uint16_t *s = frame + ((long long)sy * D.W + sx);
    const int d = (int)s[0];
    if (d < D.d_min || d > D.d_max) return DEPTH_DROPPED;
    if (D.edge_permille > 0) {
        if (sx > 0 && depth_jump(d, (int)s[-1], D.edge_permille)) return DEPTH_DROPPED;
        if (sx < D.W - 1 && depth_jump(d, (int)s[1], D.edge_permille)) return DEPTH_DROPPED;
        if (sy > 0 && depth_jump(d, (int)s[-D.W], D.edge_permille)) return DEPTH_DROPPED;
        if (sy < D.H - 1 && depth_jump(d, (int)s[D.W], D.edge_permille)) return DEPTH_DROPPED;
    }
    const float x = ((float)j + 0.5f - T.cx0) * T.inv_fx0, y = ((float)i + 0.5f - T.cy0) * T.inv_fy0;
    const float z = (float)d;
    const float cx = x * z, cy = y * z;
    const float lim = (float)(D.G << DEPTH_SUB_BITS);
    for (int a = 0; a < 3; ++a) {
        const float p = ((pose[3 * a] * cx + pose[3 * a + 1] * cy) + pose[3 * a + 2] * z) + pose[9 + a];
        const float f = __builtin_floorf((p - box[a]) * box[3]);
        if (!(f >= 0.0f && f < lim)) return DEPTH_OUTSIDE;
        q[a] = (int)f;
    }
    return ((q[0] >> DEPTH_SUB_BITS) * D.G + (q[1] >> DEPTH_SUB_BITS)) * D.G + (q[2] >> DEPTH_SUB_BITS);
}

// The depth ray of target pixel (i, j) of one frame (dbw_lens_depth_rays): p[3] is the world point exactly as depth_sample
// forms p_a -- the same operations in the same order, the lens through lens_rect_source, the nearest source pixel -- and the result is
// false where depth_sample returns DEPTH_DROPPED (lens, range, edge rule; D.G is not read) or where a coordinate of p is not finite.  The
// box is not applied: a far end is still evidence of free space in front of it.
DBW_HD bool depth_ray_end(const uint16_t *frame, const DepthRule &D, const LensCam &C, const LensTarget &T, const float *pose, int i, int j,
                          float *p) {
    float u, v;
    lens_rect_source(C, T, i, j, &u, &v);
    const float fu = __builtin_floorf(u + 0.5f), fv = __builtin_floorf(v + 0.5f);
    if (!(fu >= 0.0f && fu <= (float)(D.W - 1) && fv >= 0.0f && fv <= (float)(D.H - 1))) return false;
    const int sx = (int)fu, sy = (int)fv;
    const uint16_t *s = frame + ((long long)sy * D.W + sx);
    const int d = (int)s[0];
    if (d < D.d_min || d > D.d_max) return false;
    if (D.edge_permille > 0) {
        if (sx > 0 && depth_jump(d, (int)s[-1], D.edge_permille)) return false;
        if (sx < D.W - 1 && depth_jump(d, (int)s[1], D.edge_permille)) return false;
        if (sy > 0 && depth_jump(d, (int)s[-D.W], D.edge_permille)) return false;
        if (sy < D.H - 1 && depth_jump(d, (int)s[D.W], D.edge_permille)) return false;
    }
    const float x = ((float)j + 0.5f - T.cx0) * T.inv_fx0, y = ((float)i + 0.5f - T.cy0) * T.inv_fy0;
    const float z = (float)d;
    const float cx = x * z, cy = y * z;
    bool finite = true;
    for (int a = 0; a < 3; ++a) {
        p[a] = ((pose[3 * a] * cx + pose[3 * a + 1] * cy) + pose[3 * a + 2] * z) + pose[9 + a];
        finite = finite && (p[a] - p[a] == 0.0f);
    }
    return finite;
}

// One coordinate of a cell's point: the mean of its samples' q (each at the middle of its step) back in the world frame.
DBW_HD float depth_point(unsigned long long sum, uint32_t count, float lo, float inv_step) {
    const double n = (double)count;
    return (float)((double)lo + (((double)sum + 0.5 * n) / n) / (double)inv_step);
}

}  // namespace dbw
