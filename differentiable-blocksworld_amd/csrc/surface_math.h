// Arithmetic of the surface term (host + device: tests/test_host_surface_math.py checks the g++ build against an fp64 numpy reference
// written from the definition, tests/test_gpu_surface.py holds the kernels of csrc/surface_term.hip to the host build byte for byte).
// No reference counterpart: the reference has no geometric supervision.  Every fp32 step is + - * / sqrt with one rounding per
// operation (-ffp-contract=off on both builds; hipcc's fp32 divide is IEEE).
//
//   closest point  of p on the triangle (a, b, c), e1 = b - a, e2 = c - a, n = e1 x e2, q = p - a:
//                    the projection onto the plane has u = ((q x e2) . n) / (n . n), v = ((e1 x q) . n) / (n . n); it is accepted when
//                    u >= 0, v >= 0 and u + v <= 1, else the best of the clamped projections onto ab, bc, ca (in that order, a later one
//                    only when strictly nearer; surface_side_wins has the one exception) is taken.  A face with n . n == 0, or a sliver
//                    (SURFACE_SLIVER), goes to its segments, a segment of zero length to its first end: no division by zero, nothing but finite numbers from finite input.
//                  d2 is always |p - (a + (u e1 + v e2))|^2 of the (u, v) that is returned, never the plane's distance: value, record and
//                  gradient speak of the same point.  b = (1 - u - v, u, v).
//   key            (bits(d2) << 32) | face, dbw::nn_key: the smallest key is the smallest d2, the lowest face on ties
//   box bound      a lower bound of d2 over everything inside an axis-aligned box, made smaller by SURFACE_BOX_SLACK of the largest
//                  coordinate in play and by a factor: the d2 above is the distance to a point that rounding may have moved off the face by
//                  a few ulp of the coordinates, so the exact distance to the box is not a bound of it, this is
//   draw           the cloud index of draw i of a step: step_random(seed, step, stream 2, i).x mod N
#pragma once
#include "nn_math.h"          // nn_key
#include "rng_math.h"

#pragma clang fp contract(off)

namespace dbw {

constexpr int SURFACE_SEGMENT = 1024;           // records a backward workgroup walks by default (DBW_EVAL_SURFACE_SEGMENT)
constexpr uint32_t SURFACE_STREAM = 2u;         // the draw's stream of step_random (0: opacity noise, 1: overlap samples)
constexpr float SURFACE_BOX_SLACK = 1.52587890625e-5f;      // 2^-16 = 256 ulp of the largest coordinate
constexpr float SURFACE_BOX_FACTOR = 0.9999f;
constexpr float SURFACE_SIDE_TIE = 9.5367431640625e-7f;     // 2^-20
// A face whose sin^2 of the angle at a is at most this (n.n <= 2^-24 |e1|^2 |e2|^2; zero area included) has no plane branch: the cross
// products that give (u, v) cancel to a relative 2^-24 / sin, which meets the sliver's own width, sin |e|, at sin = 2^-12 -- below it the
// sides are the better answer, and no interior point of such a face is farther than 2^-13 |e| from one of them.
constexpr float SURFACE_SLIVER = 5.9604644775390625e-8f;

struct SurfaceHit { float d2, u, v; };

DBW_HD float surface_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// the clamped projection of q (relative to the segment's start) onto the direction d: t in [0, 1], 0 for a segment of zero length
DBW_HD float surface_segment_t(float qx, float qy, float qz, float dx, float dy, float dz) {
    const float dd = surface_dot(dx, dy, dz, dx, dy, dz);
    if (!(dd > 0.f)) return 0.f;
    const float t = surface_dot(qx, qy, qz, dx, dy, dz) / dd;
    return t > 0.f ? (t < 1.f ? t : 1.f) : 0.f;          // (NaN: 0)
}

// |q - (u e1 + v e2)|^2
DBW_HD float surface_d2_at(float qx, float qy, float qz, const float *e1, const float *e2, float u, float v) {
    const float rx = qx - (u * e1[0] + v * e2[0]), ry = qy - (u * e1[1] + v * e2[1]), rz = qz - (u * e1[2] + v * e2[2]);
    return (rx * rx + ry * ry) + rz * rz;
}

// Does a side's candidate (d2, inner: its projection was not clamped) replace the best so far?  The strictly nearer one wins -- but a foot
// point inside a side is, in exact arithmetic, no farther than that side's ends, which are what the other sides' clamped projections give,
// and next to a corner the two d2 differ by the SQUARE of the foot's distance from the corner: fp32 cannot tell them apart long before the
// points coincide.  So within SURFACE_SIDE_TIE, relatively, an unclamped projection beats a clamped one whatever the order of the d2.
DBW_HD bool surface_side_wins(float d2, bool inner, float best, bool best_inner) {
    if (inner == best_inner) return d2 < best;
    if (inner) return d2 <= best + SURFACE_SIDE_TIE * best;
    return d2 + SURFACE_SIDE_TIE * d2 < best;
}

// t: the 9 coordinates a, b, c of the face
DBW_HD SurfaceHit surface_closest(const float *t, float px, float py, float pz) {
    const float e1[3] = {t[3] - t[0], t[4] - t[1], t[5] - t[2]}, e2[3] = {t[6] - t[0], t[7] - t[1], t[8] - t[2]};
    const float qx = px - t[0], qy = py - t[1], qz = pz - t[2];
    const float nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
    const float nn = surface_dot(nx, ny, nz, nx, ny, nz);
    SurfaceHit h;
    if (nn > SURFACE_SLIVER * (surface_dot(e1[0], e1[1], e1[2], e1[0], e1[1], e1[2]) * surface_dot(e2[0], e2[1], e2[2], e2[0], e2[1], e2[2]))) {
        const float ax = qy * e2[2] - qz * e2[1], ay = qz * e2[0] - qx * e2[2], az = qx * e2[1] - qy * e2[0];       // q x e2
        const float bx = e1[1] * qz - e1[2] * qy, by = e1[2] * qx - e1[0] * qz, bz = e1[0] * qy - e1[1] * qx;       // e1 x q
        const float u = surface_dot(ax, ay, az, nx, ny, nz) / nn, v = surface_dot(bx, by, bz, nx, ny, nz) / nn;
        if (u >= 0.f && v >= 0.f && u + v <= 1.f) {
            h.u = u; h.v = v; h.d2 = surface_d2_at(qx, qy, qz, e1, e2, u, v);
            return h;
        }
    }
    // ab: (u, v) = (s, 0); bc: (1 - s, s); ca: (0, 1 - s)
    float s = surface_segment_t(qx, qy, qz, e1[0], e1[1], e1[2]);
    bool inner = s > 0.f && s < 1.f;
    h.u = s; h.v = 0.f; h.d2 = surface_d2_at(qx, qy, qz, e1, e2, s, 0.f);
    s = surface_segment_t(qx - e1[0], qy - e1[1], qz - e1[2], e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2]);
    float d2 = surface_d2_at(qx, qy, qz, e1, e2, 1.f - s, s);
    if (surface_side_wins(d2, s > 0.f && s < 1.f, h.d2, inner)) { h.u = 1.f - s; h.v = s; h.d2 = d2; inner = s > 0.f && s < 1.f; }
    s = surface_segment_t(qx - e2[0], qy - e2[1], qz - e2[2], -e2[0], -e2[1], -e2[2]);
    d2 = surface_d2_at(qx, qy, qz, e1, e2, 0.f, 1.f - s);
    if (surface_side_wins(d2, s > 0.f && s < 1.f, h.d2, inner)) { h.u = 0.f; h.v = 1.f - s; h.d2 = d2; }
    return h;
}

DBW_HD uint64_t surface_key(float d2, uint32_t face) { return nn_key(d2, face); }
DBW_HD float surface_key_d2(uint64_t key) {
    union { float f; uint32_t u; } c;
    c.u = (uint32_t)(key >> 32);
    return c.f;
}

DBW_HD float surface_max3(float a, float b, float c) { const float m = a > b ? a : b; return m > c ? m : c; }

// lo, hi: the box (3 each).  Never above the d2 that surface_closest gives for a face whose vertices lie in the box.
DBW_HD float surface_box_bound(const float *lo, const float *hi, float px, float py, float pz) {
    const float p[3] = {px, py, pz};
    float scale = 0.f, g[3];
    for (int k = 0; k < 3; ++k) scale = surface_max3(scale, surface_max3(fabsf(p[k]), fabsf(lo[k]), fabsf(hi[k])), 0.f);
    const float slack = SURFACE_BOX_SLACK * scale;
    for (int k = 0; k < 3; ++k) {
        const float out = surface_max3(lo[k] - p[k], p[k] - hi[k], 0.f) - slack;
        g[k] = out > 0.f ? out : 0.f;
    }
    return SURFACE_BOX_FACTOR * ((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
}

// the cloud index of draw i (n_cloud >= 1)
DBW_HD uint32_t surface_draw_index(uint64_t seed, uint64_t step, uint32_t i, uint32_t n_cloud) {
    return step_random(seed, step, SURFACE_STREAM, i).x % n_cloud;
}

DBW_HD float surface_rho(float d2, float tau2) { return d2 < tau2 ? d2 : tau2; }

}  // namespace dbw
