// Arithmetic of the free-space term (host + device: tests/test_host_freespace_math.py checks the g++ build against the fp64 restatement of
// tests/freespace_ref.py, tests/test_gpu_freespace.py holds the kernels of csrc/freespace_term.hip to the host build byte for byte).
// No reference counterpart: the reference has no geometric supervision.  The record (t, face, u, v) comes from + - * / alone, one rounding
// per operation (-ffp-contract=off on both builds; hipcc's fp32 divide is IEEE); the penalty adds one sqrt (the ray's length).
//
//   hit            of the segment o + t e, t in (0, 1), with the face (a, b, c): e1 = b - a, e2 = c - a, n = e1 x e2, h = e x e2, s = o - a,
//                  q = s x e1 (Moeller-Trumbore):  u = (s . h) / det,  v = (e . q) / det,  t = (e2 . q) / det,  det = e1 . h = -(n . e).
//                  det is formed as -(n . e): a face whose computed n is exactly zero (a repeated vertex, three collinear lattice points) then
//                  has det == 0 exactly and fails the strict graze test, which e1 . (e x e2), rounded otherwise, would not promise.
//                  A face is a candidate when det^2 > FREESPACE_GRAZE (n . n)(e . e), u >= 0, v >= 0, u + v <= 1, 0 < t < 1.  The inside tests
//                  are made on the numerators with the sign of det; only a face that passes is divided, and 0 < t < 1 is asked once more of
//                  the quotient (a numerator just below det can round to 1).
//   key            (bits(t) << 32) | face, dbw::nn_key: t > 0, so the smallest key is the first hit, the lowest face on ties
//   slab bound     does the segment t in (0, t_max) reach an axis-aligned box?  Made larger by FREESPACE_BOX_SLACK of the largest coordinate
//                  in play and by FREESPACE_T_SLACK in t, so that a face inside the box that freespace_hit accepts below t_max is never
//                  skipped
//   draw           the ray index of draw i of a step: step_random(seed, step, stream 3, i).x mod Nr
//   penalty        g = (1 - t) l - margin;  psi(g) = 0 (g <= 0), g^2 (g <= tau), tau (2 g - tau) beyond;  psi'(g) = 2 min(g, tau)
#pragma once
#include "nn_math.h"          // nn_key
#include "rng_math.h"

#pragma clang fp contract(off)

namespace dbw {

constexpr int FREESPACE_SEGMENT = 1024;          // records a backward workgroup walks by default (DBW_EVAL_FREESPACE_SEGMENT)
constexpr uint32_t FREESPACE_STREAM = 3u;        // the draw's stream of step_random (0: opacity noise, 1: overlap samples, 2: surface term)
constexpr float FREESPACE_GRAZE = 1.52587890625e-5f;         // 2^-16: sin^2 of the angle between ray and plane below which a face is no candidate
constexpr float FREESPACE_BOX_SLACK = 0.015625f;             // 2^-6 of the largest coordinate in play (DESIGN.md 6v has the derivation)
constexpr float FREESPACE_T_SLACK = 0.015625f;               // 2^-6 of the segment

struct FreespaceHit { float t, u, v; bool hit; };

DBW_HD float freespace_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// tri: the 9 coordinates a, b, c of the face; o: the origin; e = end - origin
DBW_HD FreespaceHit freespace_hit(const float *tri, float ox, float oy, float oz, float ex, float ey, float ez) {
    FreespaceHit r;
    r.t = 0.f; r.u = 0.f; r.v = 0.f; r.hit = false;
    const float e1x = tri[3] - tri[0], e1y = tri[4] - tri[1], e1z = tri[5] - tri[2];
    const float e2x = tri[6] - tri[0], e2y = tri[7] - tri[1], e2z = tri[8] - tri[2];
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const float det = -freespace_dot(nx, ny, nz, ex, ey, ez);
    const float nn = freespace_dot(nx, ny, nz, nx, ny, nz), ee = freespace_dot(ex, ey, ez, ex, ey, ez);
    if (!(det * det > FREESPACE_GRAZE * (nn * ee))) return r;
    const float hx = ey * e2z - ez * e2y, hy = ez * e2x - ex * e2z, hz = ex * e2y - ey * e2x;       // e x e2
    const float sx = ox - tri[0], sy = oy - tri[1], sz = oz - tri[2];
    const float un = freespace_dot(sx, sy, sz, hx, hy, hz);
    const float qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;       // s x e1
    const float vn = freespace_dot(ex, ey, ez, qx, qy, qz);
    const float tn = freespace_dot(e2x, e2y, e2z, qx, qy, qz);
    bool in;
    if (det > 0.f) in = un >= 0.f && vn >= 0.f && un + vn <= det && tn > 0.f && tn < det;
    else in = un <= 0.f && vn <= 0.f && un + vn >= det && tn < 0.f && tn > det;
    if (!in) return r;
    const float t = tn / det;
    if (!(t > 0.f && t < 1.f)) return r;
    r.t = t; r.u = un / det; r.v = vn / det; r.hit = true;
    return r;
}

DBW_HD uint64_t freespace_key(float t, uint32_t face) { return nn_key(t, face); }

DBW_HD float freespace_max(float a, float b) { return a > b ? a : b; }
DBW_HD float freespace_min(float a, float b) { return a < b ? a : b; }
DBW_HD float freespace_abs(float a) { return a < 0.f ? -a : a; }

// lo, hi: the box (3 each); o, e: the segment; t_max in (0, 1].  False only when no face with its vertices inside the box has a hit that
// freespace_hit accepts at a t <= t_max.
DBW_HD bool freespace_slab_reaches(const float *lo, const float *hi, const float *o, const float *e, float t_max) {
    float scale = 0.f;
    for (int k = 0; k < 3; ++k)
        scale = freespace_max(scale, freespace_max(freespace_max(freespace_abs(o[k]), freespace_abs(e[k])), freespace_max(freespace_abs(lo[k]), freespace_abs(hi[k]))));
    const float slack = FREESPACE_BOX_SLACK * scale;
    float t0 = -FREESPACE_T_SLACK, t1 = t_max + FREESPACE_T_SLACK;
    for (int k = 0; k < 3; ++k) {
        const float l = lo[k] - slack, h = hi[k] + slack;
        if (e[k] == 0.f) {
            if (o[k] < l || o[k] > h) return false;
            continue;
        }
        const float a = (l - o[k]) / e[k], b = (h - o[k]) / e[k];
        t0 = freespace_max(t0, freespace_min(a, b));
        t1 = freespace_min(t1, freespace_max(a, b));
    }
    return !(t0 > t1);
}

// the ray index of draw i (n_rays >= 1)
DBW_HD uint32_t freespace_draw_index(uint64_t seed, uint64_t step, uint32_t i, uint32_t n_rays) {
    return step_random(seed, step, FREESPACE_STREAM, i).x % n_rays;
}

DBW_HD float freespace_length(float ex, float ey, float ez) { return sqrtf(freespace_dot(ex, ey, ez, ex, ey, ez)); }

// the metric distance by which the hit lies in front of the ray's end, less the margin
DBW_HD float freespace_g(float t, float l, float margin) { return (1.f - t) * l - margin; }

DBW_HD float freespace_psi(float g, float tau) {
    if (!(g > 0.f)) return 0.f;
    return g <= tau ? g * g : tau * (2.f * g - tau);
}

}  // namespace dbw
