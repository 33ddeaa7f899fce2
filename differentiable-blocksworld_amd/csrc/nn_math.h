// Arithmetic of the 3D evaluation (nearest neighbours, the DTU dense lattice, the radius test of the downsample), written once for the
// device (hipcc, nn_search.hip) and for the host (g++, tests/test_eval3d_host.py builds tests/host_nn_math.cpp and compares it with numpy
// and torch without a GPU).  Both sides are built with -ffp-contract=off: one rounding per operation, in the order written here.
//
//  * nn_dist2: the squared distance of the nearest-neighbour search, ((dx*dx + dy*dy) + dz*dz) with d = x - y, fp32.
//  * lattice_*: the dense triangle sampling of the DTU protocol (reference utils/dtu_eval.py:21-30,56-78), in fp64 and in numpy's order
//    of operations: np.linalg.norm is sqrt((x*x + y*y) + z*z), np.cross is a1*b2 - a2*b1 (two rounded products), the lattice point is
//    (v1*k0 + v2*k1) + v0.  On a face with n1 == n2 the anti-diagonal of the lattice is a tie of `k0 + k1 < 1` in real arithmetic, so
//    only the same fp64 roundings give the same point count.
#pragma once
#include <math.h>
#include <stdint.h>

#include "raster_math.h"      // DBW_HD

#pragma clang fp contract(off)

namespace dbw {

// (T = float, or a 2-vector of float: the kernel evaluates two queries per packed instruction, with the same IEEE result per lane)
template <typename T>
DBW_HD T nn_dist2(T x0, T x1, T x2, T y0, T y1, T y2) {
    const T d0 = x0 - y0, d1 = x1 - y1, d2 = x2 - y2;
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

// 64-bit merge key of a (dist2, index) candidate: dist2 >= 0, so its bits order like the value, and the smaller index wins a tie
DBW_HD uint64_t nn_key(float d2, uint32_t idx) {
    union { float f; uint32_t u; } c;
    c.f = d2;
    return ((uint64_t)c.u << 32) | idx;
}

#define DBW_DTU_DENSITY 0.2       // DOWNSAMPLE_DENSITY of dtu_eval.py:17: lattice density and downsample radius

// one triangle's lattice sizes (dtu_eval.py:56-70): false when the face is dropped (area2 == 0).  t = the 9 coordinates v0, v1, v2.
DBW_HD bool lattice_setup(const double *t, double v1[3], double v2[3], double &n1, double &n2) {
    for (int c = 0; c < 3; ++c) { v1[c] = t[3 + c] - t[c]; v2[c] = t[6 + c] - t[c]; }
    const double l1 = sqrt((v1[0] * v1[0] + v1[1] * v1[1]) + v1[2] * v1[2]);
    const double l2 = sqrt((v2[0] * v2[0] + v2[1] * v2[1]) + v2[2] * v2[2]);
    const double c0 = v1[1] * v2[2] - v1[2] * v2[1];
    const double c1 = v1[2] * v2[0] - v1[0] * v2[2];
    const double c2 = v1[0] * v2[1] - v1[1] * v2[0];
    const double area2 = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
    if (!(area2 > 0.0)) return false;
    const double thr = DBW_DTU_DENSITY * sqrt(l1 * l2 / area2);
    n1 = floor(l1 / thr);
    n2 = floor(l2 / thr);
    return true;
}

// k of lattice index i along a side of n steps: (i + 0.5) / max(n, 1e-7)  (np.mgrid + 0.5, then the in-place division)
DBW_HD double lattice_k(long long i, double n) { return ((double)i + 0.5) / (n > 1e-7 ? n : 1e-7); }

// number of j in [0, n2] with k(i, n1) + k(j, n2) < 1 (`c.sum(axis=-1) < 1`): the test is monotone in j, so start from the real-arithmetic
// estimate and step to the first failing j with the exact fp64 test
DBW_HD long long lattice_row_count(long long i, double n1, double n2) {
    const double k0 = lattice_k(i, n1);
    const long long jmax = (long long)n2;
    if (!(k0 + lattice_k(0, n2) < 1.0)) return 0;
    double e = (1.0 - k0) * n2 - 0.5;
    long long j = e < 0.0 ? 0 : (e > (double)jmax ? jmax : (long long)e);
    while (j > 0 && !(k0 + lattice_k(j, n2) < 1.0)) --j;                 // now j passes (j == 0 passes, checked above)
    while (j < jmax && k0 + lattice_k(j + 1, n2) < 1.0) ++j;
    return j + 1;
}

// the lattice point count of one triangle (0 for a dropped face)
DBW_HD long long lattice_count(const double *t) {
    double v1[3], v2[3], n1, n2;
    if (!lattice_setup(t, v1, v2, n1, n2)) return 0;
    long long cnt = 0;
    for (long long i = 0; i <= (long long)n1; ++i) cnt += lattice_row_count(i, n1, n2);
    return cnt;
}

// the lattice points of one triangle in np.mgrid row-major order (i major, j minor), (v1*k0 + v2*k1) + v0 per coordinate, at most `cap`
// of them; returns the number written
DBW_HD long long lattice_emit(const double *t, double *out, long long cap) {
    double v1[3], v2[3], n1, n2;
    if (!lattice_setup(t, v1, v2, n1, n2)) return 0;
    long long m = 0;
    for (long long i = 0; i <= (long long)n1; ++i) {
        const double k0 = lattice_k(i, n1);
        const long long cnt = lattice_row_count(i, n1, n2);
        for (long long j = 0; j < cnt && m < cap; ++j, ++m) {
            const double k1 = lattice_k(j, n2);
            for (int c = 0; c < 3; ++c) out[m * 3 + c] = (v1[c] * k0 + v2[c] * k1) + t[c];
        }
    }
    return m;
}

// the radius test of the downsample (dtu_eval.py:82-96, sklearn radius_neighbors: distance <= radius), fp64
DBW_HD bool within_radius(const double *a, const double *b, double r2) {
    const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
    return (d0 * d0 + d1 * d1) + d2 * d2 <= r2;
}

}  // namespace dbw
