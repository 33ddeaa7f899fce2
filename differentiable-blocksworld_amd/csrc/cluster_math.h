// k-means and per-cluster PCA arithmetic (host + device: tests/test_host_cluster_math.py checks the g++ build against an fp64 numpy
// restatement, tests/test_gpu_cluster.py holds the kernels of csrc/cluster_fit.hip to it).  No reference counterpart: the reference
// starts its blocks at random.  Every fp32 step is one rounding per operation (-ffp-contract=off on both builds).
//
//   distance     dist2 = ((dx*dx + dy*dy) + dz*dz) with d = p - c, fp32: the formula of dbw_nn_points (nn_math.h)
//   assignment   the k of the smallest dist2, lowest k on ties; -1 for a point with a non-finite coordinate, which enters no sum
//   moments      per point, about the CURRENT centre of its cluster, fp64: n, sum d (3), sum d d^T (xx xy xz yy yz zz).  Centring is what
//                keeps the covariance sum d d^T / n - m m^T from cancelling
//   finish       mean = c + sum d / n (fp64), the new centre that mean rounded to fp32, covariance as above
//   eigen        cyclic Jacobi, fixed sweeps, eigenvalues descending, axes as rows of a proper rotation
//   seeding      keys (bits(distance) << 32 | 0xffffffff - i): the largest key is the largest distance, lowest index on ties
#pragma once
#include "raster_math.h"      // DBW_HD

namespace dbw {

constexpr int CLUSTER_NSUM = 10;                // count, sum d (3), sum d d^T (xx xy xz yy yz zz)
constexpr int CLUSTER_JACOBI_SWEEPS = 8;
constexpr int CLUSTER_MAX_K = 256;
constexpr int CLUSTER_MAX_ITER = 64;

DBW_HD float cluster_dist2(float px, float py, float pz, float cx, float cy, float cz) {
    const float dx = px - cx, dy = py - cy, dz = pz - cz;
    return (dx * dx + dy * dy) + dz * dz;
}

DBW_HD bool cluster_finite(float x, float y, float z) { return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY; }

// centres (K, stride floats each): the label of p, *best its dist2.  A distance that is NaN (a non-finite centre) is never the smallest.
DBW_HD int cluster_assign(const float *centres, int stride, int K, float x, float y, float z, float *best) {
    if (!cluster_finite(x, y, z)) { *best = INFINITY; return -1; }
    float b = INFINITY;
    int lab = 0;
    for (int k = 0; k < K; ++k) {
        const float d = cluster_dist2(x, y, z, centres[k * stride], centres[k * stride + 1], centres[k * stride + 2]);
        if (d < b) { b = d; lab = k; }
    }
    *best = b;
    return lab;
}

// one point's terms about the centre c of its cluster, added to acc (CLUSTER_NSUM)
DBW_HD void cluster_point_moments(const float *c, float x, float y, float z, double *acc) {
    const double dx = (double)x - (double)c[0], dy = (double)y - (double)c[1], dz = (double)z - (double)c[2];
    acc[0] += 1.0;
    acc[1] += dx; acc[2] += dy; acc[3] += dz;
    acc[4] += dx * dx; acc[5] += dx * dy; acc[6] += dx * dz; acc[7] += dy * dy; acc[8] += dy * dz; acc[9] += dz * dz;
}

// From the ten sums of a cluster about its centre c: mean (3, fp64), the new centre c_new (3; c itself for an empty cluster: it keeps its
// place), cov (6; zero below two points).  -> the count
DBW_HD int cluster_finish(const double *sums, const float *c, float *c_new, double *mean, double *cov) {
    const double n = sums[0];
    for (int k = 0; k < 6; ++k) cov[k] = 0.0;
    if (!(n >= 1.0)) {
        for (int k = 0; k < 3; ++k) { mean[k] = (double)c[k]; c_new[k] = c[k]; }
        return 0;
    }
    const double mx = sums[1] / n, my = sums[2] / n, mz = sums[3] / n;
    mean[0] = (double)c[0] + mx; mean[1] = (double)c[1] + my; mean[2] = (double)c[2] + mz;
    for (int k = 0; k < 3; ++k) c_new[k] = (float)mean[k];
    if (n >= 2.0) {
        cov[0] = sums[4] / n - mx * mx; cov[1] = sums[5] / n - mx * my; cov[2] = sums[6] / n - mx * mz;
        cov[3] = sums[7] / n - my * my; cov[4] = sums[8] / n - my * mz; cov[5] = sums[9] / n - mz * mz;
    }
    return (int)n;
}

// a unit row's sign: its largest-magnitude component (lowest index on ties) is made positive
DBW_HD void sym3_fix_sign(double *v) {
    int m = 0;
    if (fabs(v[1]) > fabs(v[m])) m = 1;
    if (fabs(v[2]) > fabs(v[m])) m = 2;
    if (v[m] < 0.0) { v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2]; }
}

// Full eigen-decomposition of the symmetric C = (xx xy xz yy yz zz), fp64: the rotations of plane_math.h's sym3_smallest_eigvec (cyclic
// Jacobi, Rutishauser's formulas, CLUSTER_JACOBI_SWEEPS sweeps over (0,1), (0,2), (1,2)), all three vectors kept.  evals (3) descending (of
// equal ones the lower Jacobi column first); axes (3,3) row-major, row i the unit eigenvector of evals[i], rows 0 and 1 signed by
// sym3_fix_sign, row 2 = row 0 x row 1: a proper rotation.
DBW_HD void sym3_eigen(const double C[6], double evals[3], double axes[9]) {
    double A[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < CLUSTER_JACOBI_SWEEPS; ++sweep) {
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double apq = A[p][q];
            if (apq == 0.0) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            if (!(c == c)) continue;                            // (theta overflowed: the entry is negligible against the diagonal)
            const int r = 3 - p - q;
            const double arp = A[r][p], arq = A[r][q];
            A[p][p] -= t * apq; A[q][q] += t * apq;
            A[p][q] = A[q][p] = 0.0;
            A[r][p] = A[p][r] = c * arp - s * arq;
            A[r][q] = A[q][r] = s * arp + c * arq;
            for (int k = 0; k < 3; ++k) {
                const double vp = V[k][p], vq = V[k][q];
                V[k][p] = c * vp - s * vq;
                V[k][q] = s * vp + c * vq;
            }
        }
    }
    int o0 = 0, o1 = 1, o2 = 2, t;                              // a stable sort of three, descending
    if (A[o1][o1] > A[o0][o0]) { t = o0; o0 = o1; o1 = t; }
    if (A[o2][o2] > A[o1][o1]) { t = o1; o1 = o2; o2 = t; }
    if (A[o1][o1] > A[o0][o0]) { t = o0; o0 = o1; o1 = t; }
    evals[0] = A[o0][o0]; evals[1] = A[o1][o1]; evals[2] = A[o2][o2];
    const int order[2] = {o0, o1};
    for (int i = 0; i < 2; ++i) {
        const double x = V[0][order[i]], y = V[1][order[i]], z = V[2][order[i]];
        const double L = sqrt((x * x + y * y) + z * z);
        axes[3 * i] = x / L; axes[3 * i + 1] = y / L; axes[3 * i + 2] = z / L;
        sym3_fix_sign(axes + 3 * i);
    }
    axes[6] = axes[1] * axes[5] - axes[2] * axes[4];
    axes[7] = axes[2] * axes[3] - axes[0] * axes[5];
    axes[8] = axes[0] * axes[4] - axes[1] * axes[3];
}

// what a cluster reports beside its mean: the covariance's eigenvalues and axes; identity axes and zero eigenvalues below two points
DBW_HD void cluster_axes(int n, const double *cov, double *evals, double *axes) {
    if (n < 2) {
        for (int k = 0; k < 3; ++k) evals[k] = 0.0;
        for (int k = 0; k < 9; ++k) axes[k] = (k % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    sym3_eigen(cov, evals, axes);
}

DBW_HD uint32_t cluster_float_bits(float f) {
    union { float f; uint32_t u; } c;
    c.f = f;
    return c.u;
}

// Seeding keys of point i; a non-negative distance orders as its bits do.  The largest far key is the largest distance, the largest near
// key the smallest; the lowest index on ties in both.  Key 0 is below every point's key (i < 2^31): "no point".
DBW_HD uint64_t cluster_far_key(float mind, uint32_t i) { return ((uint64_t)cluster_float_bits(mind) << 32) | (uint64_t)(0xffffffffu - i); }
DBW_HD uint64_t cluster_near_key(float d, uint32_t i) { return ((uint64_t)(0xffffffffu - cluster_float_bits(d)) << 32) | (uint64_t)(0xffffffffu - i); }
DBW_HD uint32_t cluster_key_index(uint64_t key) { return 0xffffffffu - (uint32_t)(key & 0xffffffffull); }

}  // namespace dbw
