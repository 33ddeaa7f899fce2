// Plane RANSAC arithmetic (host + device: tests/test_host_plane_math.py checks the g++ build against fp64 numpy and the reference's own
// counts, tests/test_gpu_worldfit.py holds the kernels of csrc/plane_fit.hip to it bit for bit).  Reference: src/utils/ransac.py, the
// ground filter of src/dtu_3d_process.py:36-41.  Every fp32 step is one rounding per operation (-ffp-contract=off on both builds).
//
// A plane is four floats (n.x, n.y, n.z, d); the residual of a point is ((n.x*p.x + n.y*p.y) + n.z*p.z) - d.
//   PLANE_ORTHOGONAL   n is the unit normal of the triple's triangle, the residual a distance; the inlier test is r*r < tau^2
//   PLANE_VERTICAL     the reference's regression z = p0 + p1 x + p2 y through the triple written as a plane: n = m / m.z (so n.z == 1),
//                      p = (d, -n.x, -n.y); the residual is the reference's y - predict(X) and r*r < thresh is its test (ransac.py:48-49)
#pragma once
#include "rng_math.h"

namespace dbw {

enum { PLANE_ORTHOGONAL = 0, PLANE_VERTICAL = 1 };
constexpr int PLANE_NSUM = 10;              // count, sum q (3), sum q q^T (xx xy xz yy yz zz)
constexpr int PLANE_JACOBI_SWEEPS = 8;
constexpr uint32_t PLANE_STREAM = 0x504C414Eu;      // 'PLAN': the Philox counter word that keeps these draws apart from the training step's

// the triple of hypothesis j among N points: three words of one Philox block, each scaled to [0, N) by the high half of word * N
DBW_HD void plane_draw(uint64_t seed, uint32_t j, int64_t N, int32_t idx[3]) {
    const Philox4 r = philox4x32_10(j, 0u, 0u, PLANE_STREAM, (uint32_t)seed, (uint32_t)(seed >> 32));
    idx[0] = (int32_t)(((uint64_t)r.x * (uint64_t)N) >> 32);
    idx[1] = (int32_t)(((uint64_t)r.y * (uint64_t)N) >> 32);
    idx[2] = (int32_t)(((uint64_t)r.z * (uint64_t)N) >> 32);
}

DBW_HD float plane_dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

DBW_HD float plane_residual(const float *pl, float x, float y, float z) { return plane_dot3(pl[0], pl[1], pl[2], x, y, z) - pl[3]; }

DBW_HD bool plane_inlier(const float *pl, float x, float y, float z, float thresh2) {
    const float r = plane_residual(pl, x, y, z);
    return r * r < thresh2;
}

// the plane through a, b, c -> out (n, d); false for a degenerate triple (out is then (0, 0, 0, 0)).  up (3) or NULL: the side n points to
DBW_HD bool plane_from_triple(const float *a, const float *b, const float *c, int mode, const float *up, float out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0.f;
    const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
    const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    const float mx = e1y * e2z - e1z * e2y, my = e1z * e2x - e1x * e2z, mz = e1x * e2y - e1y * e2x;
    const float L2 = plane_dot3(mx, my, mz, mx, my, mz);
    const float l1 = plane_dot3(e1x, e1y, e1z, e1x, e1y, e1z), l2 = plane_dot3(e2x, e2y, e2z, e2x, e2y, e2z);
    if (!(L2 < INFINITY) || L2 <= 1e-8f * (l1 * l2)) return false;           // (!(x < inf): NaN and inf alike)
    float nx, ny, nz;
    if (mode == PLANE_VERTICAL) {
        if (mz == 0.f) return false;
        nx = mx / mz; ny = my / mz; nz = mz / mz;
    } else {
        const float L = sqrtf(L2);
        nx = mx / L; ny = my / L; nz = mz / L;
        if (up && plane_dot3(nx, ny, nz, up[0], up[1], up[2]) < 0.f) { nx = -nx; ny = -ny; nz = -nz; }
    }
    out[0] = nx; out[1] = ny; out[2] = nz;
    out[3] = plane_dot3(nx, ny, nz, a[0], a[1], a[2]);
    return true;
}

// the priors of the world-frame fit on a PLANE_ORTHOGONAL hypothesis: its tilt against `up` (3 or NULL) is at most acos(cos_tilt), and at
// least min_cams of the M camera centres `cams` ((M,3) or NULL) lie more than tau above it
DBW_HD bool plane_admissible(const float *pl, const float *up, float cos_tilt, const float *cams, int M, float tau, int min_cams) {
    if (up && !(plane_dot3(pl[0], pl[1], pl[2], up[0], up[1], up[2]) >= cos_tilt)) return false;
    if (cams) {
        int above = 0;
        for (int k = 0; k < M; ++k) above += plane_residual(pl, cams[3 * k], cams[3 * k + 1], cams[3 * k + 2]) > tau ? 1 : 0;
        if (above < min_cams) return false;
    }
    return true;
}

// refinement: one point's terms, q = p - a0 in fp64, added to acc (PLANE_NSUM) if the point is an inlier of the fp32 plane
DBW_HD void plane_point_moments(const float *pl, const float *a0, float x, float y, float z, float thresh2, double *acc) {
    if (!plane_inlier(pl, x, y, z, thresh2)) return;
    const double qx = (double)x - (double)a0[0], qy = (double)y - (double)a0[1], qz = (double)z - (double)a0[2];
    acc[0] += 1.0;
    acc[1] += qx; acc[2] += qy; acc[3] += qz;
    acc[4] += qx * qx; acc[5] += qx * qy; acc[6] += qx * qz; acc[7] += qy * qy; acc[8] += qy * qz; acc[9] += qz * qz;
}

// Eigenvector of the smallest eigenvalue of the symmetric C = (xx xy xz yy yz zz), fp64: cyclic Jacobi (Rutishauser's rotations), a fixed
// PLANE_JACOBI_SWEEPS sweeps over (0,1), (0,2), (1,2).  The off-diagonal norm falls quadratically once it is small: 8 sweeps leave it at
// rounding level for any 3x3 input.  v is a unit vector; its sign is the caller's to fix.
DBW_HD void sym3_smallest_eigvec(const double C[6], double v[3]) {
    double A[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < PLANE_JACOBI_SWEEPS; ++sweep) {
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
    int m = 0;
    if (A[1][1] < A[m][m]) m = 1;
    if (A[2][2] < A[m][m]) m = 2;
    const double x = V[0][m], y = V[1][m], z = V[2][m];
    const double L = sqrt((x * x + y * y) + z * z);
    v[0] = x / L; v[1] = y / L; v[2] = z / L;
}

// One refinement round from the sums of plane_point_moments over all points: the covariance of the inliers about their mean, its smallest
// eigenvector signed to agree with the previous normal, d = n . (a0 + mean).  plane (4, fp64) is updated; false (plane untouched) below
// 3 inliers.
DBW_HD bool plane_refine_step(const double *sums, const float *a0, double *plane) {
    const double cnt = sums[0];
    if (cnt < 3.0) return false;
    const double mx = sums[1] / cnt, my = sums[2] / cnt, mz = sums[3] / cnt;
    const double C[6] = {sums[4] / cnt - mx * mx, sums[5] / cnt - mx * my, sums[6] / cnt - mx * mz,
                         sums[7] / cnt - my * my, sums[8] / cnt - my * mz, sums[9] / cnt - mz * mz};
    double v[3];
    sym3_smallest_eigvec(C, v);
    if ((v[0] * plane[0] + v[1] * plane[1]) + v[2] * plane[2] < 0.0) { v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2]; }
    plane[0] = v[0]; plane[1] = v[1]; plane[2] = v[2];
    plane[3] = (v[0] * ((double)a0[0] + mx) + v[1] * ((double)a0[1] + my)) + v[2] * ((double)a0[2] + mz);
    return true;
}

}  // namespace dbw
