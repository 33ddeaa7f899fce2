// Host build (g++) of csrc/plane_math.h for tests/test_host_plane_math.py and tests/test_gpu_worldfit.py: the same inline functions the
// kernels of csrc/plane_fit.hip compile, and host_plane_fit, the stages of dbw_eval_plane_fit written as plain loops over them (HOST
// pointers, same arguments and outputs).  With -DPLANE_MATH_MAIN the file is a program of its own, for a run under the sanitizers.
#include <stdio.h>

#include <vector>

#include "../differentiable-blocksworld_amd/csrc/plane_math.h"

using namespace dbw;

extern "C" {

int host_plane_draw(uint64_t seed, uint32_t j, int64_t N, int32_t *idx) {
    plane_draw(seed, j, N, idx);
    return 0;
}

// -> 1 and out (4), or 0 for a degenerate triple
int host_plane_from_triple(const float *a, const float *b, const float *c, int mode, const float *up, float *out) {
    return plane_from_triple(a, b, c, mode, up, out) ? 1 : 0;
}

int host_plane_residuals(const float *pl, const float *points, int64_t n, float *r) {
    for (int64_t i = 0; i < n; ++i) r[i] = plane_residual(pl, points[i * 3], points[i * 3 + 1], points[i * 3 + 2]);
    return 0;
}

int64_t host_plane_count(const float *pl, const float *points, int64_t n, float thresh2) {
    int64_t c = 0;
    for (int64_t i = 0; i < n; ++i) c += plane_inlier(pl, points[i * 3], points[i * 3 + 1], points[i * 3 + 2], thresh2) ? 1 : 0;
    return c;
}

int host_plane_admissible(const float *pl, const float *up, float cos_tilt, const float *cams, int M, float tau, int min_cams) {
    return plane_admissible(pl, up, cos_tilt, cams, M, tau, min_cams) ? 1 : 0;
}

int host_sym3_smallest_eigvec(const double *C, int64_t n, double *v) {
    for (int64_t i = 0; i < n; ++i) sym3_smallest_eigvec(C + i * 6, v + i * 3);
    return 0;
}

int host_plane_fit(const float *points, int64_t N, int H, int mode, float thresh2, uint64_t seed, const int32_t *triples, const float *up,
                   float cos_tilt, const float *cams, int M, float tau, int min_cams, int refine, double *plane, int32_t *info, int32_t *counts,
                   int32_t *triples_out, uint8_t *mask) {
    if (!(H >= 1 && H <= 4096 && N >= 3 && N < (1ll << 31) && refine >= 0 && refine <= 8)) return -1;
    int best = -1, best_count = -1;
    std::vector<float> hyp((size_t)H * 4);
    for (int j = 0; j < H; ++j) {
        int32_t idx[3];
        if (triples) { idx[0] = triples[3 * j]; idx[1] = triples[3 * j + 1]; idx[2] = triples[3 * j + 2]; }
        else plane_draw(seed, (uint32_t)j, N, idx);
        if (triples_out) { triples_out[3 * j] = idx[0]; triples_out[3 * j + 1] = idx[1]; triples_out[3 * j + 2] = idx[2]; }
        float *pl = &hyp[(size_t)j * 4];
        bool good = idx[0] >= 0 && idx[0] < N && idx[1] >= 0 && idx[1] < N && idx[2] >= 0 && idx[2] < N;
        if (good) good = plane_from_triple(points + (int64_t)idx[0] * 3, points + (int64_t)idx[1] * 3, points + (int64_t)idx[2] * 3, mode, up, pl);
        if (good && mode == PLANE_ORTHOGONAL) good = plane_admissible(pl, up, cos_tilt, cams, cams ? M : 0, tau, min_cams);
        int32_t c = -1;
        if (good) c = (int32_t)host_plane_count(pl, points, N, thresh2);
        if (counts) counts[j] = c;
        if (c > best_count) { best_count = c; best = j; }
    }
    info[0] = best; info[1] = best < 0 ? 0 : best_count; info[2] = 0; info[3] = 0;
    plane[0] = plane[1] = plane[2] = plane[3] = 0.0;
    if (best < 0) {
        if (mask) for (int64_t i = 0; i < N; ++i) mask[i] = 0;
        return 0;
    }
    for (int k = 0; k < 4; ++k) plane[k] = (double)hyp[(size_t)best * 4 + k];
    int32_t idx[3];
    if (triples) idx[0] = triples[3 * best];
    else plane_draw(seed, (uint32_t)best, N, idx);
    const float a0[3] = {points[(int64_t)idx[0] * 3], points[(int64_t)idx[0] * 3 + 1], points[(int64_t)idx[0] * 3 + 2]};
    if (mode == PLANE_ORTHOGONAL) {
        for (int r = 0; r < refine; ++r) {
            const float pl[4] = {(float)plane[0], (float)plane[1], (float)plane[2], (float)plane[3]};
            double sums[PLANE_NSUM] = {0.0};
            for (int64_t i = 0; i < N; ++i) plane_point_moments(pl, a0, points[i * 3], points[i * 3 + 1], points[i * 3 + 2], thresh2, sums);
            if (!plane_refine_step(sums, a0, plane)) break;
            info[3] = r + 1;
        }
    }
    const float pl[4] = {(float)plane[0], (float)plane[1], (float)plane[2], (float)plane[3]};
    int64_t c = 0;
    for (int64_t i = 0; i < N; ++i) {
        const bool in = plane_inlier(pl, points[i * 3], points[i * 3 + 1], points[i * 3 + 2], thresh2);
        if (mask) mask[i] = in ? 1 : 0;
        c += in ? 1 : 0;
    }
    info[2] = (int32_t)c;
    return 0;
}

}

#ifdef PLANE_MATH_MAIN
// A small fit on exactly sized heap buffers: a read or write outside them is the sanitizer's to report.
int main() {
    const int64_t N = 301;
    const int H = 37, M = 5;
    std::vector<float> p((size_t)N * 3), cams((size_t)M * 3);
    uint32_t s = 12345u;
    auto u = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.f - 0.5f; };
    for (int64_t i = 0; i < N; ++i) {
        p[i * 3] = u(); p[i * 3 + 1] = u();
        p[i * 3 + 2] = i % 3 ? 0.1f * p[i * 3] + 0.01f * u() : u();
    }
    for (int k = 0; k < M; ++k) { cams[k * 3] = u(); cams[k * 3 + 1] = u(); cams[k * 3 + 2] = 1.f + u(); }
    const float up[3] = {0.f, 0.f, 1.f};
    std::vector<int32_t> counts(H), tri((size_t)H * 3);
    std::vector<uint8_t> mask(N);
    double plane[4];
    int32_t info[4];
    int rc = host_plane_fit(p.data(), N, H, PLANE_ORTHOGONAL, 0.02f * 0.02f, 7, nullptr, up, 0.5f, cams.data(), M, 0.02f, 4, 2, plane, info,
                            counts.data(), tri.data(), mask.data());
    printf("rc %d best %d count %d final %d rounds %d n = %g %g %g d = %g\n", rc, info[0], info[1], info[2], info[3], plane[0], plane[1], plane[2], plane[3]);
    if (rc || info[0] < 0 || info[2] < 150) return 1;
    rc = host_plane_fit(p.data(), N, H, PLANE_VERTICAL, 0.001f, 7, tri.data(), nullptr, 0.f, nullptr, 0, 0.f, 0, 0, plane, info, counts.data(), nullptr,
                        mask.data());
    printf("rc %d best %d count %d final %d\n", rc, info[0], info[1], info[2]);
    return rc || info[0] < 0 || info[1] != info[2] ? 1 : 0;
}
#endif
