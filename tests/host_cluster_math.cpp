// Host build (g++) of csrc/cluster_math.h for tests/test_host_cluster_math.py, tests/test_cluster_host.py and tests/test_gpu_cluster.py: the
// same inline functions the kernels of csrc/cluster_fit.hip compile, and host_cluster_fit, the stages of dbw_eval_cluster_fit written as plain
// loops over them (HOST pointers, same arguments and outputs; sums (K,10) beside them).  With -DCLUSTER_MATH_MAIN the file is a
// program of its own, for a run under the sanitizers.
#include <stdio.h>

#include <vector>

#include "../differentiable-blocksworld_amd/csrc/cluster_math.h"

using namespace dbw;

extern "C" {

int host_cluster_assign(const float *points, int64_t N, const float *centres, int K, int32_t *labels, float *dist2) {
    for (int64_t i = 0; i < N; ++i) {
        float b;
        labels[i] = cluster_assign(centres, 3, K, points[i * 3], points[i * 3 + 1], points[i * 3 + 2], &b);
        if (dist2) dist2[i] = b;
    }
    return 0;
}

// sums (K,10): the moments of every cluster about its centre.  The points of a cluster are added in index order in chunks of HOST_CHUNK, as the
// 64 lanes of a wave are on the device, and the chunks' sums in order.  One running sum over all the points would not do: the terms are
// multiples of one power of two (differences of fp32 numbers and their products), so while the running sum's ulp is twice that quantum every
// other addition is an exact tie, and a tie that follows a tie rounds down (half to even, the sum is even already) -- a drift of about n / 8
// ulp, always downwards, more than any reordering bound once a cluster has a hundred points.
constexpr int HOST_CHUNK = 64;
int host_cluster_moments(const float *points, int64_t N, const float *centres, int K, const int32_t *labels, double *sums) {
    std::vector<double> part((size_t)K * CLUSTER_NSUM, 0.0);
    std::vector<int> held((size_t)K, 0);
    for (int k = 0; k < K * CLUSTER_NSUM; ++k) sums[k] = 0.0;
    auto flush = [&](int k) {
        for (int s = 0; s < CLUSTER_NSUM; ++s) { sums[k * CLUSTER_NSUM + s] += part[(size_t)k * CLUSTER_NSUM + s]; part[(size_t)k * CLUSTER_NSUM + s] = 0.0; }
        held[k] = 0;
    };
    for (int64_t i = 0; i < N; ++i) {
        const int k = labels[i];
        if (k < 0 || k >= K) continue;
        cluster_point_moments(centres + 3 * k, points[i * 3], points[i * 3 + 1], points[i * 3 + 2], &part[(size_t)k * CLUSTER_NSUM]);
        if (++held[k] == HOST_CHUNK) flush(k);
    }
    for (int k = 0; k < K; ++k) if (held[k]) flush(k);
    return 0;
}

int host_cluster_finish(const double *sums, const float *c, float *c_new, double *mean, double *cov) { return cluster_finish(sums, c, c_new, mean, cov); }

int host_sym3_eigen(const double *C, int64_t n, double *evals, double *axes) {
    for (int64_t i = 0; i < n; ++i) sym3_eigen(C + i * 6, evals + i * 3, axes + i * 9);
    return 0;
}

int host_cluster_keys(const float *d, int64_t n, uint64_t *far_keys, uint64_t *near_keys) {
    for (int64_t i = 0; i < n; ++i) { far_keys[i] = cluster_far_key(d[i], (uint32_t)i); near_keys[i] = cluster_near_key(d[i], (uint32_t)i); }
    return 0;
}

// farthest-point seeding -> centres (K,3), order (K) int64: the index of the point each centre is (-1: no finite point)
int host_cluster_seed(const float *points, int64_t N, int K, float *centres, int64_t *order) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = 0; i < N; ++i) {
        const float x = points[i * 3], y = points[i * 3 + 1], z = points[i * 3 + 2];
        if (cluster_finite(x, y, z)) { s[0] += 1.0; s[1] += (double)x; s[2] += (double)y; s[3] += (double)z; }
    }
    float c[3] = {0.f, 0.f, 0.f};
    if (s[0] >= 1.0) { c[0] = (float)(s[1] / s[0]); c[1] = (float)(s[2] / s[0]); c[2] = (float)(s[3] / s[0]); }
    std::vector<float> mind((size_t)N);
    for (int j = 0; j < K; ++j) {
        uint64_t best = 0;
        for (int64_t i = 0; i < N; ++i) {
            const float x = points[i * 3], y = points[i * 3 + 1], z = points[i * 3 + 2];
            if (!cluster_finite(x, y, z)) continue;
            const float d = cluster_dist2(x, y, z, c[0], c[1], c[2]);
            uint64_t key;
            if (j == 0) {
                key = cluster_near_key(d, (uint32_t)i);
            } else {
                float m = d;
                if (j > 1) m = d < mind[i] ? d : mind[i];
                mind[i] = m;
                key = cluster_far_key(m, (uint32_t)i);
            }
            if (key > best) best = key;
        }
        c[0] = c[1] = c[2] = 0.f;
        order[j] = -1;
        if (best != 0) {
            const int64_t w = (int64_t)cluster_key_index(best);
            order[j] = w;
            c[0] = points[w * 3]; c[1] = points[w * 3 + 1]; c[2] = points[w * 3 + 2];
        }
        centres[3 * j] = c[0]; centres[3 * j + 1] = c[1]; centres[3 * j + 2] = c[2];
    }
    return 0;
}

int host_cluster_fit(const float *points, int64_t N, int K, const float *init, int n_iter, float *centres, int32_t *labels, int32_t *counts,
                     double *mean, double *cov, double *evals, double *axes, int32_t *info, double *sums) {
    if (!(K >= 1 && K <= CLUSTER_MAX_K && N >= K && N < (1ll << 31) && n_iter >= 0 && n_iter <= CLUSTER_MAX_ITER)) return -1;
    std::vector<float> cen((size_t)K * 3);
    std::vector<int64_t> order((size_t)K);
    if (init) for (int k = 0; k < K * 3; ++k) cen[k] = init[k];
    else host_cluster_seed(points, N, K, cen.data(), order.data());
    std::vector<int32_t> lab((size_t)N), prev((size_t)N);
    std::vector<double> S((size_t)K * CLUSTER_NSUM);
    int32_t changed = 0;
    for (int r = 0; r <= n_iter; ++r) {
        prev = lab;
        host_cluster_assign(points, N, cen.data(), K, lab.data(), nullptr);
        changed = 0;
        for (int64_t i = 0; i < N; ++i) changed += (r == 0 || prev[i] != lab[i]) ? 1 : 0;
        host_cluster_moments(points, N, cen.data(), K, lab.data(), S.data());
        if (r == n_iter) break;
        for (int k = 0; k < K; ++k) {
            float c_new[3];
            double m[3], c6[6];
            cluster_finish(&S[(size_t)k * CLUSTER_NSUM], &cen[3 * k], c_new, m, c6);
            cen[3 * k] = c_new[0]; cen[3 * k + 1] = c_new[1]; cen[3 * k + 2] = c_new[2];
        }
    }
    int nonempty = 0;
    for (int k = 0; k < K; ++k) {
        float c_new[3];
        double m[3], c6[6], ev[3], ax[9];
        const int n = cluster_finish(&S[(size_t)k * CLUSTER_NSUM], &cen[3 * k], c_new, m, c6);
        cluster_axes(n, c6, ev, ax);
        counts[k] = n;
        nonempty += n > 0 ? 1 : 0;
        for (int i = 0; i < 3; ++i) centres[3 * k + i] = cen[3 * k + i];
        if (mean) for (int i = 0; i < 3; ++i) mean[3 * k + i] = m[i];
        if (cov) for (int i = 0; i < 6; ++i) cov[6 * k + i] = c6[i];
        if (evals) for (int i = 0; i < 3; ++i) evals[3 * k + i] = ev[i];
        if (axes) for (int i = 0; i < 9; ++i) axes[9 * k + i] = ax[i];
    }
    if (labels) for (int64_t i = 0; i < N; ++i) labels[i] = lab[i];
    if (sums) for (int k = 0; k < K * CLUSTER_NSUM; ++k) sums[k] = S[k];
    info[0] = n_iter; info[1] = changed; info[2] = nonempty; info[3] = 0;
    return 0;
}

}

#ifdef CLUSTER_MATH_MAIN
// A small fit on exactly sized heap buffers: a read or write outside them is the sanitizer's to report.
int main() {
    const int64_t N = 301;
    const int K = 7;
    std::vector<float> p((size_t)N * 3);
    uint32_t s = 12345u;
    auto u = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.f - 0.5f; };
    for (int64_t i = 0; i < N; ++i) for (int k = 0; k < 3; ++k) p[i * 3 + k] = (float)(i % 3) * 2.f + 0.3f * u();
    p[5 * 3 + 1] = NAN;
    std::vector<float> centres((size_t)K * 3);
    std::vector<int32_t> labels(N), counts(K);
    std::vector<double> mean((size_t)K * 3), cov((size_t)K * 6), evals((size_t)K * 3), axes((size_t)K * 9), sums((size_t)K * CLUSTER_NSUM);
    int32_t info[4];
    const int rc = host_cluster_fit(p.data(), N, K, nullptr, 5, centres.data(), labels.data(), counts.data(), mean.data(), cov.data(), evals.data(),
                                    axes.data(), info, sums.data());
    int total = 0;
    for (int k = 0; k < K; ++k) total += counts[k];
    printf("rc %d rounds %d changed %d nonempty %d total %d label[5] %d\n", rc, info[0], info[1], info[2], total, labels[5]);
    return rc || total != N - 1 || labels[5] != -1 || info[2] < 3 ? 1 : 0;
}
#endif
