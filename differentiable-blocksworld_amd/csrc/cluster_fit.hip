// k-means with per-cluster PCA behind one call (include/dbw_eval.h: dbw_eval_cluster_fit).  The arithmetic is csrc/cluster_math.h (also
// built by g++ for the host tests); this file is the schedule.
//
// Launches, all on one stream, kernel boundaries the only ordering, nothing read by the host:
//   cluster_begin_kernel     one workgroup: the state and the seeding keys cleared, info zeroed, `init` copied to the working centres
//   seeding (init == NULL)   cluster_mean_kernel (fp64 partial sums of the finite points), then cluster_seed_kernel once per round j = 0 .. K:
//                            round j reads the winner of round j - 1 (round 0: the mean) on the device, writes it as centre j - 1, updates
//                            mind (N floats in the workspace) and merges the round's winner with a 64-bit integer atomic max on its key
//   n_iter x (cluster_assign_kernel, cluster_update_kernel)      one Lloyd round: labels and moments in ONE pass over the points, new centres
//   cluster_assign_kernel, cluster_update_kernel (final)         the same pass against the final centres: every output comes from it
//
// Assignment.  A workgroup of 256 lanes takes tiles of 256 * CLUSTER_PTS points, CLUSTER_PTS points per lane in registers, and walks ALL
// centres per tile: a point is read once per round, whatever K.  The centre index is wave-uniform, so its floats arrive by scalar loads.
//
// Sums.  No floating-point atomics.  After the labels of a tile are known a wave walks the clusters present among its lanes (ballot, first
// pending lane's label, readfirstlane): a lane adds its own points of that cluster in index order in fp64, the lanes are added by a shuffle
// tree, and lane 0 adds the result to the wave's OWN table in LDS (K x 10 doubles per wave), which no other wave touches.  At the end of the
// workgroup the four tables are added in wave order into the workgroup's row of partials, and cluster_update_kernel adds the rows in
// workgroup order, one lane per sum.  The grid depends on N alone: the same call gives the same bytes every time.  The count of labels that
// changed is an integer and uses an integer atomic.
#include "dbw_common.h"
#include "cluster_math.h"
#include "../../include/dbw_eval.h"

#include <math.h>

namespace {

constexpr int CL_BLOCK = 256;
constexpr int CL_WAVES = CL_BLOCK / DBW_WAVE;
constexpr int CL_PTS = 4;                       // points a lane keeps in registers
constexpr int CL_TILE = CL_BLOCK * CL_PTS;
constexpr int CL_MAX_GROUPS = 512;              // workgroups of the assignment kernel, at most: one row of partials each
constexpr int CL_MEAN_PARTS = 128;              // workgroups of the mean kernel, at most
constexpr int CL_SEED_GROUPS = 1024;            // workgroups of a seeding round, at most
constexpr int NSUM = dbw::CLUSTER_NSUM;

struct ClusterState {
    int32_t rounds, changed;
    int32_t pad[2];
};
static_assert(sizeof(ClusterState) % 16 == 0, "the state keeps what follows it 16-byte aligned");

struct ClusterLayout {          // byte offsets into the workspace
    size_t state, cen, keys, mean_parts, partials, mind, lab, total;
    int groups, mean_parts_n, seed_groups;
};

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

inline bool cluster_sizes_ok(int64_t N, int K) { return K >= 1 && K <= dbw::CLUSTER_MAX_K && N >= K && N < (1ll << 31); }

inline ClusterLayout cluster_layout(int64_t N, int K) {
    ClusterLayout L;
    const int64_t tiles = (N + CL_TILE - 1) / CL_TILE, blocks = (N + CL_BLOCK - 1) / CL_BLOCK;
    L.groups = (int)(tiles < CL_MAX_GROUPS ? tiles : CL_MAX_GROUPS);
    L.mean_parts_n = (int)(blocks < CL_MEAN_PARTS ? blocks : CL_MEAN_PARTS);
    L.seed_groups = (int)(blocks < CL_SEED_GROUPS ? blocks : CL_SEED_GROUPS);
    size_t o = 0;
    L.state = o; o = align16(o + sizeof(ClusterState));
    L.cen = o; o = align16(o + (size_t)K * 4 * sizeof(float));
    L.keys = o; o = align16(o + (size_t)K * sizeof(unsigned long long));
    L.mean_parts = o; o = align16(o + (size_t)CL_MEAN_PARTS * 4 * sizeof(double));
    L.partials = o; o = align16(o + (size_t)L.groups * K * NSUM * sizeof(double));
    L.mind = o; o = align16(o + (size_t)N * sizeof(float));
    L.lab = o; o = align16(o + (size_t)N * sizeof(int32_t));
    L.total = o;
    return L;
}

__global__ __launch_bounds__(CL_BLOCK) void cluster_begin_kernel(const float *__restrict__ init, int K, ClusterState *__restrict__ state,
                                                                 float4 *__restrict__ cen, unsigned long long *__restrict__ keys,
                                                                 int32_t *__restrict__ info) {
    const int t = threadIdx.x;
    if (t < K) {
        keys[t] = 0ull;
        cen[t] = init ? make_float4(init[3 * t], init[3 * t + 1], init[3 * t + 2], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (t < 4) info[t] = 0;
    if (t == 0) { state->rounds = 0; state->changed = 0; state->pad[0] = state->pad[1] = 0; }
}

// count and coordinate sums of the finite points, fp64, in the fixed order of the header comment -> parts (gridDim.x, 4)
__global__ __launch_bounds__(CL_BLOCK) void cluster_mean_kernel(const float *__restrict__ points, long long N, double *__restrict__ parts) {
    __shared__ double sh[CL_WAVES][4];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long i = (long long)blockIdx.x * CL_BLOCK + threadIdx.x; i < N; i += (long long)gridDim.x * CL_BLOCK) {
        const float x = points[i * 3], y = points[i * 3 + 1], z = points[i * 3 + 2];
        if (dbw::cluster_finite(x, y, z)) { acc[0] += 1.0; acc[1] += (double)x; acc[2] += (double)y; acc[3] += (double)z; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        acc[k] = v;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sh[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double v = sh[0][threadIdx.x];
        for (int w = 1; w < CL_WAVES; ++w) v += sh[w][threadIdx.x];
        parts[(long long)blockIdx.x * 4 + threadIdx.x] = v;
    }
}

// Seeding round j of K (launched for j = 0 .. K; j == K with one workgroup, which only writes centre K - 1).
__global__ __launch_bounds__(CL_BLOCK) void cluster_seed_kernel(const float *__restrict__ points, long long N, int j, int K,
                                                                const double *__restrict__ mean_parts, int n_parts,
                                                                unsigned long long *__restrict__ keys, float4 *__restrict__ cen,
                                                                float *__restrict__ mind) {
    __shared__ unsigned long long sh_key[CL_WAVES];
    float cx = 0.f, cy = 0.f, cz = 0.f;
    if (j == 0) {                                               // the fp32-rounded mean of the finite points (zero without any)
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int b = 0; b < n_parts; ++b) {
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] += mean_parts[b * 4 + k];
        }
        if (s[0] >= 1.0) { cx = (float)(s[1] / s[0]); cy = (float)(s[2] / s[0]); cz = (float)(s[3] / s[0]); }
    } else {                                                    // the winner of the round before (key 0: no finite point, the centre is zero)
        const unsigned long long key = keys[j - 1];
        if (key != 0ull) {
            const long long w = (long long)dbw::cluster_key_index(key);
            cx = points[w * 3]; cy = points[w * 3 + 1]; cz = points[w * 3 + 2];
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) cen[j - 1] = make_float4(cx, cy, cz, 0.f);
    }
    if (j >= K) return;
    unsigned long long best = 0ull;
    for (long long i = (long long)blockIdx.x * CL_BLOCK + threadIdx.x; i < N; i += (long long)gridDim.x * CL_BLOCK) {
        const float x = points[i * 3], y = points[i * 3 + 1], z = points[i * 3 + 2];
        if (!dbw::cluster_finite(x, y, z)) continue;
        const float d = dbw::cluster_dist2(x, y, z, cx, cy, cz);
        unsigned long long key;
        if (j == 0) {
            key = dbw::cluster_near_key(d, (uint32_t)i);
        } else {
            float m = d;
            if (j > 1) { const float old = mind[i]; m = d < old ? d : old; }
            mind[i] = m;
            key = dbw::cluster_far_key(m, (uint32_t)i);
        }
        best = key > best ? key : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_down(best, o, 64);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0) sh_key[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CL_WAVES; ++w) best = sh_key[w] > best ? sh_key[w] : best;
        if (best != 0ull) atomicMax(&keys[j], best);           // integer: the order of arrival does not matter
    }
}

// dynamic LDS: CL_WAVES tables of K x NSUM doubles
__global__ __launch_bounds__(CL_BLOCK) void cluster_assign_kernel(const float *__restrict__ points, long long N, const float4 *__restrict__ cen,
                                                                  int K, int first, int32_t *__restrict__ lab, int32_t *__restrict__ labels_out,
                                                                  ClusterState *__restrict__ state, double *__restrict__ partials) {
    extern __shared__ double sh_tab[];
    const int n_entries = K * NSUM;
    for (int e = threadIdx.x; e < CL_WAVES * n_entries; e += CL_BLOCK) sh_tab[e] = 0.0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *tab = sh_tab + wave * n_entries;
    int changed = 0;
    const long long n_tiles = (N + CL_TILE - 1) / CL_TILE;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        float px[CL_PTS], py[CL_PTS], pz[CL_PTS], best[CL_PTS];
        int label[CL_PTS];
        unsigned pend = 0u;                                     // bit q: point q of this lane waits to be added to its cluster's sums
#pragma unroll
        for (int q = 0; q < CL_PTS; ++q) {
            const long long i = tile * CL_TILE + q * CL_BLOCK + threadIdx.x;
            px[q] = py[q] = pz[q] = NAN;                        // (past the end: as a non-finite point, no label and no sum)
            if (i < N) { px[q] = points[i * 3]; py[q] = points[i * 3 + 1]; pz[q] = points[i * 3 + 2]; }
            best[q] = INFINITY;
            label[q] = dbw::cluster_finite(px[q], py[q], pz[q]) ? 0 : -1;
            if (label[q] == 0) pend |= 1u << q;
        }
#pragma unroll 4
        for (int k = 0; k < K; ++k) {
            const float4 c = cen[k];                            // wave-uniform address: scalar loads
#pragma unroll
            for (int q = 0; q < CL_PTS; ++q) {
                const float d = dbw::cluster_dist2(px[q], py[q], pz[q], c.x, c.y, c.z);
                const bool less = d < best[q];                  // (NaN for a past-the-end point: never; its label stays -1)
                best[q] = less ? d : best[q];
                label[q] = less ? k : label[q];
            }
        }
#pragma unroll
        for (int q = 0; q < CL_PTS; ++q) {
            const long long i = tile * CL_TILE + q * CL_BLOCK + threadIdx.x;
            if (i < N) {
                changed += (first || lab[i] != label[q]) ? 1 : 0;
                lab[i] = label[q];
                if (labels_out) labels_out[i] = label[q];
            }
        }
        // the clusters present in this wave, one at a time
        for (;;) {
            const unsigned long long waiting = __ballot(pend != 0u);
            if (waiting == 0ull) break;
            const int leader = __ffsll((long long)waiting) - 1;
            int mine = -1;                                      // the label of this lane's first pending point
#pragma unroll
            for (int q = CL_PTS - 1; q >= 0; --q) mine = ((pend >> q) & 1u) ? label[q] : mine;
            const int k = __builtin_amdgcn_readfirstlane(__shfl(mine, leader, 64));
            const float4 c4 = cen[k];
            const float c[3] = {c4.x, c4.y, c4.z};
            double acc[NSUM];
#pragma unroll
            for (int s = 0; s < NSUM; ++s) acc[s] = 0.0;
#pragma unroll
            for (int q = 0; q < CL_PTS; ++q) {                  // (q ascending is index ascending)
                if (((pend >> q) & 1u) && label[q] == k) {
                    dbw::cluster_point_moments(c, px[q], py[q], pz[q], acc);
                    pend &= ~(1u << q);
                }
            }
#pragma unroll
            for (int s = 0; s < NSUM; ++s) {
                double v = acc[s];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
                acc[s] = v;
            }
            if (lane == 0) {
#pragma unroll
                for (int s = 0; s < NSUM; ++s) tab[k * NSUM + s] += acc[s];
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) changed += __shfl_down(changed, o, 64);
    if (lane == 0 && changed) atomicAdd(&state->changed, changed);
    __syncthreads();
    for (int e = threadIdx.x; e < n_entries; e += CL_BLOCK) {
        double v = sh_tab[e];
        for (int w = 1; w < CL_WAVES; ++w) v += sh_tab[w * n_entries + e];
        partials[(long long)blockIdx.x * n_entries + e] = v;
    }
}

// One wave per cluster: lane s < NSUM adds the partials of sum s in workgroup order, lane 0 finishes.  A Lloyd round (final == 0) moves the
// centre; the final pass leaves it and writes the outputs.
__global__ __launch_bounds__(DBW_WAVE) void cluster_update_kernel(const double *__restrict__ partials, int groups, int K, int final_pass,
                                                                  ClusterState *__restrict__ state, float4 *__restrict__ cen,
                                                                  float *__restrict__ centres, int32_t *__restrict__ counts,
                                                                  double *__restrict__ mean_out, double *__restrict__ cov_out,
                                                                  double *__restrict__ evals_out, double *__restrict__ axes_out,
                                                                  int32_t *__restrict__ info) {
    __shared__ double sums[NSUM];
    const int k = blockIdx.x;
    if (threadIdx.x < NSUM) {
        double v = 0.0;
#pragma unroll 8
        for (int b = 0; b < groups; ++b) v += partials[((long long)b * K + k) * NSUM + threadIdx.x];       // (loads ahead, adds in order)
        sums[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s[NSUM], mean[3], cov[6];
    for (int i = 0; i < NSUM; ++i) s[i] = sums[i];
    const float4 c4 = cen[k];
    const float c[3] = {c4.x, c4.y, c4.z};
    float c_new[3];
    const int n = dbw::cluster_finish(s, c, c_new, mean, cov);
    if (!final_pass) {
        cen[k] = make_float4(c_new[0], c_new[1], c_new[2], 0.f);
        if (k == 0) { state->rounds += 1; state->changed = 0; }      // (the next pass counts from zero: it starts after this kernel)
        return;
    }
    centres[3 * k] = c[0]; centres[3 * k + 1] = c[1]; centres[3 * k + 2] = c[2];
    counts[k] = n;
    if (mean_out) { for (int i = 0; i < 3; ++i) mean_out[3 * k + i] = mean[i]; }
    if (cov_out) { for (int i = 0; i < 6; ++i) cov_out[6 * k + i] = cov[i]; }
    if (evals_out || axes_out) {
        double ev[3], ax[9];
        dbw::cluster_axes(n, cov, ev, ax);
        if (evals_out) { for (int i = 0; i < 3; ++i) evals_out[3 * k + i] = ev[i]; }
        if (axes_out) { for (int i = 0; i < 9; ++i) axes_out[9 * k + i] = ax[i]; }
    }
    if (n > 0) atomicAdd(&info[2], 1);
    if (k == 0) { info[0] = state->rounds; info[1] = state->changed; }
}

}  // namespace

extern "C" size_t dbw_eval_cluster_workspace_bytes(int64_t N, int K) { return cluster_sizes_ok(N, K) ? cluster_layout(N, K).total : 0; }

extern "C" int dbw_eval_cluster_fit(const float *points, int64_t N, int K, const float *init, int n_iter, void *workspace, float *centres,
                                    int32_t *labels, int32_t *counts, double *mean, double *cov, double *evals, double *axes, int32_t *info,
                                    dbw_stream_t stream) {
    DBW_REQUIRE(points && workspace && centres && counts && info, "null pointer");
    DBW_REQUIRE(K >= 1 && K <= dbw::CLUSTER_MAX_K, "K must be in [1, 256]");
    DBW_REQUIRE(N >= K && N < (1ll << 31), "N must be in [K, 2^31)");
    DBW_REQUIRE(n_iter >= 0 && n_iter <= dbw::CLUSTER_MAX_ITER, "n_iter must be in [0, 64]");
    DBW_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace is not 16-byte aligned");
    DBW_REQUIRE(((uintptr_t)points & 3) == 0 && ((uintptr_t)init & 3) == 0 && ((uintptr_t)centres & 3) == 0 && ((uintptr_t)labels & 3) == 0 &&
                    ((uintptr_t)counts & 3) == 0 && ((uintptr_t)info & 3) == 0 && ((uintptr_t)mean & 7) == 0 && ((uintptr_t)cov & 7) == 0 &&
                    ((uintptr_t)evals & 7) == 0 && ((uintptr_t)axes & 7) == 0,
                "misaligned pointer");
    const hipStream_t st = (hipStream_t)stream;
    const ClusterLayout L = cluster_layout(N, K);
    char *ws = (char *)workspace;
    ClusterState *state = (ClusterState *)(ws + L.state);
    float4 *cen = (float4 *)(ws + L.cen);
    unsigned long long *keys = (unsigned long long *)(ws + L.keys);
    double *mean_parts = (double *)(ws + L.mean_parts), *partials = (double *)(ws + L.partials);
    float *mind = (float *)(ws + L.mind);
    int32_t *lab = (int32_t *)(ws + L.lab);

    const size_t lds = (size_t)CL_WAVES * K * NSUM * sizeof(double);        // 80 KiB at K = 256
    if (lds > 64 * 1024) {                      // (a host-side attribute of the kernel on the current device: no launch, no synchronisation)
        if (hipFuncSetAttribute((const void *)cluster_assign_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                CL_WAVES * dbw::CLUSTER_MAX_K * NSUM * (int)sizeof(double)) != hipSuccess) {
            dbw_set_error("%s: %s", __func__, "cannot raise the LDS limit of cluster_assign_kernel");
            return DBW_ERR_INVALID;
        }
    }

    hipLaunchKernelGGL(cluster_begin_kernel, dim3(1), dim3(CL_BLOCK), 0, st, init, K, state, cen, keys, info);
    int rc = dbw_check_launch("cluster_begin_kernel");
    if (rc) return rc;
    if (!init) {
        hipLaunchKernelGGL(cluster_mean_kernel, dim3((unsigned)L.mean_parts_n), dim3(CL_BLOCK), 0, st, points, (long long)N, mean_parts);
        if ((rc = dbw_check_launch("cluster_mean_kernel"))) return rc;
        for (int j = 0; j <= K; ++j) {
            hipLaunchKernelGGL(cluster_seed_kernel, dim3(j < K ? (unsigned)L.seed_groups : 1u), dim3(CL_BLOCK), 0, st, points, (long long)N, j, K,
                               (const double *)mean_parts, L.mean_parts_n, keys, cen, mind);
            if ((rc = dbw_check_launch("cluster_seed_kernel"))) return rc;
        }
    }
    for (int r = 0; r <= n_iter; ++r) {
        const int final_pass = r == n_iter ? 1 : 0;
        hipLaunchKernelGGL(cluster_assign_kernel, dim3((unsigned)L.groups), dim3(CL_BLOCK), lds, st, points, (long long)N, (const float4 *)cen, K,
                           r == 0 ? 1 : 0, lab, final_pass ? labels : (int32_t *)nullptr, state, partials);
        if ((rc = dbw_check_launch("cluster_assign_kernel"))) return rc;
        hipLaunchKernelGGL(cluster_update_kernel, dim3((unsigned)K), dim3(DBW_WAVE), 0, st, (const double *)partials, L.groups, K, final_pass, state, cen,
                           centres, counts, mean, cov, evals, axes, info);
        if ((rc = dbw_check_launch("cluster_update_kernel"))) return rc;
    }
    return 0;
}
