// Gradient ICP behind one call (include/dbw_icp.h; reference src/utils/icp.py:11-78).  The arithmetic is csrc/icp_math.h (also built by g++
// for the host tests); the two searches of an iteration are nn_search_kernel through csrc/nn_search.h.
//
// An iteration is five launches on one stream, and kernel boundaries are the only ordering: transform (q from each instance's 12-float
// M | T block), search pred -> gt, search gt -> pred, moments, update.  Nothing is read by the host: the Adam scalars of every step are
// computed on the host beforehand and travel as kernel arguments, the keep-best meter lives in the workspace.
//
// Moments.  A workgroup of 256 lanes walks its points with a fixed stride; a lane adds its pairs' 13 terms in index order in fp64 registers,
// the lanes of a wave are added by a shuffle tree, the four waves through LDS in wave order, and the workgroup writes its 13 partials to the
// workspace.  The update kernel adds the partials of a (instance, direction, sum) in workgroup order, one lane per sum.  No atomics: the
// order of every addition is a function of the sizes alone, so two runs give the same bits.  The gathers (g[idx], q[idx], p[idx]) are random
// reads over 1.2 MB per cloud at the evaluator's 100k points: they stay in L2.
#include "dbw_common.h"
#include "icp_math.h"
#include "nn_search.h"
#include "../../include/dbw_icp.h"

#include <math.h>

namespace {

constexpr int ICP_BLOCK = 256;
constexpr int ICP_WAVES = ICP_BLOCK / DBW_WAVE;
constexpr int ICP_MAX_PARTS = 128;      // workgroups per (instance, direction) of the moments kernel, at most

struct IcpState {                       // one instance, fp32
    float param[dbw::ICP_NPARAM], m[dbw::ICP_NPARAM], v[dbw::ICP_NPARAM];
    float blk[12];                      // M | T of the next transform
    float best[dbw::ICP_NRTS];          // the kept R | T | s
    float pad;
};
static_assert(sizeof(IcpState) % 16 == 0, "instances stay 16-byte aligned");

struct IcpLayout {                      // byte offsets into the workspace
    size_t keys1, keys2, partials, sums, meter, state, q, total;
    int parts;
};

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

inline IcpLayout icp_layout(int N, int P1, int P2) {
    IcpLayout L;
    const int pmax = P1 > P2 ? P1 : P2;
    const long long want = ((long long)pmax + ICP_BLOCK - 1) / ICP_BLOCK;
    L.parts = (int)(want < ICP_MAX_PARTS ? want : ICP_MAX_PARTS);
    size_t o = 0;
    L.keys1 = o; o = align16(o + (size_t)N * P1 * sizeof(unsigned long long));
    L.keys2 = o; o = align16(o + (size_t)N * P2 * sizeof(unsigned long long));
    L.partials = o; o = align16(o + (size_t)N * 2 * L.parts * dbw::ICP_NSUM * sizeof(double));
    L.sums = o; o = align16(o + (size_t)N * 2 * dbw::ICP_NSUM * sizeof(double));
    L.meter = o; o = align16(o + sizeof(dbw::IcpMeter));
    L.state = o; o = align16(o + (size_t)N * sizeof(IcpState));
    L.q = o; o = align16(o + (size_t)N * P1 * 3 * sizeof(float));
    L.total = o;
    return L;
}

inline bool icp_sizes_ok(int N, int P1, int P2, int n_iter) {
    return N > 0 && N < 65536 && P1 > 0 && P2 > 0 && n_iter >= 0 && n_iter <= (1 << 24) && (long long)N * P1 < (1ll << 34) &&
           (long long)N * P2 < (1ll << 34);
}

__global__ void icp_init_kernel(IcpState *__restrict__ state, dbw::IcpMeter *__restrict__ meter, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n == 0) dbw::icp_meter_init(*meter);
    if (n >= N) return;
    IcpState &s = state[n];
    dbw::icp_identity(s.param, s.best, s.blk);
    for (int k = 0; k < dbw::ICP_NPARAM; ++k) s.m[k] = s.v[k] = 0.f;
    s.pad = 0.f;
}

// q[n, i] = transform of p[n, i] by instance n's block, or (from_best) by the block of its kept parameters
__global__ __launch_bounds__(ICP_BLOCK) void icp_transform_kernel(const float *__restrict__ p, const IcpState *__restrict__ state, int P1,
                                                                  int from_best, float *__restrict__ q) {
    const int n = blockIdx.y;
    const int i = blockIdx.x * ICP_BLOCK + threadIdx.x;
    if (i >= P1) return;
    float blk[12];
    if (from_best) {
        const float *b = state[n].best;
        dbw::icp_block(b, b + 9, b + 12, blk);
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) blk[k] = state[n].blk[k];
    }
    const float *src = p + ((long long)n * P1 + i) * 3;
    float out[3];
    dbw::icp_transform(blk, src[0], src[1], src[2], out);
    float *dst = q + ((long long)n * P1 + i) * 3;
    dst[0] = out[0]; dst[1] = out[1]; dst[2] = out[2];
}

// grid (parts, 2, N): direction 0 walks the pred points (pair: q_i, g[key1_i], p_i), direction 1 the gt points (q[key2_j], g_j, p[key2_j])
__global__ __launch_bounds__(ICP_BLOCK) void icp_moments_kernel(const float *__restrict__ p, const float *__restrict__ g,
                                                                const float *__restrict__ q, const unsigned long long *__restrict__ keys1,
                                                                const unsigned long long *__restrict__ keys2, int P1, int P2,
                                                                double *__restrict__ partials) {
    __shared__ double sh[ICP_WAVES][dbw::ICP_NSUM];
    const int dir = blockIdx.y, n = blockIdx.z, parts = gridDim.x;
    const int P = dir == 0 ? P1 : P2;
    const unsigned other = (unsigned)(dir == 0 ? P2 : P1);
    const unsigned long long *keys = dir == 0 ? keys1 + (long long)n * P1 : keys2 + (long long)n * P2;
    const float *pb = p + (long long)n * P1 * 3, *qb = q + (long long)n * P1 * 3, *gb = g + (long long)n * P2 * 3;
    double acc[dbw::ICP_NSUM];
#pragma unroll
    for (int k = 0; k < dbw::ICP_NSUM; ++k) acc[k] = 0.0;
    for (long long i = (long long)blockIdx.x * ICP_BLOCK + threadIdx.x; i < P; i += (long long)parts * ICP_BLOCK) {
        const unsigned j = (unsigned)(keys[i] & 0xffffffffull);
        if (j >= other) continue;                                   // (a query without a neighbour: cannot happen with full clouds)
        const long long ip = dir == 0 ? i : (long long)j, ig = dir == 0 ? (long long)j : i;
        dbw::icp_pair_moments(qb + ip * 3, gb + ig * 3, pb + ip * 3, acc);
    }
#pragma unroll
    for (int k = 0; k < dbw::ICP_NSUM; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        acc[k] = v;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < dbw::ICP_NSUM; ++k) sh[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < dbw::ICP_NSUM) {
        double v = sh[0][threadIdx.x];
        for (int w = 1; w < ICP_WAVES; ++w) v += sh[w][threadIdx.x];
        partials[(((long long)n * 2 + dir) * parts + blockIdx.x) * dbw::ICP_NSUM + threadIdx.x] = v;
    }
}

struct IcpUpdateArgs {
    const double *partials;
    double *sums;
    dbw::IcpMeter *meter;
    IcpState *state;
    double *trace;              // this iteration's row, or NULL
    int N, P1, P2, parts, it, estimate_scale, anisotropic;
    dbw::IcpAdam adam;
};

// one workgroup: (1) every (instance, direction, sum) adds its partials in workgroup order, one lane each; (2) thread 0 forms the
// batch-mean loss and applies the keep-best rule; (3) one thread per instance takes the step
__global__ __launch_bounds__(ICP_BLOCK) void icp_update_kernel(IcpUpdateArgs A) {
    __shared__ int keep;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int NS = 2 * dbw::ICP_NSUM;
    if (lane < NS) {
        for (int n = wave; n < A.N; n += ICP_WAVES) {
            const double *src = A.partials + ((long long)n * 2 + lane / dbw::ICP_NSUM) * A.parts * dbw::ICP_NSUM + lane % dbw::ICP_NSUM;
            double v = 0.0;
            for (int b = 0; b < A.parts; ++b) v += src[(long long)b * dbw::ICP_NSUM];
            A.sums[(long long)n * NS + lane] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double loss = 0.0;
        for (int n = 0; n < A.N; ++n) loss += dbw::icp_instance_loss(A.sums + (long long)n * NS, A.P1, A.P2);
        loss /= (double)A.N;
        dbw::IcpMeter m = *A.meter;
        keep = dbw::icp_keep_best(m, loss, A.N, A.it) ? 1 : 0;
        *A.meter = m;
        if (A.trace) A.trace[0] = loss;
    }
    __syncthreads();
    for (int n = threadIdx.x; n < A.N; n += ICP_BLOCK) {
        IcpState &s = A.state[n];
        float rts[dbw::ICP_NRTS];
        dbw::icp_step(s.param, s.m, s.v, A.sums + (long long)n * NS, A.N, A.P1, A.P2, A.estimate_scale, A.anisotropic, A.adam, s.blk, rts);
        if (keep) {
#pragma unroll
            for (int k = 0; k < dbw::ICP_NRTS; ++k) s.best[k] = rts[k];
        }
        if (A.trace) {
#pragma unroll
            for (int k = 0; k < dbw::ICP_NRTS; ++k) A.trace[1 + (long long)n * dbw::ICP_NRTS + k] = (double)rts[k];
        }
    }
}

__global__ void icp_output_kernel(const IcpState *__restrict__ state, const dbw::IcpMeter *__restrict__ meter, int N, float *__restrict__ out_R,
                                  float *__restrict__ out_T, float *__restrict__ out_s, double *__restrict__ out_best) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n == 0) { out_best[0] = meter->loss_min; out_best[1] = meter->best_iter; }
    if (n >= N) return;
    const float *b = state[n].best;
    for (int k = 0; k < 9; ++k) out_R[(long long)n * 9 + k] = b[k];
    for (int k = 0; k < 3; ++k) { out_T[(long long)n * 3 + k] = b[9 + k]; out_s[(long long)n * 3 + k] = b[12 + k]; }
}

}  // namespace

extern "C" int dbw_icp_abi_version(void) { return DBW_ICP_ABI_VERSION; }      // (history: include/dbw_icp.h)

extern "C" size_t dbw_icp_workspace_bytes(int N, int P1, int P2, int n_iter) {
    return icp_sizes_ok(N, P1, P2, n_iter) ? icp_layout(N, P1, P2).total : 0;
}

extern "C" int dbw_icp_run(const float *pred, const float *gt, int N, int P1, int P2, int estimate_scale, int anisotropic_scale, double lr,
                           int n_iter, int splits, void *workspace, float *out_cloud, float *out_R, float *out_T, float *out_s, double *out_best,
                           double *trace, dbw_stream_t stream) {
    DBW_REQUIRE(pred && gt && workspace && out_cloud && out_R && out_T && out_s && out_best, "null pointer");
    DBW_REQUIRE(icp_sizes_ok(N, P1, P2, n_iter) && splits >= 0, "bad size");
    DBW_REQUIRE((estimate_scale == 0 || estimate_scale == 1) && (anisotropic_scale == 0 || anisotropic_scale == 1), "flags must be 0 or 1");
    DBW_REQUIRE(lr > 0.0 && lr < INFINITY, "lr must be positive and finite");
    DBW_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace is not 16-byte aligned");
    DBW_REQUIRE(((uintptr_t)pred & 3) == 0 && ((uintptr_t)gt & 3) == 0 && ((uintptr_t)out_cloud & 3) == 0 && ((uintptr_t)out_R & 3) == 0 &&
                    ((uintptr_t)out_T & 3) == 0 && ((uintptr_t)out_s & 3) == 0 && ((uintptr_t)out_best & 7) == 0 && ((uintptr_t)trace & 7) == 0,
                "misaligned pointer");
    int splits1 = 1, splits2 = 1;
    if (n_iter > 0) {
        splits1 = dbw_nn_search_plan(__func__, N, P1, P2, splits);
        if (splits1 < 0) return splits1;
        splits2 = dbw_nn_search_plan(__func__, N, P2, P1, splits);
        if (splits2 < 0) return splits2;
    }
    const hipStream_t st = (hipStream_t)stream;
    const IcpLayout L = icp_layout(N, P1, P2);
    char *ws = (char *)workspace;
    unsigned long long *keys1 = (unsigned long long *)(ws + L.keys1), *keys2 = (unsigned long long *)(ws + L.keys2);
    double *partials = (double *)(ws + L.partials);
    IcpState *state = (IcpState *)(ws + L.state);
    dbw::IcpMeter *meter = (dbw::IcpMeter *)(ws + L.meter);
    float *q = (float *)(ws + L.q);
    const dim3 grid_t((unsigned)((P1 + ICP_BLOCK - 1) / ICP_BLOCK), (unsigned)N);

    hipLaunchKernelGGL(icp_init_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, state, meter, N);
    int rc = dbw_check_launch("icp_init_kernel");
    if (rc) return rc;
    IcpUpdateArgs A;
    A.partials = partials; A.sums = (double *)(ws + L.sums); A.meter = meter; A.state = state;
    A.N = N; A.P1 = P1; A.P2 = P2; A.parts = L.parts; A.estimate_scale = estimate_scale; A.anisotropic = anisotropic_scale;
    for (int it = 0; it < n_iter; ++it) {
        hipLaunchKernelGGL(icp_transform_kernel, grid_t, dim3(ICP_BLOCK), 0, st, pred, (const IcpState *)state, P1, 0, q);
        if ((rc = dbw_check_launch("icp_transform_kernel"))) return rc;
        if ((rc = dbw_nn_search_launch(q, gt, nullptr, nullptr, N, P1, P2, splits1, keys1, st))) return rc;
        if ((rc = dbw_nn_search_launch(gt, q, nullptr, nullptr, N, P2, P1, splits2, keys2, st))) return rc;
        hipLaunchKernelGGL(icp_moments_kernel, dim3((unsigned)L.parts, 2, (unsigned)N), dim3(ICP_BLOCK), 0, st, pred, gt, (const float *)q,
                           (const unsigned long long *)keys1, (const unsigned long long *)keys2, P1, P2, partials);
        if ((rc = dbw_check_launch("icp_moments_kernel"))) return rc;
        A.it = it;
        A.adam = dbw::icp_adam_scalars(lr, it + 1);
        A.trace = trace ? trace + (long long)it * (1 + (long long)N * dbw::ICP_NRTS) : nullptr;
        hipLaunchKernelGGL(icp_update_kernel, dim3(1), dim3(ICP_BLOCK), 0, st, A);
        if ((rc = dbw_check_launch("icp_update_kernel"))) return rc;
    }
    hipLaunchKernelGGL(icp_transform_kernel, grid_t, dim3(ICP_BLOCK), 0, st, pred, (const IcpState *)state, P1, 1, out_cloud);
    if ((rc = dbw_check_launch("icp_transform_kernel"))) return rc;
    hipLaunchKernelGGL(icp_output_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, (const IcpState *)state, (const dbw::IcpMeter *)meter, N,
                       out_R, out_T, out_s, out_best);
    return dbw_check_launch("icp_output_kernel");
}
