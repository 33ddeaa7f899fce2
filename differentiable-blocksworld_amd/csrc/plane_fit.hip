// Plane RANSAC behind one call (include/dbw_eval.h: dbw_eval_plane_fit; reference src/utils/ransac.py).  The arithmetic is
// csrc/plane_math.h (also built by g++ for the host tests); this file is the schedule.
//
// Launches, all on one stream, kernel boundaries the only ordering, nothing read by the host:
//   plane_hyp_kernel      one lane per hypothesis: the triple (given or plane_draw), the plane, the priors -> hyp (Hpad,4) fp32, valid (Hpad)
//   plane_score_kernel    the hot one: N x H point-plane tests -> counts (Hpad) int32
//   plane_best_kernel     one workgroup: counts of invalid hypotheses -> -1, the largest count (lowest j on ties), the state of the refinement
//   refine x (plane_moments_kernel, plane_update_kernel)      ORTHOGONAL only: fp64 sums of the inliers, smallest eigenvector
//   plane_mask_kernel     the inliers of the final plane: mask, info[2]
//
// Scoring.  A workgroup of 256 lanes takes tiles of 256 * PLANE_PTS points, PLANE_PTS points per lane in registers, and walks ALL
// hypotheses per tile: a point is read once, whatever H.  The hypothesis index is wave-uniform, so its four floats arrive by scalar loads
// and sit in SGPRs; every test ends in a ballot, the wave's population counts are added in an SGPR, and the count of hypothesis j0 + k
// is kept in lane k of one VGPR (a select on the lane index): after 64 hypotheses the wave adds that VGPR to the workgroup's LDS table with one
// integer ds_add per lane.  A workgroup adds its table to the global counts once, at its end, with integer atomics: integer sums do not
// depend on the order.  There is no (H, N) array: the only per-hypothesis storage is hyp, valid and counts.
//
// Refinement sums are added in a fixed order, as csrc/icp_align.hip does: a lane adds its points in index order in fp64, the lanes of a
// wave by a shuffle tree, the waves through LDS in wave order, the workgroups' partials in index order by one lane per sum.
#include "dbw_common.h"
#include "plane_math.h"
#include "../../include/dbw_eval.h"

#include <math.h>

namespace {

constexpr int PLANE_BLOCK = 256;
constexpr int PLANE_WAVES = PLANE_BLOCK / DBW_WAVE;
constexpr int PLANE_PTS = 4;                    // points a lane keeps in registers
constexpr int PLANE_TILE = PLANE_BLOCK * PLANE_PTS;
constexpr int PLANE_MAX_GROUPS = 2048;          // workgroups of the scoring kernel, at most (256 CUs x 8)
constexpr int PLANE_MAX_PARTS = 128;            // workgroups of the moments kernel, at most
constexpr int PLANE_MAX_H = 4096;
constexpr int PLANE_MAX_REFINE = 8;

struct PlaneState {
    double plane[4];            // the current plane
    float a0[3];                // first point of the best triple: the origin of the refinement sums
    int32_t best, rounds, done;
    int32_t pad[2];
};
static_assert(sizeof(PlaneState) % 16 == 0, "the state keeps what follows it 16-byte aligned");

struct PlaneLayout {            // byte offsets into the workspace
    size_t hyp, valid, counts, state, partials, total;
    int hpad, parts;
};

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

inline PlaneLayout plane_layout(int64_t N, int H) {
    PlaneLayout L;
    L.hpad = (H + DBW_WAVE - 1) / DBW_WAVE * DBW_WAVE;
    const int64_t want = (N + PLANE_BLOCK - 1) / PLANE_BLOCK;
    L.parts = (int)(want < PLANE_MAX_PARTS ? want : PLANE_MAX_PARTS);
    size_t o = 0;
    L.hyp = o; o = align16(o + (size_t)L.hpad * 4 * sizeof(float));
    L.valid = o; o = align16(o + (size_t)L.hpad * sizeof(int32_t));
    L.counts = o; o = align16(o + (size_t)L.hpad * sizeof(int32_t));
    L.state = o; o = align16(o + sizeof(PlaneState));
    L.partials = o; o = align16(o + (size_t)L.parts * dbw::PLANE_NSUM * sizeof(double));
    L.total = o;
    return L;
}

inline bool plane_sizes_ok(int64_t N, int H) { return H >= 1 && H <= PLANE_MAX_H && N >= 3 && N < (1ll << 31); }

struct PlaneHypArgs {
    const float *points;
    const int32_t *triples;
    const float *up, *cams;
    float *hyp;
    int32_t *valid, *counts, *triples_out;
    long long N;
    unsigned long long seed;
    int H, hpad, mode, M, min_cams;
    float cos_tilt, tau;
};

__global__ __launch_bounds__(PLANE_BLOCK) void plane_hyp_kernel(PlaneHypArgs A) {
    const int j = blockIdx.x * PLANE_BLOCK + threadIdx.x;
    if (j >= A.hpad) return;
    float pl[4] = {0.f, 0.f, 0.f, INFINITY};                  // (a padding hypothesis: every residual is -inf, no inlier)
    int ok = 0;
    if (j < A.H) {
        int32_t idx[3];
        if (A.triples) {
            idx[0] = A.triples[3 * j]; idx[1] = A.triples[3 * j + 1]; idx[2] = A.triples[3 * j + 2];
        } else {
            dbw::plane_draw(A.seed, (uint32_t)j, A.N, idx);
        }
        if (A.triples_out) { A.triples_out[3 * j] = idx[0]; A.triples_out[3 * j + 1] = idx[1]; A.triples_out[3 * j + 2] = idx[2]; }
        const bool in_range = idx[0] >= 0 && idx[0] < A.N && idx[1] >= 0 && idx[1] < A.N && idx[2] >= 0 && idx[2] < A.N;
        if (in_range) {                                         // (a given triple outside the cloud is a degenerate one: never read)
            const float *a = A.points + (long long)idx[0] * 3, *b = A.points + (long long)idx[1] * 3, *c = A.points + (long long)idx[2] * 3;
            float out[4];
            bool good = dbw::plane_from_triple(a, b, c, A.mode, A.up, out);
            if (good && A.mode == dbw::PLANE_ORTHOGONAL) good = dbw::plane_admissible(out, A.up, A.cos_tilt, A.cams, A.M, A.tau, A.min_cams);
            if (good) { pl[0] = out[0]; pl[1] = out[1]; pl[2] = out[2]; pl[3] = out[3]; ok = 1; }
        }
    }
    A.hyp[4 * j] = pl[0]; A.hyp[4 * j + 1] = pl[1]; A.hyp[4 * j + 2] = pl[2]; A.hyp[4 * j + 3] = pl[3];
    A.valid[j] = ok;
    A.counts[j] = 0;
}

// dynamic LDS: hpad int32 counters
__global__ __launch_bounds__(PLANE_BLOCK) void plane_score_kernel(const float *__restrict__ points, long long N, const float4 *__restrict__ hyp, int hpad,
                                                                  float thresh2, int32_t *__restrict__ counts) {
    extern __shared__ int32_t sh_counts[];
    for (int j = threadIdx.x; j < hpad; j += PLANE_BLOCK) sh_counts[j] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long n_tiles = (N + PLANE_TILE - 1) / PLANE_TILE;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        float px[PLANE_PTS], py[PLANE_PTS], pz[PLANE_PTS];
#pragma unroll
        for (int k = 0; k < PLANE_PTS; ++k) {
            const long long i = tile * PLANE_TILE + k * PLANE_BLOCK + threadIdx.x;
            px[k] = py[k] = pz[k] = NAN;                        // (past the end: a NaN residual is no inlier)
            if (i < N) { px[k] = points[i * 3]; py[k] = points[i * 3 + 1]; pz[k] = points[i * 3 + 2]; }
        }
        for (int j0 = 0; j0 < hpad; j0 += DBW_WAVE) {
            int acc = 0;                                        // lane k: the wave's count of hypothesis j0 + k
#pragma unroll 8
            for (int k = 0; k < DBW_WAVE; ++k) {
                const float4 h = hyp[j0 + k];                   // wave-uniform address: scalar loads
                int cnt = 0;
#pragma unroll
                for (int q = 0; q < PLANE_PTS; ++q) {
                    const float r = ((h.x * px[q] + h.y * py[q]) + h.z * pz[q]) - h.w;
                    cnt += __popcll(__ballot(r * r < thresh2));
                }
                acc = lane == k ? cnt : acc;
            }
            atomicAdd(&sh_counts[j0 + lane], acc);
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < hpad; j += PLANE_BLOCK) {
        const int32_t c = sh_counts[j];
        if (c) atomicAdd(&counts[j], c);
    }
}

__global__ __launch_bounds__(PLANE_BLOCK) void plane_best_kernel(const float *__restrict__ points, const float *__restrict__ hyp,
                                                                 const int32_t *__restrict__ valid, int32_t *__restrict__ counts, int H, int mode,
                                                                 const int32_t *__restrict__ triples, unsigned long long seed, long long N,
                                                                 PlaneState *__restrict__ state, double *__restrict__ plane, int32_t *__restrict__ info,
                                                                 int32_t *__restrict__ counts_out) {
    __shared__ long long sh_key[PLANE_BLOCK];
    long long key = -1;                                         // count << 32 | (0xffffffff - j): the largest key is the largest count, lowest j
    for (int j = threadIdx.x; j < H; j += PLANE_BLOCK) {
        const int32_t c = valid[j] ? counts[j] : -1;
        if (counts_out) counts_out[j] = c;
        if (c >= 0) {
            const long long k = ((long long)c << 32) | (long long)(0xffffffffu - (unsigned)j);
            key = k > key ? k : key;
        }
    }
    sh_key[threadIdx.x] = key;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int t = 1; t < PLANE_BLOCK; ++t) key = sh_key[t] > key ? sh_key[t] : key;
    PlaneState s;
    s.pad[0] = s.pad[1] = 0;
    s.rounds = 0;
    if (key < 0) {
        s.best = -1; s.done = 1;
        s.plane[0] = s.plane[1] = s.plane[2] = s.plane[3] = 0.0;
        s.a0[0] = s.a0[1] = s.a0[2] = 0.f;
        info[1] = 0;
    } else {
        const int j = (int)(0xffffffffu - (unsigned)(key & 0xffffffffll));
        s.best = j; s.done = mode == dbw::PLANE_ORTHOGONAL ? 0 : 1;
        for (int k = 0; k < 4; ++k) s.plane[k] = (double)hyp[4 * j + k];
        int32_t idx[3];
        if (triples) idx[0] = triples[3 * j];
        else dbw::plane_draw(seed, (uint32_t)j, N, idx);
        for (int k = 0; k < 3; ++k) s.a0[k] = points[(long long)idx[0] * 3 + k];
        info[1] = (int32_t)(key >> 32);
    }
    *state = s;
    for (int k = 0; k < 4; ++k) plane[k] = s.plane[k];
    info[0] = s.best; info[2] = 0; info[3] = 0;
}

__global__ __launch_bounds__(PLANE_BLOCK) void plane_moments_kernel(const float *__restrict__ points, long long N, float thresh2,
                                                                    const PlaneState *__restrict__ state, double *__restrict__ partials) {
    __shared__ double sh[PLANE_WAVES][dbw::PLANE_NSUM];
    if (state->done) return;                                    // (uniform over the grid: the update kernel does not read the partials then)
    const float pl[4] = {(float)state->plane[0], (float)state->plane[1], (float)state->plane[2], (float)state->plane[3]};
    const float a0[3] = {state->a0[0], state->a0[1], state->a0[2]};
    double acc[dbw::PLANE_NSUM];
#pragma unroll
    for (int k = 0; k < dbw::PLANE_NSUM; ++k) acc[k] = 0.0;
    for (long long i = (long long)blockIdx.x * PLANE_BLOCK + threadIdx.x; i < N; i += (long long)gridDim.x * PLANE_BLOCK)
        dbw::plane_point_moments(pl, a0, points[i * 3], points[i * 3 + 1], points[i * 3 + 2], thresh2, acc);
#pragma unroll
    for (int k = 0; k < dbw::PLANE_NSUM; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        acc[k] = v;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < dbw::PLANE_NSUM; ++k) sh[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < dbw::PLANE_NSUM) {
        double v = sh[0][threadIdx.x];
        for (int w = 1; w < PLANE_WAVES; ++w) v += sh[w][threadIdx.x];
        partials[(long long)blockIdx.x * dbw::PLANE_NSUM + threadIdx.x] = v;
    }
}

// one wave: lane k < PLANE_NSUM adds the partials of sum k in workgroup order, lane 0 takes the step
__global__ __launch_bounds__(DBW_WAVE) void plane_update_kernel(const double *__restrict__ partials, int parts, PlaneState *__restrict__ state,
                                                                double *__restrict__ plane, int32_t *__restrict__ info) {
    __shared__ double sums[dbw::PLANE_NSUM];
    if (state->done) return;
    if (threadIdx.x < dbw::PLANE_NSUM) {
        double v = 0.0;
#pragma unroll 8
        for (int b = 0; b < parts; ++b) v += partials[(long long)b * dbw::PLANE_NSUM + threadIdx.x];       // (loads ahead, adds in order)
        sums[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s[dbw::PLANE_NSUM], pl[4];
    for (int k = 0; k < dbw::PLANE_NSUM; ++k) s[k] = sums[k];
    for (int k = 0; k < 4; ++k) pl[k] = state->plane[k];
    const float a0[3] = {state->a0[0], state->a0[1], state->a0[2]};
    if (!dbw::plane_refine_step(s, a0, pl)) { state->done = 1; return; }
    for (int k = 0; k < 4; ++k) { state->plane[k] = pl[k]; plane[k] = pl[k]; }
    state->rounds += 1;
    info[3] = state->rounds;
}

__global__ __launch_bounds__(PLANE_BLOCK) void plane_mask_kernel(const float *__restrict__ points, long long N, float thresh2,
                                                                 const PlaneState *__restrict__ state, uint8_t *__restrict__ mask,
                                                                 int32_t *__restrict__ info) {
    __shared__ int sh_count[PLANE_WAVES];
    const bool none = state->best < 0;
    const float pl[4] = {(float)state->plane[0], (float)state->plane[1], (float)state->plane[2], (float)state->plane[3]};
    int mine = 0;
    for (long long i = (long long)blockIdx.x * PLANE_BLOCK + threadIdx.x; i < N; i += (long long)gridDim.x * PLANE_BLOCK) {
        const bool in = !none && dbw::plane_inlier(pl, points[i * 3], points[i * 3 + 1], points[i * 3 + 2], thresh2);
        if (mask) mask[i] = in ? 1 : 0;
        mine += in ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
    if ((threadIdx.x & 63) == 0) sh_count[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {                                     // one integer atomic per workgroup
        int c = 0;
        for (int w = 0; w < PLANE_WAVES; ++w) c += sh_count[w];
        if (c) atomicAdd(&info[2], c);
    }
}

}  // namespace

extern "C" size_t dbw_eval_plane_workspace_bytes(int64_t N, int H) { return plane_sizes_ok(N, H) ? plane_layout(N, H).total : 0; }

extern "C" int dbw_eval_plane_fit(const float *points, int64_t N, int H, int mode, float thresh2, int64_t seed, const int32_t *triples,
                                  const float *up, float cos_tilt, const float *cams, int M, float tau, int min_cams, int refine, void *workspace,
                                  double *plane, int32_t *info, int32_t *counts, int32_t *triples_out, uint8_t *mask, dbw_stream_t stream) {
    DBW_REQUIRE(points && workspace && plane && info, "null pointer");
    DBW_REQUIRE(H >= 1 && H <= PLANE_MAX_H, "H must be in [1, 4096]");
    DBW_REQUIRE(N >= 3 && N < (1ll << 31), "N must be in [3, 2^31)");
    DBW_REQUIRE(refine >= 0 && refine <= PLANE_MAX_REFINE, "refine must be in [0, 8]");
    DBW_REQUIRE(mode == dbw::PLANE_ORTHOGONAL || mode == dbw::PLANE_VERTICAL, "mode must be 0 (orthogonal) or 1 (vertical)");
    DBW_REQUIRE(thresh2 > 0.f && thresh2 < INFINITY, "thresh2 must be positive and finite");
    DBW_REQUIRE(cams ? (M >= 1 && M <= 65536 && min_cams >= 0 && min_cams <= M && tau >= 0.f && tau < INFINITY) : M == 0,
                "cams need 1 <= M <= 65536, 0 <= min_cams <= M and a finite tau >= 0; without cams M must be 0");
    DBW_REQUIRE(!up || (cos_tilt >= -1.f && cos_tilt <= 1.f), "cos_tilt must be in [-1, 1]");
    DBW_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace is not 16-byte aligned");
    DBW_REQUIRE(((uintptr_t)points & 3) == 0 && ((uintptr_t)triples & 3) == 0 && ((uintptr_t)up & 3) == 0 && ((uintptr_t)cams & 3) == 0 &&
                    ((uintptr_t)plane & 7) == 0 && ((uintptr_t)info & 3) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)triples_out & 3) == 0,
                "misaligned pointer");
    const hipStream_t st = (hipStream_t)stream;
    const PlaneLayout L = plane_layout(N, H);
    char *ws = (char *)workspace;
    float *hyp = (float *)(ws + L.hyp);
    int32_t *valid = (int32_t *)(ws + L.valid), *cnt = (int32_t *)(ws + L.counts);
    PlaneState *state = (PlaneState *)(ws + L.state);
    double *partials = (double *)(ws + L.partials);

    PlaneHypArgs A;
    A.points = points; A.triples = triples; A.up = up; A.cams = cams; A.hyp = hyp; A.valid = valid; A.counts = cnt; A.triples_out = triples_out;
    A.N = N; A.seed = (unsigned long long)seed; A.H = H; A.hpad = L.hpad; A.mode = mode; A.M = cams ? M : 0; A.min_cams = min_cams;
    A.cos_tilt = cos_tilt; A.tau = tau;
    hipLaunchKernelGGL(plane_hyp_kernel, dim3((unsigned)((L.hpad + PLANE_BLOCK - 1) / PLANE_BLOCK)), dim3(PLANE_BLOCK), 0, st, A);
    int rc = dbw_check_launch("plane_hyp_kernel");
    if (rc) return rc;
    const long long n_tiles = (N + PLANE_TILE - 1) / PLANE_TILE;
    const unsigned groups = (unsigned)(n_tiles < PLANE_MAX_GROUPS ? n_tiles : PLANE_MAX_GROUPS);
    hipLaunchKernelGGL(plane_score_kernel, dim3(groups), dim3(PLANE_BLOCK), (size_t)L.hpad * sizeof(int32_t), st, points, (long long)N,
                       (const float4 *)hyp, L.hpad, thresh2, cnt);
    if ((rc = dbw_check_launch("plane_score_kernel"))) return rc;
    hipLaunchKernelGGL(plane_best_kernel, dim3(1), dim3(PLANE_BLOCK), 0, st, points, (const float *)hyp, (const int32_t *)valid, cnt, H, mode, triples,
                       (unsigned long long)seed, (long long)N, state, plane, info, counts);
    if ((rc = dbw_check_launch("plane_best_kernel"))) return rc;
    if (mode == dbw::PLANE_ORTHOGONAL) {
        for (int r = 0; r < refine; ++r) {
            hipLaunchKernelGGL(plane_moments_kernel, dim3((unsigned)L.parts), dim3(PLANE_BLOCK), 0, st, points, (long long)N, thresh2,
                               (const PlaneState *)state, partials);
            if ((rc = dbw_check_launch("plane_moments_kernel"))) return rc;
            hipLaunchKernelGGL(plane_update_kernel, dim3(1), dim3(DBW_WAVE), 0, st, (const double *)partials, L.parts, state, plane, info);
            if ((rc = dbw_check_launch("plane_update_kernel"))) return rc;
        }
    }
    const long long want = (N + PLANE_BLOCK - 1) / PLANE_BLOCK;
    hipLaunchKernelGGL(plane_mask_kernel, dim3((unsigned)(want < PLANE_MAX_GROUPS ? want : PLANE_MAX_GROUPS)), dim3(PLANE_BLOCK), 0, st, points, (long long)N,
                       thresh2, (const PlaneState *)state, mask, info);
    return dbw_check_launch("plane_mask_kernel");
}
