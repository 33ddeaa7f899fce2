// The point cloud of a capture's depth maps (include/dbw_lens.h: dbw_lens_depth_cloud): (N,H,W) uint16 depths, every frame
// with its own lens and pose, unprojected into the normalised world frame and reduced on a grid of G^3 cells to one point per occupied
// cell.  The arithmetic is depth_math.h (host + device).
//
// Four steps on the caller's stream, nothing read by the host:
//   clear       the workspace is zeroed (16-byte stores), whatever it held
//   accumulate  one thread per selected target pixel, the frame in blockIdx.z: the camera and pose rows are uniform (scalar) loads from the
//               kernel-argument block, where they travel BY VALUE, DEPTH_GROUP = 16 frames to a launch (64 + 48 bytes a frame: within the
//               2 KiB of arguments dbw_lens_rectify_u8 sends); the launches of a call add into the same cells.  A sample is four relaxed
//               agent-scope integer atomics into ONE 32-byte cell record (the count and the three sums share a cache line); integer
//               addition is associative, so the words do not depend on the order of arrival.  The two sample counters take one add a wave.
//   count, scan, emit   occupied cells (count >= min_count) per tile of 1024 cells, an exclusive scan of the tile counts by one block, and
//               the rows written in ascending cell order: a thread owns 4 consecutive cells, a block scan places them.
// No lane pre-aggregation in front of the atomics: profiles/depth_cloud.md has what was measured.
#include "dbw_common.h"
#include "depth_math.h"
#include "../../include/dbw_lens.h"

namespace {

using namespace dbw;

constexpr int DEPTH_GROUP = 16;             // frames of one launch
constexpr int DEPTH_BLOCK = 256;
constexpr int DEPTH_PER_THREAD = 4;         // consecutive cells of a thread of the compaction
constexpr int DEPTH_TILE = DEPTH_BLOCK * DEPTH_PER_THREAD;
constexpr int DEPTH_SCAN_BLOCK = 1024;      // the one block that scans the tile counts

struct DepthCell {                          // 32 bytes: one cache-line sector per sample
    unsigned long long sum[3];
    uint32_t count, pad;
};
static_assert(sizeof(DepthCell) == 32, "a cell record is 32 bytes");

struct DepthArgs {
    int n, Hs, Ws, stride;                  // n: frames of this launch; Hs x Ws: the selected pixels of a frame
    DepthRule rule;
    int pad[2];
    float target[4], box[4];
    float cams[DEPTH_GROUP][LENS_RECT_N_PARAMS];
    float poses[DEPTH_GROUP][DEPTH_POSE_N];
};
struct DepthBox {
    float v[4];
};

// cells | tile counts (then offsets) | the two sample counters
struct DepthLayout {
    long long n_cells;
    int n_tiles;
    size_t tiles, counters, total;
};
DepthLayout depth_layout(int G) {
    DepthLayout L;
    L.n_cells = (long long)G * G * G;
    L.n_tiles = (int)((L.n_cells + DEPTH_TILE - 1) / DEPTH_TILE);
    L.tiles = (size_t)L.n_cells * sizeof(DepthCell);
    L.counters = L.tiles + (((size_t)L.n_tiles * 4 + 15) / 16) * 16;
    L.total = L.counters + 16;
    return L;
}

__global__ void __launch_bounds__(DEPTH_BLOCK) depth_clear_kernel(uint4 *w, long long n16) {
    for (long long k = (long long)blockIdx.x * DEPTH_BLOCK + threadIdx.x; k < n16; k += (long long)gridDim.x * DEPTH_BLOCK) w[k] = make_uint4(0u, 0u, 0u, 0u);
}

template <typename T>
__device__ __forceinline__ void depth_add(T *p, T v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(DEPTH_BLOCK) depth_accumulate_kernel(DepthArgs A, const uint16_t *__restrict__ depth, DepthCell *__restrict__ cells,
                                                                      unsigned long long *__restrict__ counters) {
    const long long p = (long long)blockIdx.x * DEPTH_BLOCK + threadIdx.x;
    const int n = blockIdx.z;                                       // (gridDim.z == A.n)
    int cell = DEPTH_DROPPED, q[3] = {0, 0, 0};
    if (p < (long long)A.Hs * A.Ws) {
        const int i = (int)(p / A.Ws) * A.stride, j = (int)(p % A.Ws) * A.stride;
        cell = depth_sample(depth + (long long)n * A.rule.H * A.rule.W, A.rule, lens_cam(A.cams[n]), lens_target(A.target), A.poses[n], A.box, i, j, q);
    }
    if (cell >= 0) {                                                // (cell < G^3: every q >> 10 is below G)
        DepthCell *c = cells + cell;
        depth_add(&c->count, 1u);
        depth_add(&c->sum[0], (unsigned long long)q[0]);
        depth_add(&c->sum[1], (unsigned long long)q[1]);
        depth_add(&c->sum[2], (unsigned long long)q[2]);
    }
    const unsigned long long in = __ballot(cell >= 0), outside = __ballot(cell == DEPTH_OUTSIDE);
    if ((threadIdx.x & 63) == 0) {
        if (in) depth_add(counters, (unsigned long long)__popcll(in));
        if (outside) depth_add(counters + 1, (unsigned long long)__popcll(outside));
    }
}

// The depth rays (dbw_lens_depth_rays): the accumulate kernel's layout -- one thread per selected pixel, the frame in blockIdx.z, camera and
// pose rows by value --, one 16-byte record a pixel: the ray's end and its frame, or zeros and -1 where there is no measurement.
__global__ void __launch_bounds__(DEPTH_BLOCK) depth_rays_kernel(DepthArgs A, int frame0, const uint16_t *__restrict__ depth, float4 *__restrict__ rays) {
    const long long p = (long long)blockIdx.x * DEPTH_BLOCK + threadIdx.x;
    const int n = blockIdx.z;                                       // (gridDim.z == A.n)
    const long long px = (long long)A.Hs * A.Ws;
    if (p >= px) return;
    const int i = (int)(p / A.Ws) * A.stride, j = (int)(p % A.Ws) * A.stride;
    float e[3] = {0.0f, 0.0f, 0.0f};
    const bool ok = depth_ray_end(depth + (long long)n * A.rule.H * A.rule.W, A.rule, lens_cam(A.cams[n]), lens_target(A.target), A.poses[n], i, j, e);
    rays[(long long)n * px + p] = ok ? make_float4(e[0], e[1], e[2], __int_as_float(frame0 + n)) : make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
}

// The exclusive scan of one int per thread over a block of THREADS (a multiple of 64); *total: the block's sum.  lds: THREADS / 64 + 1 ints.
template <int THREADS>
__device__ __forceinline__ int block_scan(int v, int *lds, int *total) {
    constexpr int NW = THREADS / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(x, o, 64);
        if (lane >= o) x += t;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int w = 0; w < NW; ++w) {
            const int t = lds[w];
            lds[w] = run;
            run += t;
        }
        lds[NW] = run;
    }
    __syncthreads();
    *total = lds[NW];
    return x - v + lds[wave];
}

__global__ void __launch_bounds__(DEPTH_BLOCK) depth_count_kernel(const DepthCell *__restrict__ cells, long long n_cells, uint32_t min_count,
                                                                 int *__restrict__ tiles) {
    __shared__ int lds[DEPTH_BLOCK / 64 + 1];
    const long long base = (long long)blockIdx.x * DEPTH_TILE + threadIdx.x * DEPTH_PER_THREAD;
    int c = 0;
#pragma unroll
    for (int k = 0; k < DEPTH_PER_THREAD; ++k)
        if (base + k < n_cells && cells[base + k].count >= min_count) ++c;
    int total;
    block_scan<DEPTH_BLOCK>(c, lds, &total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

// tiles[0 .. n_tiles): counts -> exclusive offsets, in place; info = [M, samples accumulated, samples outside the box]
__global__ void __launch_bounds__(DEPTH_SCAN_BLOCK) depth_scan_kernel(int *__restrict__ tiles, int n_tiles, const unsigned long long *__restrict__ counters,
                                                                     int64_t *__restrict__ info) {
    __shared__ int lds[DEPTH_SCAN_BLOCK / 64 + 1];
    const int per = (n_tiles + DEPTH_SCAN_BLOCK - 1) / DEPTH_SCAN_BLOCK;        // consecutive tiles of a thread
    const int t0 = threadIdx.x * per;
    int sum = 0;
    for (int k = 0; k < per; ++k)
        if (t0 + k < n_tiles) sum += tiles[t0 + k];
    int total;
    int run = block_scan<DEPTH_SCAN_BLOCK>(sum, lds, &total);
    for (int k = 0; k < per; ++k)
        if (t0 + k < n_tiles) {
            const int t = tiles[t0 + k];
            tiles[t0 + k] = run;
            run += t;
        }
    if (threadIdx.x == 0) {
        info[0] = total;
        info[1] = (int64_t)counters[0];
        info[2] = (int64_t)counters[1];
    }
}

__global__ void __launch_bounds__(DEPTH_BLOCK) depth_emit_kernel(const DepthCell *__restrict__ cells, long long n_cells, uint32_t min_count,
                                                                const int *__restrict__ tiles, DepthBox B, float *__restrict__ points,
                                                                int32_t *__restrict__ counts, long long capacity) {
    __shared__ int lds[DEPTH_BLOCK / 64 + 1];
    const long long base = (long long)blockIdx.x * DEPTH_TILE + threadIdx.x * DEPTH_PER_THREAD;
    uint32_t cnt[DEPTH_PER_THREAD];
    int c = 0;
#pragma unroll
    for (int k = 0; k < DEPTH_PER_THREAD; ++k) {
        cnt[k] = base + k < n_cells ? cells[base + k].count : 0u;
        if (cnt[k] >= min_count) ++c;                               // (min_count >= 1: a cell past the end counts nothing)
    }
    int total;
    long long row = tiles[blockIdx.x] + block_scan<DEPTH_BLOCK>(c, lds, &total);
#pragma unroll
    for (int k = 0; k < DEPTH_PER_THREAD; ++k) {
        if (cnt[k] < min_count) continue;
        if (row < capacity) {                                       // (always: capacity was checked against min(G^3, samples))
            const DepthCell *s = cells + base + k;
            for (int a = 0; a < 3; ++a) points[row * 3 + a] = depth_point(s->sum[a], cnt[k], B.v[a], B.v[3]);
            counts[row] = (int32_t)cnt[k];
        }
        ++row;
    }
}

}  // namespace

extern "C" size_t dbw_lens_depth_cloud_workspace_bytes(int G) {
    if (G < 1 || G > DEPTH_MAX_GRID) return 0;
    return depth_layout(G).total;
}

extern "C" int dbw_lens_depth_cloud(const uint16_t *depth, int N, int H, int W, const float *cams, const float *target, const float *poses,
                                    const float *box, int G, int d_min, int d_max, int stride, int edge_permille, int min_count, void *workspace,
                                    float *points, int32_t *counts, int64_t capacity, int64_t *info, dbw_stream_t stream) {
    DBW_REQUIRE(depth && cams && target && poses && box && workspace && points && counts && info, "null pointer");
    DBW_REQUIRE((uintptr_t)workspace % 16 == 0, "workspace is not 16-byte aligned");
    DBW_REQUIRE((uintptr_t)depth % 2 == 0, "depth: misaligned pointer");
    DBW_REQUIRE((uintptr_t)points % 4 == 0 && (uintptr_t)counts % 4 == 0, "points, counts: misaligned pointer");
    DBW_REQUIRE((uintptr_t)info % 8 == 0, "info: misaligned pointer");
    DBW_REQUIRE(N >= 1, "N below 1");
    DBW_REQUIRE(H >= 1 && W >= 1, "H, W below 1");
    DBW_REQUIRE((long long)H * W < (1LL << 29), "H * W must be below 2^29");
    DBW_REQUIRE(G >= 1 && G <= DEPTH_MAX_GRID, "G must be in [1, 256]");
    DBW_REQUIRE(stride >= 1, "stride below 1");
    DBW_REQUIRE(d_max <= 65535, "d_max above 65535");
    DBW_REQUIRE(d_min >= 1 && d_min <= d_max, "d_min must be in [1, d_max]");
    DBW_REQUIRE(edge_permille >= 0 && edge_permille <= 1000, "edge_permille must be in [0, 1000]");
    DBW_REQUIRE(min_count >= 1, "min_count below 1");
    const int Hs = (H + stride - 1) / stride, Ws = (W + stride - 1) / stride;
    const long long samples = (long long)N * Hs * Ws;
    DBW_REQUIRE(samples < (1LL << 31), "N * ceil(H / stride) * ceil(W / stride) must be below 2^31: a cell's count is 32 bits");
    const DepthLayout L = depth_layout(G);
    DBW_REQUIRE(capacity >= (L.n_cells < samples ? L.n_cells : samples), "capacity below min(G^3, N * ceil(H / stride) * ceil(W / stride))");
    for (int k = 0; k < 4; ++k) DBW_REQUIRE(target[k] - target[k] == 0.0f, "target: a value that is not finite");
    DBW_REQUIRE(target[2] > 0.0f && target[3] > 0.0f, "target: a reciprocal focal length that is not positive");
    for (int k = 0; k < 4; ++k) DBW_REQUIRE(box[k] - box[k] == 0.0f, "box: a value that is not finite");
    DBW_REQUIRE(box[3] > 0.0f, "box: inv_step is not positive");
    for (long long n = 0; n < N; ++n) {
        const float *row = cams + n * LENS_RECT_N_PARAMS, *pose = poses + n * DEPTH_POSE_N;
        for (int k = 0; k < LENS_RECT_N_PARAMS; ++k) DBW_REQUIRE(row[k] - row[k] == 0.0f, "cams: a value that is not finite");
        DBW_REQUIRE(row[0] == (float)LENS_RECT_PINHOLE || row[0] == (float)LENS_RECT_FISHEYE, "cams: a model id that is neither 0 nor 1");
        DBW_REQUIRE(row[1] > 0.0f && row[2] > 0.0f, "cams: a focal length that is not positive");
        for (int k = 0; k < DEPTH_POSE_N; ++k) DBW_REQUIRE(pose[k] - pose[k] == 0.0f, "poses: a value that is not finite");
    }
    static_assert(LENS_RECT_N_PARAMS == DBW_LENS_RECT_N_PARAMS, "lens_math.h and dbw_lens.h disagree");
    static_assert(sizeof(DepthArgs) + 3 * sizeof(void *) <= 2096, "the arguments of a launch exceed those of dbw_lens_rectify_u8");

    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    DepthCell *cells = (DepthCell *)ws;
    int *tiles = (int *)(ws + L.tiles);
    unsigned long long *counters = (unsigned long long *)(ws + L.counters);
    const long long n16 = (long long)(L.total / 16);
    const unsigned clear_blocks = (unsigned)(n16 / DEPTH_BLOCK + 1 < 2048 ? n16 / DEPTH_BLOCK + 1 : 2048);
    hipLaunchKernelGGL(depth_clear_kernel, dim3(clear_blocks), dim3(DEPTH_BLOCK), 0, s, (uint4 *)ws, n16);
    if (const int rc = dbw_check_launch("depth_clear_kernel")) return rc;

    DepthArgs A;
    A.Hs = Hs; A.Ws = Ws; A.stride = stride;
    A.rule.H = H; A.rule.W = W; A.rule.G = G; A.rule.d_min = d_min; A.rule.d_max = d_max; A.rule.edge_permille = edge_permille;
    A.pad[0] = A.pad[1] = 0;
    for (int k = 0; k < 4; ++k) { A.target[k] = target[k]; A.box[k] = box[k]; }
    const long long frame = (long long)H * W, px = (long long)Hs * Ws;
    for (int n0 = 0; n0 < N; n0 += DEPTH_GROUP) {
        const int n = N - n0 < DEPTH_GROUP ? N - n0 : DEPTH_GROUP;
        A.n = n;
        for (int f = 0; f < DEPTH_GROUP; ++f) {
            for (int k = 0; k < LENS_RECT_N_PARAMS; ++k) A.cams[f][k] = f < n ? cams[(long long)(n0 + f) * LENS_RECT_N_PARAMS + k] : 0.0f;
            for (int k = 0; k < DEPTH_POSE_N; ++k) A.poses[f][k] = f < n ? poses[(long long)(n0 + f) * DEPTH_POSE_N + k] : 0.0f;
        }
        hipLaunchKernelGGL(depth_accumulate_kernel, dim3((unsigned)((px + DEPTH_BLOCK - 1) / DEPTH_BLOCK), 1, (unsigned)n), dim3(DEPTH_BLOCK), 0, s, A,
                           depth + n0 * frame, cells, counters);
        if (const int rc = dbw_check_launch("depth_accumulate_kernel")) return rc;
    }

    DepthBox B;
    for (int k = 0; k < 4; ++k) B.v[k] = box[k];
    hipLaunchKernelGGL(depth_count_kernel, dim3((unsigned)L.n_tiles), dim3(DEPTH_BLOCK), 0, s, (const DepthCell *)cells, L.n_cells, (uint32_t)min_count, tiles);
    if (const int rc = dbw_check_launch("depth_count_kernel")) return rc;
    hipLaunchKernelGGL(depth_scan_kernel, dim3(1), dim3(DEPTH_SCAN_BLOCK), 0, s, tiles, L.n_tiles, (const unsigned long long *)counters, info);
    if (const int rc = dbw_check_launch("depth_scan_kernel")) return rc;
    hipLaunchKernelGGL(depth_emit_kernel, dim3((unsigned)L.n_tiles), dim3(DEPTH_BLOCK), 0, s, (const DepthCell *)cells, L.n_cells, (uint32_t)min_count,
                       (const int *)tiles, B, points, counts, (long long)capacity);
    return dbw_check_launch("depth_emit_kernel");
}

extern "C" int dbw_lens_depth_rays(const uint16_t *depth, int N, int H, int W, const float *cams, const float *target, const float *poses, int d_min,
                                   int d_max, int stride, int edge_permille, void *rays, dbw_stream_t stream) {
    DBW_REQUIRE(depth && cams && target && poses && rays, "null pointer");
    DBW_REQUIRE((uintptr_t)rays % 16 == 0, "rays are not 16-byte aligned");
    DBW_REQUIRE((uintptr_t)depth % 2 == 0, "depth: misaligned pointer");
    DBW_REQUIRE(N >= 1, "N below 1");
    DBW_REQUIRE(H >= 1 && W >= 1, "H, W below 1");
    DBW_REQUIRE((long long)H * W < (1LL << 29), "H * W must be below 2^29");
    DBW_REQUIRE(stride >= 1, "stride below 1");
    DBW_REQUIRE(d_max <= 65535, "d_max above 65535");
    DBW_REQUIRE(d_min >= 1 && d_min <= d_max, "d_min must be in [1, d_max]");
    DBW_REQUIRE(edge_permille >= 0 && edge_permille <= 1000, "edge_permille must be in [0, 1000]");
    const int Hs = (H + stride - 1) / stride, Ws = (W + stride - 1) / stride;
    DBW_REQUIRE((long long)N * Hs * Ws < (1LL << 31), "N * ceil(H / stride) * ceil(W / stride) must be below 2^31");
    for (int k = 0; k < 4; ++k) DBW_REQUIRE(target[k] - target[k] == 0.0f, "target: a value that is not finite");
    DBW_REQUIRE(target[2] > 0.0f && target[3] > 0.0f, "target: a reciprocal focal length that is not positive");
    for (long long n = 0; n < N; ++n) {
        const float *row = cams + n * LENS_RECT_N_PARAMS, *pose = poses + n * DEPTH_POSE_N;
        for (int k = 0; k < LENS_RECT_N_PARAMS; ++k) DBW_REQUIRE(row[k] - row[k] == 0.0f, "cams: a value that is not finite");
        DBW_REQUIRE(row[0] == (float)LENS_RECT_PINHOLE || row[0] == (float)LENS_RECT_FISHEYE, "cams: a model id that is neither 0 nor 1");
        DBW_REQUIRE(row[1] > 0.0f && row[2] > 0.0f, "cams: a focal length that is not positive");
        for (int k = 0; k < DEPTH_POSE_N; ++k) DBW_REQUIRE(pose[k] - pose[k] == 0.0f, "poses: a value that is not finite");
    }

    hipStream_t s = (hipStream_t)stream;
    DepthArgs A;
    A.Hs = Hs; A.Ws = Ws; A.stride = stride;
    A.rule.H = H; A.rule.W = W; A.rule.G = 1; A.rule.d_min = d_min; A.rule.d_max = d_max; A.rule.edge_permille = edge_permille;
    A.pad[0] = A.pad[1] = 0;
    for (int k = 0; k < 4; ++k) { A.target[k] = target[k]; A.box[k] = 0.0f; }
    const long long frame = (long long)H * W, px = (long long)Hs * Ws;
    for (int n0 = 0; n0 < N; n0 += DEPTH_GROUP) {
        const int n = N - n0 < DEPTH_GROUP ? N - n0 : DEPTH_GROUP;
        A.n = n;
        for (int f = 0; f < DEPTH_GROUP; ++f) {
            for (int k = 0; k < LENS_RECT_N_PARAMS; ++k) A.cams[f][k] = f < n ? cams[(long long)(n0 + f) * LENS_RECT_N_PARAMS + k] : 0.0f;
            for (int k = 0; k < DEPTH_POSE_N; ++k) A.poses[f][k] = f < n ? poses[(long long)(n0 + f) * DEPTH_POSE_N + k] : 0.0f;
        }
        hipLaunchKernelGGL(depth_rays_kernel, dim3((unsigned)((px + DEPTH_BLOCK - 1) / DEPTH_BLOCK), 1, (unsigned)n), dim3(DEPTH_BLOCK), 0, s, A, n0,
                           depth + n0 * frame, (float4 *)rays + n0 * px);
        if (const int rc = dbw_check_launch("depth_rays_kernel")) return rc;
    }
    return 0;
}
