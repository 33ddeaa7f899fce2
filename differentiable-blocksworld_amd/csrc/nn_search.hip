// 3D evaluation kernels (include/dbw_eval.h): exact batched 1-nearest neighbour, the DTU dense triangle lattice, one round of the greedy
// radius downsample.  The arithmetic is csrc/nn_math.h (also built by g++ for the host tests).
//
// Nearest neighbour.  A workgroup of 256 lanes owns 256 * NN_Q queries (NN_Q per lane, in registers, as float2 pairs so that the
// subtractions, products and sums issue as packed fp32 instructions: v_pk_add_f32 / v_pk_mul_f32, two pairs per instruction, the same
// IEEE result as the scalar expression).  The y points of the workgroup's range come through LDS in tiles of NN_TILE and are read as
// broadcasts.  The search itself tracks only the minimum distance of every sub-chunk of NN_CH y points (one v_min per pair); a query
// remembers the first sub-chunk whose minimum beats its best, and after the scan looks for the lowest index of that sub-chunk whose
// distance equals the best: the same (dist2, idx) as a strict `<` scan, at ~5 instead of ~7 VALU per pair.  When the y range is split
// across workgroups, each writes its candidate with a 64-bit atomic min on (dist2 bits << 32 | idx): dist2 >= 0, so the key orders like
// (dist2, idx) and the merge is exact and independent of the order of arrival.
#include "dbw_common.h"
#include "nn_math.h"
#include "nn_search.h"
#include "../../include/dbw_eval.h"

#include <math.h>

namespace {

constexpr int NN_BLOCK = 256;
constexpr int NN_Q = 8;                 // queries per lane
constexpr int NN_TILE = 512;            // y points per LDS tile
constexpr int NN_CH = 64;               // y points per tracked sub-chunk
typedef float pf2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(NN_BLOCK) void nn_search_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                             const int64_t *__restrict__ xl, const int64_t *__restrict__ yl, int P1,
                                                             int P2, int chunk, int merge, unsigned long long *__restrict__ keys) {
    __shared__ float4 sy[NN_TILE];
    const int n = blockIdx.z;
    const long long lx = xl ? (xl[n] < 0 ? 0 : (xl[n] > P1 ? P1 : xl[n])) : P1;
    const long long ly = yl ? (yl[n] < 0 ? 0 : (yl[n] > P2 ? P2 : yl[n])) : P2;
    const int q0 = blockIdx.x * (NN_BLOCK * NN_Q);
    const long long y0 = (long long)blockIdx.y * chunk, y1 = y0 + chunk < ly ? y0 + chunk : ly;
    if (q0 >= lx || y0 >= y1) return;                            // (uniform over the workgroup)
    const float *xb = x + (long long)n * P1 * 3;
    const float *yb = y + (long long)n * P2 * 3;
    pf2 qx[NN_Q / 2], qy[NN_Q / 2], qz[NN_Q / 2], best[NN_Q / 2];
    int bch[NN_Q];
#pragma unroll
    for (int k = 0; k < NN_Q; ++k) {
        const int q = q0 + k * NN_BLOCK + threadIdx.x;
        const bool ok = q < lx;
        qx[k / 2][k % 2] = ok ? xb[(long long)q * 3 + 0] : 0.f;
        qy[k / 2][k % 2] = ok ? xb[(long long)q * 3 + 1] : 0.f;
        qz[k / 2][k % 2] = ok ? xb[(long long)q * 3 + 2] : 0.f;
        best[k / 2][k % 2] = INFINITY;
        bch[k] = (int)y0;
    }
    for (long long t0 = y0; t0 < y1; t0 += NN_TILE) {
        const int cnt = (int)(y1 - t0 < NN_TILE ? y1 - t0 : NN_TILE);
        __syncthreads();
        for (int j = threadIdx.x; j < cnt; j += NN_BLOCK) {
            const float *p = yb + (t0 + j) * 3;
            sy[j] = make_float4(p[0], p[1], p[2], 0.f);
        }
        __syncthreads();
        for (int c0 = 0; c0 < cnt; c0 += NN_CH) {
            const int ce = c0 + NN_CH < cnt ? c0 + NN_CH : cnt;
            pf2 m[NN_Q / 2];
#pragma unroll
            for (int h = 0; h < NN_Q / 2; ++h) m[h] = (pf2)(INFINITY);
#pragma unroll 4
            for (int j = c0; j < ce; ++j) {
                const float4 p = sy[j];
#pragma unroll
                for (int h = 0; h < NN_Q / 2; ++h) {
                    const pf2 d = dbw::nn_dist2(qx[h], qy[h], qz[h], (pf2)(p.x), (pf2)(p.y), (pf2)(p.z));
                    m[h].x = __builtin_fminf(m[h].x, d.x);
                    m[h].y = __builtin_fminf(m[h].y, d.y);
                }
            }
#pragma unroll
            for (int k = 0; k < NN_Q; ++k)
                if (m[k / 2][k % 2] < best[k / 2][k % 2]) { best[k / 2][k % 2] = m[k / 2][k % 2]; bch[k] = (int)(t0 + c0); }
        }
    }
    // the lowest index of the winning sub-chunk at the best distance (same expression, so the same bits)
#pragma unroll
    for (int k = 0; k < NN_Q; ++k) {
        const int q = q0 + k * NN_BLOCK + threadIdx.x;
        if (q >= lx) continue;
        const float b = best[k / 2][k % 2];
        const long long e = bch[k] + NN_CH < y1 ? bch[k] + NN_CH : y1;
        int bi = bch[k];
        for (long long j = bch[k]; j < e; ++j) {
            const float *p = yb + j * 3;
            if (dbw::nn_dist2(qx[k / 2][k % 2], qy[k / 2][k % 2], qz[k / 2][k % 2], p[0], p[1], p[2]) == b) { bi = (int)j; break; }
        }
        unsigned long long *dst = keys + (long long)n * P1 + q;
        const unsigned long long key = dbw::nn_key(b, (uint32_t)bi);
        if (merge)
            atomicMin(dst, key);
        else
            *dst = key;
    }
}

__global__ void nn_finalize_kernel(const unsigned long long *__restrict__ keys, const int64_t *__restrict__ xl, int N, int P1,
                                   float *__restrict__ dist2, int64_t *__restrict__ idx) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)N * P1) return;
    const int n = (int)(t / P1), q = (int)(t % P1);
    const long long lx = xl ? xl[n] : P1;
    const unsigned long long k = keys[t];
    if (q >= lx) {
        dist2[t] = 0.f; idx[t] = -1;
    } else if (k == ~0ull) {
        dist2[t] = INFINITY; idx[t] = -1;
    } else {
        dist2[t] = dbw::u2f((uint32_t)(k >> 32));
        idx[t] = (int64_t)(uint32_t)(k & 0xffffffffull);
    }
}

__global__ void lattice_count_kernel(const double *__restrict__ tri, long long F, int64_t *__restrict__ counts) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f < F) counts[f] = dbw::lattice_count(tri + f * 9);
}

__global__ void lattice_points_kernel(const double *__restrict__ tri, long long F, const int64_t *__restrict__ counts,
                                      const int64_t *__restrict__ offsets, long long n_out, double *__restrict__ points) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const long long o = offsets[f], c = counts[f];
    if (o < 0 || c < 0 || o + c > n_out) return;
    dbw::lattice_emit(tri + f * 9, points + o * 3, c);
}

__device__ __forceinline__ long long lower_bound_keys(const int64_t *keys, long long n, long long v) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void radius_round_kernel(const double *__restrict__ pts, const int64_t *__restrict__ keys, const int64_t *__restrict__ rank,
                                    long long n, long long ny, long long nz, double r2, const int32_t *__restrict__ st_in,
                                    int32_t *__restrict__ st_out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t s = st_in[i];
    if (s != 0) { st_out[i] = s; return; }
    const long long ri = rank[i], key = keys[i], nyz = ny * nz;
    const long long cx = key / nyz, cy = (key % nyz) / nz, cz = key % nz;
    const double *p = pts + i * 3;
    bool kept_nb = false, open_nb = false;
    for (int dx = -1; dx <= 1 && !kept_nb; ++dx)
        for (int dy = -1; dy <= 1 && !kept_nb; ++dy) {
            // cells (cx+dx, cy+dy, cz-1 .. cz+1) are consecutive keys, so their points are one run of the sorted array
            const long long klo = ((cx + dx) * ny + (cy + dy)) * nz + cz - 1, khi = klo + 2;
            for (long long j = lower_bound_keys(keys, n, klo); j < n && keys[j] <= khi; ++j) {
                if (rank[j] >= ri) continue;                         // later in the order (or the point itself)
                const int32_t sj = st_in[j];
                if (sj == 2 || !dbw::within_radius(p, pts + j * 3, r2)) continue;
                if (sj == 1) { kept_nb = true; break; }
                open_nb = true;
            }
        }
    st_out[i] = kept_nb ? 2 : (open_nb ? 0 : 1);
}

}  // namespace

extern "C" int dbw_eval_abi_version(void) { return DBW_EVAL_ABI_VERSION; }      // (history: include/dbw_eval.h)

int dbw_nn_search_plan(const char *caller, int N, int P1, int P2, int splits) {
    const long long bx = (P1 + NN_BLOCK * NN_Q - 1) / (NN_BLOCK * NN_Q);
    if (splits == 0) {
        // at most as many workgroups as the chip holds at once (CUs x resident workgroups per CU): one round, no partial second one;
        // at least 4096 y points per workgroup.  (500k x 500k: 245 x 5 workgroups, 35.4 ms; 245 x 9 = two rounds: 34.7 ms, the same)
        static thread_local long long slots = 0;
        if (slots == 0) {
            int dev = 0, cus = 0, per_cu = 0;
            if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
                hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, nn_search_kernel, NN_BLOCK, 0) != hipSuccess || cus <= 0 || per_cu <= 0) {
                cus = 256;
                per_cu = 4;
            }
            slots = (long long)cus * per_cu;
        }
        const long long want = slots / (bx * N), most = (P2 + 4095) / 4096;
        splits = (int)(want < most ? want : most);
        if (splits < 1) splits = 1;
    }
    if (splits > P2) splits = P2;
    if (!(bx * splits < (1ll << 31) && N < 65536 && splits < 65536)) {      // (DBW_REQUIRE's text, under the entry point's name)
        dbw_set_error("%s: %s", caller, "grid too large");
        return DBW_ERR_INVALID;
    }
    return splits;
}

int dbw_nn_search_launch(const float *x, const float *y, const int64_t *x_lengths, const int64_t *y_lengths, int N, int P1, int P2,
                         int splits, void *keys, hipStream_t st) {
    const long long bx = (P1 + NN_BLOCK * NN_Q - 1) / (NN_BLOCK * NN_Q);
    const int chunk = (int)((P2 + splits - 1) / splits);
    if (hipMemsetAsync(keys, 0xff, (size_t)N * P1 * sizeof(unsigned long long), st) != hipSuccess) {
        dbw_set_error("nearest-neighbour search: hipMemsetAsync failed");
        return DBW_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(nn_search_kernel, dim3((unsigned)bx, (unsigned)splits, (unsigned)N), dim3(NN_BLOCK), 0, st, x, y, x_lengths,
                       y_lengths, P1, P2, chunk, splits > 1 ? 1 : 0, (unsigned long long *)keys);
    return dbw_check_launch("nn_search_kernel");
}

extern "C" int dbw_nn_points(const float *x, const float *y, const int64_t *x_lengths, const int64_t *y_lengths, int N, int P1, int P2,
                             int splits, void *keys, float *dist2, int64_t *idx, dbw_stream_t stream) {
    DBW_REQUIRE(x && y && keys && dist2 && idx, "null pointer");
    DBW_REQUIRE(N > 0 && P1 > 0 && P2 > 0 && splits >= 0, "bad size");
    DBW_REQUIRE((long long)N * P1 < (1ll << 40) && (long long)P1 * 3 < (1ll << 40), "too large");
    const hipStream_t st = (hipStream_t)stream;
    splits = dbw_nn_search_plan(__func__, N, P1, P2, splits);
    if (splits < 0) return splits;
    int rc = dbw_nn_search_launch(x, y, x_lengths, y_lengths, N, P1, P2, splits, keys, st);
    if (rc) return rc;
    const long long tot = (long long)N * P1;
    hipLaunchKernelGGL(nn_finalize_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const unsigned long long *)keys,
                       x_lengths, N, P1, dist2, idx);
    return dbw_check_launch("nn_finalize_kernel");
}

extern "C" int dbw_dtu_lattice_counts(const double *tri, int64_t F, int64_t *counts, dbw_stream_t stream) {
    DBW_REQUIRE(tri && counts, "null pointer");
    DBW_REQUIRE(F > 0 && F < (1ll << 36), "bad size");
    hipLaunchKernelGGL(lattice_count_kernel, dim3((unsigned)((F + 127) / 128)), dim3(128), 0, (hipStream_t)stream, tri, (long long)F, counts);
    return dbw_check_launch("lattice_count_kernel");
}

extern "C" int dbw_dtu_lattice_points(const double *tri, int64_t F, const int64_t *counts, const int64_t *offsets, int64_t n_out,
                                      double *points, dbw_stream_t stream) {
    DBW_REQUIRE(tri && counts && offsets && points, "null pointer");
    DBW_REQUIRE(F > 0 && F < (1ll << 36) && n_out >= 0, "bad size");
    hipLaunchKernelGGL(lattice_points_kernel, dim3((unsigned)((F + 127) / 128)), dim3(128), 0, (hipStream_t)stream, tri, (long long)F,
                       counts, offsets, (long long)n_out, points);
    return dbw_check_launch("lattice_points_kernel");
}

extern "C" int dbw_radius_downsample_round(const double *points, const int64_t *cell_keys, const int64_t *rank, int64_t n, int64_t ny,
                                           int64_t nz, double radius, const int32_t *status_in, int32_t *status_out, dbw_stream_t stream) {
    DBW_REQUIRE(points && cell_keys && rank && status_in && status_out, "null pointer");
    DBW_REQUIRE(n > 0 && n < (1ll << 40) && ny >= 3 && nz >= 3 && radius > 0.0, "bad size");
    DBW_REQUIRE(status_in != status_out, "status_in and status_out must differ");
    hipLaunchKernelGGL(radius_round_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points, cell_keys, rank,
                       (long long)n, (long long)ny, (long long)nz, radius * radius, status_in, status_out);
    return dbw_check_launch("radius_round_kernel");
}
