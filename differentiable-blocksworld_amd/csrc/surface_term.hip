// The surface term behind two calls (include/dbw_eval.h: dbw_eval_surface_fwd / _bwd): the truncated squared distance of drawn cloud points
// to the posed meshes, and of the block vertices to the cloud.  The arithmetic is csrc/surface_math.h (also built by g++ for the host
// tests); this file is the schedule.  No MFMA, no floating-point atomics, no cross-workgroup waiting: plain launches on the caller's
// stream, kernel boundaries the only ordering, nothing read by the host.
//
// Forward launches
//   surface_box_kernel    one workgroup per group (ground, block 0, block 1, ...): the 9 coordinates of each of its faces gathered into the
//                         workspace (12 floats a face: three 16-byte scalar loads later) and the group's axis-aligned box.  A face index
//                         outside [0, V) is read as vertex 0: no launch reads outside `verts`, whatever `faces` holds.
//   surface_fwd_kernel    one point per lane, drawn in the kernel (surface_draw_index).  The groups are walked in order; group and face are
//                         wave-uniform, so box and face coordinates arrive by scalar loads and every lane runs surface_closest on them.  A
//                         group is skipped when it is not kept or (cull) when EVERY lane's box bound is strictly above its running best d2:
//                         the bound is never above a d2 that the group could give, so a skipped group holds no key below any lane's best and
//                         the records do not depend on `cull`.  One 16-byte record a point; the workgroup's sum of rho in fp64 through
//                         block_sum, one partial a workgroup.
//   nn search             (back > 0) the exact nearest cloud point of every vertex: dbw_nn_search_launch, 64-bit keys
//   surface_back_kernel   (back > 0) rho of every block vertex, a_k * rho summed like the forward's
//   partials_finish       twice: value[0] = sum rho / M, value[1] = sum a rho / back_count
//
// Backward launches
//   surface_bwd_kernel    grid (segment, 256 vertices): a workgroup walks its segment of the records in index order, the record uniform across
//                         the workgroup; a thread whose vertex is a corner of the record's face adds -2 b_m (p - c) to its own fp64 sum.  A
//                         wave none of whose vertices is a corner does no arithmetic for the record.  Partials [segment][V][3].
//   surface_bwd_finish    one thread per vertex: the segments' partials added in segment order, the back direction's 2 a_k (x_v - nn) added,
//                         scaled, rounded to fp32
//   surface_alpha_kernel  one workgroup per opacity: the rho of its vertices added in a fixed order (thread t takes t, t + 256, ...; block_sum)
// The grids depend on the sizes alone and every sum has one order: the same call gives the same bytes.
#include "dbw_common.h"
#include "loss_reduce.h"
#include "nn_search.h"
#include "surface_box.h"
#include "surface_math.h"
#include "../../include/dbw_eval.h"

#include <math.h>

namespace {

constexpr int SF_BLOCK = dbw::LOSS_THREADS;
constexpr int SF_TRI = 12;                      // floats a gathered face takes
constexpr int SF_MAX_G = 4096, SF_MAX_F = 1 << 20, SF_MAX_V = 1 << 21, SF_MAX_M = 1 << 24, SF_MAX_SEGS = 65535;
static_assert(DBW_EVAL_SURFACE_SEGMENT == dbw::SURFACE_SEGMENT, "the header mirrors the segment length of surface_math.h");

struct SurfaceLayout {          // byte offsets into the workspace
    size_t boxes, tri, fwd_part, keys, back_part, rho_back, bwd_part, total;
    int fwd_groups, vert_groups, segs;
};

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

inline bool surface_sizes_ok(int64_t M, int F, int V, int G, int segment) {
    if (!(M >= 1 && M <= SF_MAX_M && F >= 1 && F <= SF_MAX_F && V >= 1 && V <= SF_MAX_V && G >= 1 && G <= SF_MAX_G)) return false;
    if (segment < 0) return false;
    const int64_t L = segment ? segment : dbw::SURFACE_SEGMENT;
    return (M + L - 1) / L <= SF_MAX_SEGS;
}

inline SurfaceLayout surface_layout(int64_t M, int F, int V, int G, int segment) {
    SurfaceLayout L;
    const int64_t seg = segment ? segment : dbw::SURFACE_SEGMENT;
    L.fwd_groups = (int)((M + SF_BLOCK - 1) / SF_BLOCK);
    L.vert_groups = (V + SF_BLOCK - 1) / SF_BLOCK;
    L.segs = (int)((M + seg - 1) / seg);
    size_t o = 0;
    L.boxes = o; o = align16(o + (size_t)G * 8 * sizeof(float));
    L.tri = o; o = align16(o + (size_t)F * SF_TRI * sizeof(float));
    L.fwd_part = o; o = align16(o + (size_t)L.fwd_groups * sizeof(double));
    L.keys = o; o = align16(o + (size_t)V * sizeof(unsigned long long));
    L.back_part = o; o = align16(o + (size_t)L.vert_groups * sizeof(double));
    L.rho_back = o; o = align16(o + (size_t)V * sizeof(float));
    L.bwd_part = o; o = align16(o + (size_t)L.segs * V * 3 * sizeof(double));
    L.total = o;
    return L;
}

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

__global__ __launch_bounds__(SF_BLOCK) void surface_box_kernel(const float *__restrict__ verts, int V, const int32_t *__restrict__ faces, int F,
                                                               const int32_t *__restrict__ face_group, const int32_t *__restrict__ group_keep,
                                                               float *__restrict__ tri, float *__restrict__ boxes) {
    __shared__ float sh[SF_BLOCK / DBW_WAVE][6];
    const int g = blockIdx.x;
    const int f0 = clampi(face_group[g], 0, F), f1 = clampi(face_group[g + 1], 0, F);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (!group_keep || group_keep[g]) {
        for (int f = f0 + (int)threadIdx.x; f < f1; f += SF_BLOCK) {
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                int i = faces[f * 3 + m];
                i = (i >= 0 && i < V) ? i : 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float x = verts[(size_t)i * 3 + k];
                    tri[(size_t)f * SF_TRI + m * 3 + k] = x;
                    lo[k] = x < lo[k] ? x : lo[k];
                    hi[k] = x > hi[k] ? x : hi[k];
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float a = __shfl_xor(lo[k], o, DBW_WAVE), b = __shfl_xor(hi[k], o, DBW_WAVE);
            lo[k] = a < lo[k] ? a : lo[k];
            hi[k] = b > hi[k] ? b : hi[k];
        }
    }
    const int lane = threadIdx.x & (DBW_WAVE - 1), wave = threadIdx.x / DBW_WAVE;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { sh[wave][k] = lo[k]; sh[wave][3 + k] = hi[k]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        float a = sh[0][threadIdx.x], b = sh[0][3 + threadIdx.x];
        for (int w = 1; w < SF_BLOCK / DBW_WAVE; ++w) {
            a = sh[w][threadIdx.x] < a ? sh[w][threadIdx.x] : a;
            b = sh[w][3 + threadIdx.x] > b ? sh[w][3 + threadIdx.x] : b;
        }
        boxes[g * 8 + threadIdx.x] = a;
        boxes[g * 8 + 4 + threadIdx.x] = b;
    }
}

// the cloud point of draw i
__device__ __forceinline__ void surface_point(const float *__restrict__ points, uint32_t N, int draw, uint64_t seed, uint64_t step, uint32_t i,
                                              float &x, float &y, float &z) {
    const size_t j = draw ? dbw::surface_draw_index(seed, step, i, N) : i;
    x = points[j * 3]; y = points[j * 3 + 1]; z = points[j * 3 + 2];
}

__global__ __launch_bounds__(SF_BLOCK) void surface_fwd_kernel(const float *__restrict__ points, uint32_t N, int M, int draw, uint64_t seed,
                                                               uint64_t step, const float *__restrict__ tri, const float *__restrict__ boxes,
                                                               const int32_t *__restrict__ face_group, const int32_t *__restrict__ group_keep,
                                                               int F, int G, float tau2, int cull, float4 *__restrict__ records,
                                                               double *__restrict__ partial) {
    __shared__ double red[dbw::LOSS_WAVES][1];
    const int i = blockIdx.x * SF_BLOCK + threadIdx.x;
    const bool live = i < M;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (live) surface_point(points, N, draw, seed, step, (uint32_t)i, px, py, pz);
    unsigned long long best = ~0ull;
    float best_d2 = INFINITY, bu = 0.f, bv = 0.f;
    for (int g = 0; g < G; ++g) {
        if (group_keep && !group_keep[g]) continue;
        if (cull) {
            const float *b = boxes + g * 8;
            const float lo[3] = {b[0], b[1], b[2]}, hi[3] = {b[4], b[5], b[6]};
            const bool want = live && !(dbw::surface_box_bound(lo, hi, px, py, pz) > best_d2);
            if (__ballot(want) == 0ull) continue;
        }
        const int f0 = clampi(face_group[g], 0, F), f1 = clampi(face_group[g + 1], 0, F);
#pragma unroll 2
        for (int f = f0; f < f1; ++f) {
            const float *t = tri + (size_t)f * SF_TRI;              // wave-uniform address: scalar loads
            const float tt[9] = {t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]};
            const dbw::SurfaceHit h = dbw::surface_closest(tt, px, py, pz);
            const unsigned long long key = dbw::surface_key(h.d2, (uint32_t)f);
            if (key < best) { best = key; best_d2 = h.d2; bu = h.u; bv = h.v; }
        }
    }
    double s = 0.0;
    if (live) {
        const float d2 = dbw::surface_key_d2(best);
        records[i] = make_float4(d2, __int_as_float((int)(uint32_t)(best & 0xffffffffull)), bu, bv);
        s = (double)dbw::surface_rho(d2, tau2);
    }
    const double tsum = dbw::block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tsum;
}

__global__ __launch_bounds__(SF_BLOCK) void surface_back_kernel(const unsigned long long *__restrict__ keys, int V,
                                                                const float *__restrict__ vert_alpha, const int32_t *__restrict__ vert_group,
                                                                int A, float tau2, float *__restrict__ rho_back, double *__restrict__ partial) {
    __shared__ double red[dbw::LOSS_WAVES][1];
    const int v = blockIdx.x * SF_BLOCK + threadIdx.x;
    double s = 0.0;
    if (v < V) {
        const int k = vert_group[v];
        float rho = 0.f;
        if (k >= 0 && k < A) {
            rho = dbw::surface_rho(dbw::surface_key_d2(keys[v]), tau2);
            s = (double)vert_alpha[k] * (double)rho;
        }
        rho_back[v] = rho;
    }
    const double tsum = dbw::block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tsum;
}

__global__ __launch_bounds__(SF_BLOCK) void surface_bwd_kernel(const float *__restrict__ points, uint32_t N, int M, int draw, uint64_t seed,
                                                               uint64_t step, const float4 *__restrict__ records, const float *__restrict__ tri,
                                                               const int32_t *__restrict__ faces, int F, int V, int seg_len, float tau2,
                                                               double *__restrict__ part) {
    const int v = blockIdx.y * SF_BLOCK + threadIdx.x;
    const long long r0 = (long long)blockIdx.x * seg_len;
    const int r1 = (int)(r0 + seg_len < M ? r0 + seg_len : M);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int r = (int)r0; r < r1; ++r) {
        const float4 rec = records[r];                              // uniform across the workgroup
        if (!(rec.x < tau2)) continue;
        const int f = __float_as_int(rec.y);
        if (f < 0 || f >= F) continue;
        const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
        const bool m0 = v == i0, m1 = v == i1, m2 = v == i2;
        if (__ballot(m0 || m1 || m2) == 0ull) continue;
        float px, py, pz;
        surface_point(points, N, draw, seed, step, (uint32_t)r, px, py, pz);
        const float *t = tri + (size_t)f * SF_TRI;
        const float e1[3] = {t[3] - t[0], t[4] - t[1], t[5] - t[2]}, e2[3] = {t[6] - t[0], t[7] - t[1], t[8] - t[2]};
        const float q[3] = {px - t[0], py - t[1], pz - t[2]};
        const double coef = (m0 ? (double)((1.f - rec.z) - rec.w) : 0.0) + (m1 ? (double)rec.z : 0.0) + (m2 ? (double)rec.w : 0.0);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float d = q[k] - (rec.z * e1[k] + rec.w * e2[k]);                 // p - c, the forward's own operations
            acc[k] -= 2.0 * coef * (double)d;
        }
    }
    if (v < V) {
        double *o = part + ((size_t)blockIdx.x * V + v) * 3;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
    }
}

// scale_fwd = weight / M, scale_back = weight * back / back_count; both times grad_out[0] (1 without one)
__global__ __launch_bounds__(SF_BLOCK) void surface_bwd_finish_kernel(const double *__restrict__ part, int segs, int V, const float *__restrict__ verts,
                                                                      const float *__restrict__ points, const unsigned long long *__restrict__ keys,
                                                                      const float *__restrict__ vert_alpha, const int32_t *__restrict__ vert_group,
                                                                      int A, uint32_t N, float tau2, double scale_fwd, double scale_back,
                                                                      const float *__restrict__ grad_out, float *__restrict__ grad_verts) {
    const int v = blockIdx.x * SF_BLOCK + threadIdx.x;
    if (v >= V) return;
    const double go = grad_out ? (double)grad_out[0] : 1.0;
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < segs; ++b) {
        const double *p = part + ((size_t)b * V + v) * 3;
        s[0] += p[0]; s[1] += p[1]; s[2] += p[2];
    }
    double gb[3] = {0.0, 0.0, 0.0};
    if (keys) {
        const int k = vert_group[v];
        if (k >= 0 && k < A) {
            const unsigned long long key = keys[v];
            if (dbw::surface_key_d2(key) < tau2 && (uint32_t)(key & 0xffffffffull) < N) {
                const size_t j = (size_t)(key & 0xffffffffull);
                const double a = (double)vert_alpha[k];
#pragma unroll
                for (int c = 0; c < 3; ++c) gb[c] = 2.0 * a * (double)(verts[(size_t)v * 3 + c] - points[j * 3 + c]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) grad_verts[(size_t)v * 3 + c] = (float)((s[c] * scale_fwd + gb[c] * scale_back) * go);
}

__global__ __launch_bounds__(SF_BLOCK) void surface_alpha_kernel(const float *__restrict__ rho_back, const int32_t *__restrict__ vert_group, int V,
                                                                 double scale_back, const float *__restrict__ grad_out,
                                                                 float *__restrict__ grad_alpha) {
    __shared__ double red[dbw::LOSS_WAVES][1];
    const int k = blockIdx.x;
    double s = 0.0;
    if (rho_back) {
        for (int v = threadIdx.x; v < V; v += SF_BLOCK) s += vert_group[v] == k ? (double)rho_back[v] : 0.0;
    }
    const double t = dbw::block_sum(s, red);
    if (threadIdx.x == 0) grad_alpha[k] = (float)(t * scale_back * (grad_out ? (double)grad_out[0] : 1.0));
}

}  // namespace

// the box launch for the other term that walks the same gathered faces (csrc/freespace_term.hip): tri (F, 12 floats), boxes (G, 8 floats)
int dbw_surface_box_launch(const float *verts, int V, const int32_t *faces, int F, const int32_t *face_group, const int32_t *group_keep, int G,
                           float *tri, float *boxes, hipStream_t stream) {
    hipLaunchKernelGGL(surface_box_kernel, dim3((unsigned)G), dim3(SF_BLOCK), 0, stream, verts, V, faces, F, face_group, group_keep, tri, boxes);
    return dbw_check_launch("surface_box_kernel");
}

extern "C" size_t dbw_eval_surface_workspace_bytes(int64_t M, int F, int V, int G, int segment) {
    return surface_sizes_ok(M, F, V, G, segment) ? surface_layout(M, F, V, G, segment).total : 0;
}

#define SURFACE_COMMON_CHECKS                                                                                                              \
    DBW_REQUIRE(N >= 1 && N < (1ll << 31), "N must be in [1, 2^31)");                                                                      \
    DBW_REQUIRE(n_points >= 0 && n_points <= SF_MAX_M && (n_points > 0 || N <= SF_MAX_M), "the points of a step (n_points, or N when it is 0) must be in [1, 2^24]"); \
    DBW_REQUIRE(F >= 1 && F <= SF_MAX_F, "F must be in [1, 2^20]");                                                                        \
    DBW_REQUIRE(V >= 1 && V <= SF_MAX_V, "V must be in [1, 2^21]");                                                                        \
    DBW_REQUIRE(G >= 1 && G <= SF_MAX_G, "G must be in [1, 4096]");                                                                        \
    DBW_REQUIRE(tau > 0.f && tau < INFINITY, "tau must be positive and finite");                                                           \
    DBW_REQUIRE(back >= 0.f && back < INFINITY, "back must be non-negative and finite");                                                   \
    DBW_REQUIRE(back == 0.f || (vert_alpha && vert_group), "back > 0 needs vert_alpha and vert_group");                                    \
    DBW_REQUIRE(A >= 0 && A <= V, "A must be in [0, V]");                                                                                  \
    DBW_REQUIRE(back == 0.f || (A >= 1 && back_count > 0.0), "back > 0 needs A >= 1 and a positive back_count");                           \
    DBW_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace is not 16-byte aligned");                                                     \
    DBW_REQUIRE(((uintptr_t)records & 15) == 0, "records are not 16-byte aligned")

extern "C" int dbw_eval_surface_fwd(const float *points, int64_t N, int64_t n_points, int64_t seed, int64_t step, const float *verts, int V,
                                    const int32_t *faces, const int32_t *faces_host, int F, const int32_t *face_group, const int32_t *group_keep, int G,
                                    const float *vert_alpha, const int32_t *vert_group, int A, double back_count, float tau, float back, int cull,
                                    void *workspace, void *records, double *value, dbw_stream_t stream) {
    DBW_REQUIRE(points && verts && faces && face_group && workspace && records && value, "null pointer");
    SURFACE_COMMON_CHECKS;
    DBW_REQUIRE(cull == 0 || cull == 1, "cull must be 0 or 1");
    DBW_REQUIRE(((uintptr_t)points & 3) == 0 && ((uintptr_t)verts & 3) == 0 && ((uintptr_t)faces & 3) == 0 && ((uintptr_t)faces_host & 3) == 0 &&
                    ((uintptr_t)face_group & 3) == 0 && ((uintptr_t)group_keep & 3) == 0 && ((uintptr_t)vert_alpha & 3) == 0 &&
                    ((uintptr_t)vert_group & 3) == 0 && ((uintptr_t)value & 7) == 0,
                "misaligned pointer");
    if (faces_host) {
        for (int64_t k = 0; k < (int64_t)F * 3; ++k) DBW_REQUIRE(faces_host[k] >= 0 && faces_host[k] < V, "a face index is outside [0, V)");
    }
    const int64_t M = n_points ? n_points : N;
    const int draw = n_points ? 1 : 0;
    int splits = 0;
    if (back > 0.f) {
        splits = dbw_nn_search_plan(__func__, 1, V, (int)N, 0);
        if (splits < 0) return splits;
    }
    const hipStream_t st = (hipStream_t)stream;
    const SurfaceLayout L = surface_layout(M, F, V, G, 0);      // (the backward's partials come last: the offsets before them do not depend on the segment)
    char *ws = (char *)workspace;
    float *boxes = (float *)(ws + L.boxes), *tri = (float *)(ws + L.tri), *rho_back = (float *)(ws + L.rho_back);
    double *fwd_part = (double *)(ws + L.fwd_part), *back_part = (double *)(ws + L.back_part);
    const float tau2 = tau * tau;

    hipLaunchKernelGGL(surface_box_kernel, dim3((unsigned)G), dim3(SF_BLOCK), 0, st, verts, V, faces, F, face_group, group_keep, tri, boxes);
    int rc = dbw_check_launch("surface_box_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(surface_fwd_kernel, dim3((unsigned)L.fwd_groups), dim3(SF_BLOCK), 0, st, points, (uint32_t)N, (int)M, draw, (uint64_t)seed,
                       (uint64_t)step, (const float *)tri, (const float *)boxes, face_group, group_keep, F, G, tau2, cull, (float4 *)records, fwd_part);
    if ((rc = dbw_check_launch("surface_fwd_kernel"))) return rc;
    if ((rc = dbw::partials_finish(fwd_part, L.fwd_groups, 1.0, (double)M, value, st))) return rc;
    if (back > 0.f) {
        if ((rc = dbw_nn_search_launch(verts, points, nullptr, nullptr, 1, V, (int)N, splits, ws + L.keys, st))) return rc;
        hipLaunchKernelGGL(surface_back_kernel, dim3((unsigned)L.vert_groups), dim3(SF_BLOCK), 0, st, (const unsigned long long *)(ws + L.keys), V,
                           vert_alpha, vert_group, A, tau2, rho_back, back_part);
        if ((rc = dbw_check_launch("surface_back_kernel"))) return rc;
    }
    return dbw::partials_finish(back_part, back > 0.f ? L.vert_groups : 0, 1.0, back > 0.f ? back_count : 1.0, value + 1, st);
}

extern "C" int dbw_eval_surface_bwd(const float *points, int64_t N, int64_t n_points, int64_t seed, int64_t step, const float *verts, int V,
                                    const int32_t *faces, int F, int G, const float *vert_alpha, const int32_t *vert_group, int A, double back_count,
                                    float tau, float back, float weight, const float *grad_out, int segment, const void *records, void *workspace,
                                    float *grad_verts, float *grad_alpha, dbw_stream_t stream) {
    DBW_REQUIRE(points && verts && faces && workspace && records && grad_verts, "null pointer");
    SURFACE_COMMON_CHECKS;
    DBW_REQUIRE(back == 0.f || grad_alpha, "back > 0 needs grad_alpha");
    DBW_REQUIRE(weight == weight && fabsf(weight) < INFINITY, "weight must be finite");
    DBW_REQUIRE(segment == 0 || (segment >= 64 && segment <= (1 << 20)), "segment must be 0 or in [64, 2^20]");
    DBW_REQUIRE(((uintptr_t)points & 3) == 0 && ((uintptr_t)verts & 3) == 0 && ((uintptr_t)faces & 3) == 0 && ((uintptr_t)vert_alpha & 3) == 0 &&
                    ((uintptr_t)vert_group & 3) == 0 && ((uintptr_t)grad_out & 3) == 0 && ((uintptr_t)grad_verts & 3) == 0 &&
                    ((uintptr_t)grad_alpha & 3) == 0,
                "misaligned pointer");
    const int64_t M = n_points ? n_points : N;
    DBW_REQUIRE(surface_sizes_ok(M, F, V, G, segment), "too many segments: raise segment");
    const hipStream_t st = (hipStream_t)stream;
    const SurfaceLayout L = surface_layout(M, F, V, G, segment);
    const int seg_len = segment ? segment : dbw::SURFACE_SEGMENT;
    char *ws = (char *)workspace;
    const float tau2 = tau * tau;
    const bool has_back = back > 0.f;
    const double scale_fwd = (double)weight / (double)M, scale_back = has_back ? (double)weight * (double)back / back_count : 0.0;
    double *part = (double *)(ws + L.bwd_part);

    hipLaunchKernelGGL(surface_bwd_kernel, dim3((unsigned)L.segs, (unsigned)L.vert_groups), dim3(SF_BLOCK), 0, st, points, (uint32_t)N, (int)M,
                       n_points ? 1 : 0, (uint64_t)seed, (uint64_t)step, (const float4 *)records, (const float *)(ws + L.tri), faces, F, V, seg_len, tau2,
                       part);
    int rc = dbw_check_launch("surface_bwd_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(surface_bwd_finish_kernel, dim3((unsigned)L.vert_groups), dim3(SF_BLOCK), 0, st, (const double *)part, L.segs, V, verts, points,
                       has_back ? (const unsigned long long *)(ws + L.keys) : (const unsigned long long *)nullptr, vert_alpha, vert_group, A, (uint32_t)N, tau2,
                       scale_fwd, scale_back, grad_out, grad_verts);
    if ((rc = dbw_check_launch("surface_bwd_finish_kernel"))) return rc;
    if (grad_alpha && A >= 1) {
        hipLaunchKernelGGL(surface_alpha_kernel, dim3((unsigned)A), dim3(SF_BLOCK), 0, st,
                           has_back ? (const float *)(ws + L.rho_back) : (const float *)nullptr, vert_group, V, scale_back, grad_out, grad_alpha);
        if ((rc = dbw_check_launch("surface_alpha_kernel"))) return rc;
    }
    return 0;
}
