// The surface term behind two calls (include/dbw_eval.h: dbw_eval_surface_fwd / _bwd): the truncated squared distance of drawn cloud points
// to the posed meshes, and of the block vertices to the cloud.  The arithmetic is csrc/surface_math.h (also built by g++ for the host
// tests); the workspace's common regions, the two walks, the segment sum and the checks both terms make are csrc/mesh_walk.h.
//
// Forward launches
//   surface_box_kernel    one workgroup per group (ground, block 0, block 1, ...): the 9 coordinates of each of its faces gathered into the
//                         workspace (12 floats a face: three 16-byte scalar loads later) and the group's axis-aligned box.  A face index
//                         outside [0, V) is read as vertex 0: no launch reads outside `verts`, whatever `faces` holds.
//   surface_fwd_kernel    one point per lane, drawn in the kernel (surface_draw_index), through the group walk of csrc/mesh_walk.h with
//                         surface_closest per face.  With cull a group is skipped when EVERY lane's box bound is strictly above its running
//                         best d2: the bound is never above a d2 that the group could give, so a skipped group holds no key below any
//                         lane's best and the records do not depend on `cull`.  One 16-byte record a point; the workgroup's sum of rho in
//                         fp64 through block_sum, one partial a workgroup.
//   nn search             (back > 0) the exact nearest cloud point of every vertex: dbw_nn_search_launch, 64-bit keys
//   surface_back_kernel   (back > 0) rho of every block vertex, a_k * rho summed like the forward's
//   partials_finish       twice: value[0] = sum rho / M, value[1] = sum a rho / back_count
//
// Backward launches
//   surface_bwd_kernel    the segment walk of csrc/mesh_walk.h: a corner of the record's face adds -2 b_m (p - c) for a record inside tau
//   surface_bwd_finish    one thread per vertex: the segments' partials added in segment order, the back direction's 2 a_k (x_v - nn) added,
//                         scaled, rounded to fp32
//   surface_alpha_kernel  one workgroup per opacity: the rho of its vertices added in a fixed order (thread t takes t, t + 256, ...; block_sum)
#include "dbw_common.h"
#include "loss_reduce.h"
#include "mesh_walk.h"
#include "nn_search.h"
#include "surface_box.h"
#include "surface_math.h"
#include "../../include/dbw_eval.h"

#include <math.h>

namespace {

using dbw::MESH_BLOCK;
using dbw::MESH_TRI;
using dbw::clampi;
static_assert(DBW_EVAL_SURFACE_SEGMENT == dbw::SURFACE_SEGMENT, "the header mirrors the segment length of surface_math.h");

struct SurfaceLayout : dbw::MeshLayout {
    size_t keys, back_part, rho_back;
    SurfaceLayout(int64_t M, int F, int V, int G, int segment) : dbw::MeshLayout(M, F, V, G, segment, dbw::SURFACE_SEGMENT) {
        keys = add((size_t)V * sizeof(unsigned long long));
        back_part = add((size_t)vert_groups * sizeof(double));
        rho_back = add((size_t)V * sizeof(float));
        close(V);
    }
};

inline bool surface_sizes_ok(int64_t M, int F, int V, int G, int segment) { return dbw::mesh_sizes_ok(M, F, V, G, segment, dbw::SURFACE_SEGMENT); }

__global__ __launch_bounds__(MESH_BLOCK) void surface_box_kernel(const float *__restrict__ verts, int V, const int32_t *__restrict__ faces, int F,
                                                               const int32_t *__restrict__ face_group, const int32_t *__restrict__ group_keep,
                                                               float *__restrict__ tri, float *__restrict__ boxes) {
    __shared__ float sh[MESH_BLOCK / DBW_WAVE][6];
    const int g = blockIdx.x;
    const int f0 = clampi(face_group[g], 0, F), f1 = clampi(face_group[g + 1], 0, F);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (!group_keep || group_keep[g]) {
        for (int f = f0 + (int)threadIdx.x; f < f1; f += MESH_BLOCK) {
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                int i = faces[f * 3 + m];
                i = (i >= 0 && i < V) ? i : 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float x = verts[(size_t)i * 3 + k];
                    tri[(size_t)f * MESH_TRI + m * 3 + k] = x;
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
        for (int w = 1; w < MESH_BLOCK / DBW_WAVE; ++w) {
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

// a point's nearest face so far: the visitor of mesh_group_walk
struct SurfaceNearest {
    float px = 0.f, py = 0.f, pz = 0.f;
    unsigned long long best = ~0ull;
    float best_d2 = INFINITY, bu = 0.f, bv = 0.f;
    __device__ __forceinline__ bool reaches(const float lo[3], const float hi[3]) const { return !(dbw::surface_box_bound(lo, hi, px, py, pz) > best_d2); }
    __device__ __forceinline__ void face(const float tt[9], int f) {
        const dbw::SurfaceHit h = dbw::surface_closest(tt, px, py, pz);
        const unsigned long long key = dbw::surface_key(h.d2, (uint32_t)f);
        if (key < best) { best = key; best_d2 = h.d2; bu = h.u; bv = h.v; }
    }
};

__global__ __launch_bounds__(MESH_BLOCK) void surface_fwd_kernel(const float *__restrict__ points, uint32_t N, int M, int draw, uint64_t seed,
                                                               uint64_t step, const float *__restrict__ tri, const float *__restrict__ boxes,
                                                               const int32_t *__restrict__ face_group, const int32_t *__restrict__ group_keep,
                                                               int F, int G, float tau2, int cull, float4 *__restrict__ records,
                                                               double *__restrict__ partial) {
    __shared__ double red[dbw::LOSS_WAVES][1];
    const int i = blockIdx.x * MESH_BLOCK + threadIdx.x;
    const bool live = i < M;
    SurfaceNearest near;
    if (live) surface_point(points, N, draw, seed, step, (uint32_t)i, near.px, near.py, near.pz);
    dbw::mesh_group_walk(tri, boxes, face_group, group_keep, F, G, 0, F, cull, live, near);
    double s = 0.0;
    if (live) {
        const float d2 = dbw::surface_key_d2(near.best);
        records[i] = make_float4(d2, __int_as_float((int)(uint32_t)(near.best & 0xffffffffull)), near.bu, near.bv);
        s = (double)dbw::surface_rho(d2, tau2);
    }
    const double tsum = dbw::block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tsum;
}

__global__ __launch_bounds__(MESH_BLOCK) void surface_back_kernel(const unsigned long long *__restrict__ keys, int V,
                                                                const float *__restrict__ vert_alpha, const int32_t *__restrict__ vert_group,
                                                                int A, float tau2, float *__restrict__ rho_back, double *__restrict__ partial) {
    __shared__ double red[dbw::LOSS_WAVES][1];
    const int v = blockIdx.x * MESH_BLOCK + threadIdx.x;
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

__global__ __launch_bounds__(MESH_BLOCK) void surface_bwd_kernel(const float *__restrict__ points, uint32_t N, int M, int draw, uint64_t seed,
                                                               uint64_t step, const float4 *__restrict__ records, const float *__restrict__ tri,
                                                               const int32_t *__restrict__ faces, int F, int V, int seg_len, float tau2,
                                                               double *__restrict__ part) {
    // a record inside tau gives the corners of its face -2 b_m (p - c)
    dbw::mesh_bwd_walk(records, tri, faces, M, F, V, seg_len, part, [&](const float4 &rec) { return rec.x < tau2; },
                       [&](int r, const float4 &rec, int f, const float *__restrict__ t, double coef, double acc[3]) {
        float px, py, pz;
        surface_point(points, N, draw, seed, step, (uint32_t)r, px, py, pz);
        const float e1[3] = {t[3] - t[0], t[4] - t[1], t[5] - t[2]}, e2[3] = {t[6] - t[0], t[7] - t[1], t[8] - t[2]};
        const float q[3] = {px - t[0], py - t[1], pz - t[2]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float d = q[k] - (rec.z * e1[k] + rec.w * e2[k]);                 // p - c, the forward's own operations
            acc[k] -= 2.0 * coef * (double)d;
        }
    });
}

// scale_fwd = weight / M, scale_back = weight * back / back_count; both times grad_out[0] (1 without one)
__global__ __launch_bounds__(MESH_BLOCK) void surface_bwd_finish_kernel(const double *__restrict__ part, int segs, int V, const float *__restrict__ verts,
                                                                      const float *__restrict__ points, const unsigned long long *__restrict__ keys,
                                                                      const float *__restrict__ vert_alpha, const int32_t *__restrict__ vert_group,
                                                                      int A, uint32_t N, float tau2, double scale_fwd, double scale_back,
                                                                      const float *__restrict__ grad_out, float *__restrict__ grad_verts) {
    const int v = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (v >= V) return;
    const double go = grad_out ? (double)grad_out[0] : 1.0;
    double s[3];
    dbw::mesh_segment_sum(part, segs, V, v, s);
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

__global__ __launch_bounds__(MESH_BLOCK) void surface_alpha_kernel(const float *__restrict__ rho_back, const int32_t *__restrict__ vert_group, int V,
                                                                 double scale_back, const float *__restrict__ grad_out,
                                                                 float *__restrict__ grad_alpha) {
    __shared__ double red[dbw::LOSS_WAVES][1];
    const int k = blockIdx.x;
    double s = 0.0;
    if (rho_back) {
        for (int v = threadIdx.x; v < V; v += MESH_BLOCK) s += vert_group[v] == k ? (double)rho_back[v] : 0.0;
    }
    const double t = dbw::block_sum(s, red);
    if (threadIdx.x == 0) grad_alpha[k] = (float)(t * scale_back * (grad_out ? (double)grad_out[0] : 1.0));
}

}  // namespace

// the box launch for the other term that walks the same gathered faces (csrc/freespace_term.hip): tri (F, 12 floats), boxes (G, 8 floats)
int dbw_surface_box_launch(const float *verts, int V, const int32_t *faces, int F, const int32_t *face_group, const int32_t *group_keep, int G,
                           float *tri, float *boxes, hipStream_t stream) {
    hipLaunchKernelGGL(surface_box_kernel, dim3((unsigned)G), dim3(MESH_BLOCK), 0, stream, verts, V, faces, F, face_group, group_keep, tri, boxes);
    return dbw_check_launch("surface_box_kernel");
}

extern "C" size_t dbw_eval_surface_workspace_bytes(int64_t M, int F, int V, int G, int segment) {
    return surface_sizes_ok(M, F, V, G, segment) ? SurfaceLayout(M, F, V, G, segment).total : 0;
}

#define SURFACE_CHECKS                                                                                                                     \
    DBW_REQUIRE(N >= 1 && N < (1ll << 31), "N must be in [1, 2^31)");                                                                      \
    DBW_REQUIRE(n_points >= 0 && n_points <= dbw::MESH_MAX_M && (n_points > 0 || N <= dbw::MESH_MAX_M), "the points of a step (n_points, or N when it is 0) must be in [1, 2^24]"); \
    MESH_COMMON_CHECKS;                                                                                                                    \
    DBW_REQUIRE(back >= 0.f && back < INFINITY, "back must be non-negative and finite");                                                   \
    DBW_REQUIRE(back == 0.f || (vert_alpha && vert_group), "back > 0 needs vert_alpha and vert_group");                                    \
    DBW_REQUIRE(back == 0.f || (A >= 1 && back_count > 0.0), "back > 0 needs A >= 1 and a positive back_count")

extern "C" int dbw_eval_surface_fwd(const float *points, int64_t N, int64_t n_points, int64_t seed, int64_t step, const float *verts, int V,
                                    const int32_t *faces, const int32_t *faces_host, int F, const int32_t *face_group, const int32_t *group_keep, int G,
                                    const float *vert_alpha, const int32_t *vert_group, int A, double back_count, float tau, float back, int cull,
                                    void *workspace, void *records, double *value, dbw_stream_t stream) {
    DBW_REQUIRE(points && verts && faces && face_group && workspace && records && value, "null pointer");
    SURFACE_CHECKS;
    DBW_REQUIRE(cull == 0 || cull == 1, "cull must be 0 or 1");
    DBW_REQUIRE(((uintptr_t)points & 3) == 0 && ((uintptr_t)verts & 3) == 0 && ((uintptr_t)faces & 3) == 0 && ((uintptr_t)faces_host & 3) == 0 &&
                    ((uintptr_t)face_group & 3) == 0 && ((uintptr_t)group_keep & 3) == 0 && ((uintptr_t)vert_alpha & 3) == 0 &&
                    ((uintptr_t)vert_group & 3) == 0 && ((uintptr_t)value & 7) == 0,
                "misaligned pointer");
    DBW_REQUIRE(!faces_host || dbw::mesh_faces_inside(faces_host, F, V), "a face index is outside [0, V)");
    const int64_t M = n_points ? n_points : N;
    const int draw = n_points ? 1 : 0;
    int splits = 0;
    if (back > 0.f) {
        splits = dbw_nn_search_plan(__func__, 1, V, (int)N, 0);
        if (splits < 0) return splits;
    }
    const hipStream_t st = (hipStream_t)stream;
    const SurfaceLayout L(M, F, V, G, 0);      // (the backward's partials come last: the offsets before them do not depend on the segment)
    char *ws = (char *)workspace;
    float *boxes = (float *)(ws + L.boxes), *tri = (float *)(ws + L.tri), *rho_back = (float *)(ws + L.rho_back);
    double *fwd_part = (double *)(ws + L.fwd_part), *back_part = (double *)(ws + L.back_part);
    const float tau2 = tau * tau;

    int rc = dbw_surface_box_launch(verts, V, faces, F, face_group, group_keep, G, tri, boxes, st);
    if (rc) return rc;
    hipLaunchKernelGGL(surface_fwd_kernel, dim3((unsigned)L.fwd_groups), dim3(MESH_BLOCK), 0, st, points, (uint32_t)N, (int)M, draw, (uint64_t)seed,
                       (uint64_t)step, (const float *)tri, (const float *)boxes, face_group, group_keep, F, G, tau2, cull, (float4 *)records, fwd_part);
    if ((rc = dbw_check_launch("surface_fwd_kernel"))) return rc;
    if ((rc = dbw::partials_finish(fwd_part, L.fwd_groups, 1.0, (double)M, value, st))) return rc;
    if (back > 0.f) {
        if ((rc = dbw_nn_search_launch(verts, points, nullptr, nullptr, 1, V, (int)N, splits, ws + L.keys, st))) return rc;
        hipLaunchKernelGGL(surface_back_kernel, dim3((unsigned)L.vert_groups), dim3(MESH_BLOCK), 0, st, (const unsigned long long *)(ws + L.keys), V,
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
    SURFACE_CHECKS;
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
    const SurfaceLayout L(M, F, V, G, segment);
    const int seg_len = segment ? segment : dbw::SURFACE_SEGMENT;
    char *ws = (char *)workspace;
    const float tau2 = tau * tau;
    const bool has_back = back > 0.f;
    const double scale_fwd = (double)weight / (double)M, scale_back = has_back ? (double)weight * (double)back / back_count : 0.0;
    double *part = (double *)(ws + L.bwd_part);

    hipLaunchKernelGGL(surface_bwd_kernel, dim3((unsigned)L.segs, (unsigned)L.vert_groups), dim3(MESH_BLOCK), 0, st, points, (uint32_t)N, (int)M,
                       n_points ? 1 : 0, (uint64_t)seed, (uint64_t)step, (const float4 *)records, (const float *)(ws + L.tri), faces, F, V, seg_len, tau2,
                       part);
    int rc = dbw_check_launch("surface_bwd_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(surface_bwd_finish_kernel, dim3((unsigned)L.vert_groups), dim3(MESH_BLOCK), 0, st, (const double *)part, L.segs, V, verts, points,
                       has_back ? (const unsigned long long *)(ws + L.keys) : (const unsigned long long *)nullptr, vert_alpha, vert_group, A, (uint32_t)N, tau2,
                       scale_fwd, scale_back, grad_out, grad_verts);
    if ((rc = dbw_check_launch("surface_bwd_finish_kernel"))) return rc;
    if (grad_alpha && A >= 1) {
        hipLaunchKernelGGL(surface_alpha_kernel, dim3((unsigned)A), dim3(MESH_BLOCK), 0, st,
                           has_back ? (const float *)(ws + L.rho_back) : (const float *)nullptr, vert_group, V, scale_back, grad_out, grad_alpha);
        if ((rc = dbw_check_launch("surface_alpha_kernel"))) return rc;
    }
    return 0;
}
