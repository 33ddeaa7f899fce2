// The free-space term behind two calls (include/dbw_eval.h: dbw_eval_freespace_fwd / _bwd): depth rays, from a camera centre to the measured
// surface point, against the posed meshes -- the first face a ray meets before its end is penalised by the metric distance it lies in front
// of that end.  The arithmetic is csrc/freespace_math.h (also built by g++ for the host tests); the workspace's common regions, the two
// walks, the segment sum and the checks both terms make are csrc/mesh_walk.h.
//
// Forward launches
//   surface_box_kernel      (csrc/surface_term.hip, dbw_surface_box_launch) the kept faces gathered, 12 floats a face, and the groups' boxes
//   freespace_tag_kernel    one workgroup per group: float 9 of each of its faces' 12 gets the group's row of the opacities (-1: ground), so
//                           that a face index alone leads to its opacity
//   freespace_fwd_kernel    one ray per lane, drawn in the kernel (freespace_draw_index), through the group walk of csrc/mesh_walk.h with
//                           freespace_hit per face.  With cull a group is skipped when NO lane's segment t in (0, best t so far) reaches
//                           the group's slackened box (freespace_slab_reaches): the records do not depend on `cull`.  One 16-byte record a
//                           ray, its psi (fp32) for the opacity gradient, and the workgroup's sum of a psi in fp64 through block_sum.
//   partials_finish         value[0] = sum a psi / M
// The forward has a second layout (layout 2, the default: profiles/freespace_term.md has both times).  At M = 16384 the layout above is 64
// workgroups on 256 CUs, each walking every face.
//   keys                    one 64-bit key a ray, set to all ones (hipMemsetAsync)
//   freespace_chunk_kernel  grid (ray tile of 256, face chunk of FS_CHUNK): a lane draws its ray as above and takes the same walk over the
//                           faces of its chunk; its best key goes into the ray's word with a 64-bit integer atomicMin -- the minimum of
//                           integers does not depend on the order of arrival
//   freespace_pick_kernel   one ray per lane: the winner's (t, u, v) formed again by freespace_hit on the same inputs (the same bytes; t is
//                           the key's), the record, psi and the workgroup's partial as the first layout writes them
//
// Backward launches
//   freespace_bwd_kernel    the segment walk of csrc/mesh_walk.h: a corner of the record's face adds -a psi'(g) l wts_m n / (n . e)
//   freespace_bwd_finish    one thread per vertex: the segments' partials added in segment order, scaled, rounded to fp32
//   freespace_alpha_kernel  one workgroup per opacity: the psi of the records that hit its block, added in a fixed order (thread t takes
//                           t, t + 256, ...; block_sum)
#include "dbw_common.h"
#include "freespace_math.h"
#include "loss_reduce.h"
#include "mesh_walk.h"
#include "surface_box.h"
#include "../../include/dbw_eval.h"

#include <math.h>

namespace {

using dbw::MESH_BLOCK;
using dbw::MESH_TRI;                            // (float 9 of a gathered face is this term's tag)
using dbw::clampi;
constexpr int FS_CHUNK = 128;                   // faces of a workgroup of the second forward layout
constexpr int FS_MAX_FRAMES = 1 << 20;
static_assert(DBW_EVAL_FREESPACE_SEGMENT == dbw::FREESPACE_SEGMENT, "the header mirrors the segment length of freespace_math.h");

struct FreespaceLayout : dbw::MeshLayout {
    size_t psi, keys;
    FreespaceLayout(int64_t M, int F, int V, int G, int segment) : dbw::MeshLayout(M, F, V, G, segment, dbw::FREESPACE_SEGMENT) {
        psi = add((size_t)M * sizeof(float));
        keys = add((size_t)M * sizeof(unsigned long long));
        close(V);
    }
};

inline bool freespace_sizes_ok(int64_t M, int F, int V, int G, int segment) { return dbw::mesh_sizes_ok(M, F, V, G, segment, dbw::FREESPACE_SEGMENT); }

__global__ __launch_bounds__(MESH_BLOCK) void freespace_tag_kernel(const int32_t *__restrict__ face_group, const int32_t *__restrict__ group_alpha, int F,
                                                                 float *__restrict__ tri) {
    const int g = blockIdx.x;
    const int f0 = clampi(face_group[g], 0, F), f1 = clampi(face_group[g + 1], 0, F);
    const float tag = __int_as_float(group_alpha[g]);
    for (int f = f0 + (int)threadIdx.x; f < f1; f += MESH_BLOCK) tri[(size_t)f * MESH_TRI + 9] = tag;
}

struct FreespaceRay { float o[3], e[3]; };

// Ray `draw i` of the step: origin and end - origin.  A ray whose frame is outside [0, Nf) has e = 0: no face is a candidate for it.
__device__ __forceinline__ FreespaceRay freespace_ray(const float *__restrict__ ends, const int32_t *__restrict__ frame, const float *__restrict__ origins,
                                                      uint32_t Nr, int Nf, int draw, uint64_t seed, uint64_t step, uint32_t i) {
    const size_t j = draw ? dbw::freespace_draw_index(seed, step, i, Nr) : i;
    const float px = ends[j * 3], py = ends[j * 3 + 1], pz = ends[j * 3 + 2];
    const int fr = frame[j];
    FreespaceRay r;
    if (fr >= 0 && fr < Nf) {
        r.o[0] = origins[(size_t)fr * 3]; r.o[1] = origins[(size_t)fr * 3 + 1]; r.o[2] = origins[(size_t)fr * 3 + 2];
    } else {
        r.o[0] = px; r.o[1] = py; r.o[2] = pz;
    }
    r.e[0] = px - r.o[0]; r.e[1] = py - r.o[1]; r.e[2] = pz - r.o[2];
    return r;
}

// the opacity of the block a face belongs to (1: the ground, or a row outside [0, A)) and that row
__device__ __forceinline__ float freespace_face_alpha(const float *__restrict__ tri, int f, const float *__restrict__ vert_alpha, int A, int &row) {
    row = __float_as_int(tri[(size_t)f * MESH_TRI + 9]);
    return (vert_alpha && row >= 0 && row < A) ? vert_alpha[row] : 1.f;
}

// What a ray leaves behind once its first hit is known: the record, its psi, and (returned) a psi for the workgroup's sum.
__device__ __forceinline__ double freespace_emit(int i, unsigned long long best, float best_t, float bu, float bv, const FreespaceRay &ray,
                                                 const float *__restrict__ tri, const float *__restrict__ vert_alpha, int A, float tau, float margin,
                                                 float4 *__restrict__ records, float *__restrict__ psi_out) {
    double s = 0.0;
    float psi = 0.f;
    if (best != ~0ull) {
        const int f = (int)(uint32_t)(best & 0xffffffffull);
        records[i] = make_float4(best_t, __int_as_float(f), bu, bv);
        const float l = dbw::freespace_length(ray.e[0], ray.e[1], ray.e[2]);
        psi = dbw::freespace_psi(dbw::freespace_g(best_t, l, margin), tau);
        int row;
        s = (double)freespace_face_alpha(tri, f, vert_alpha, A, row) * (double)psi;
    } else {
        records[i] = make_float4(__int_as_float(0x7fc00000), __int_as_float(-1), 0.f, 0.f);
    }
    psi_out[i] = psi;
    return s;
}

// a ray's first hit so far: the visitor of mesh_group_walk
struct FreespaceFirstHit {
    FreespaceRay ray = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};          // (what a lane past the rays keeps)
    unsigned long long best = ~0ull;
    float best_t = 1.f, bu = 0.f, bv = 0.f;
    __device__ __forceinline__ bool reaches(const float lo[3], const float hi[3]) const { return dbw::freespace_slab_reaches(lo, hi, ray.o, ray.e, best_t); }
    __device__ __forceinline__ void face(const float tt[9], int f) {
        const dbw::FreespaceHit h = dbw::freespace_hit(tt, ray.o[0], ray.o[1], ray.o[2], ray.e[0], ray.e[1], ray.e[2]);
        if (h.hit) {
            const unsigned long long key = dbw::freespace_key(h.t, (uint32_t)f);
            if (key < best) { best = key; best_t = h.t; bu = h.u; bv = h.v; }
        }
    }
};

__global__ __launch_bounds__(MESH_BLOCK) void freespace_fwd_kernel(const float *__restrict__ ends, const int32_t *__restrict__ frame,
                                                                 const float *__restrict__ origins, uint32_t Nr, int Nf, int M, int draw, uint64_t seed,
                                                                 uint64_t step, const float *__restrict__ tri, const float *__restrict__ boxes,
                                                                 const int32_t *__restrict__ face_group, const int32_t *__restrict__ group_keep,
                                                                 const float *__restrict__ vert_alpha, int A, int F, int G, float tau, float margin,
                                                                 int cull, float4 *__restrict__ records, float *__restrict__ psi_out,
                                                                 double *__restrict__ partial) {
    __shared__ double red[dbw::LOSS_WAVES][1];
    const int i = blockIdx.x * MESH_BLOCK + threadIdx.x;
    const bool live = i < M;
    FreespaceFirstHit h;
    if (live) h.ray = freespace_ray(ends, frame, origins, Nr, Nf, draw, seed, step, (uint32_t)i);
    dbw::mesh_group_walk(tri, boxes, face_group, group_keep, F, G, 0, F, cull, live, h);
    double s = 0.0;
    if (live) s = freespace_emit(i, h.best, h.best_t, h.bu, h.bv, h.ray, tri, vert_alpha, A, tau, margin, records, psi_out);
    const double tsum = dbw::block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tsum;
}

__global__ __launch_bounds__(MESH_BLOCK) void freespace_chunk_kernel(const float *__restrict__ ends, const int32_t *__restrict__ frame,
                                                                   const float *__restrict__ origins, uint32_t Nr, int Nf, int M, int draw,
                                                                   uint64_t seed, uint64_t step, const float *__restrict__ tri,
                                                                   const float *__restrict__ boxes, const int32_t *__restrict__ face_group,
                                                                   const int32_t *__restrict__ group_keep, int F, int G, int cull,
                                                                   unsigned long long *__restrict__ keys) {
    const int i = blockIdx.x * MESH_BLOCK + threadIdx.x;
    const bool live = i < M;
    const int c0 = blockIdx.y * FS_CHUNK, c1 = c0 + FS_CHUNK < F ? c0 + FS_CHUNK : F;
    FreespaceFirstHit h;
    if (live) h.ray = freespace_ray(ends, frame, origins, Nr, Nf, draw, seed, step, (uint32_t)i);
    dbw::mesh_group_walk(tri, boxes, face_group, group_keep, F, G, c0, c1, cull, live, h);
    if (live && h.best != ~0ull) atomicMin(keys + i, h.best);
}

__global__ __launch_bounds__(MESH_BLOCK) void freespace_pick_kernel(const float *__restrict__ ends, const int32_t *__restrict__ frame,
                                                                  const float *__restrict__ origins, uint32_t Nr, int Nf, int M, int draw,
                                                                  uint64_t seed, uint64_t step, const float *__restrict__ tri,
                                                                  const unsigned long long *__restrict__ keys, const float *__restrict__ vert_alpha,
                                                                  int A, int F, float tau, float margin, float4 *__restrict__ records,
                                                                  float *__restrict__ psi_out, double *__restrict__ partial) {
    __shared__ double red[dbw::LOSS_WAVES][1];
    const int i = blockIdx.x * MESH_BLOCK + threadIdx.x;
    double s = 0.0;
    if (i < M) {
        const FreespaceRay ray = freespace_ray(ends, frame, origins, Nr, Nf, draw, seed, step, (uint32_t)i);
        unsigned long long best = keys[i];
        float bt = 1.f, bu = 0.f, bv = 0.f;
        const uint32_t f = (uint32_t)(best & 0xffffffffull);
        if (best != ~0ull && f < (uint32_t)F) {
            const float *t = tri + (size_t)f * MESH_TRI;
            const float tt[9] = {t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]};
            const dbw::FreespaceHit h = dbw::freespace_hit(tt, ray.o[0], ray.o[1], ray.o[2], ray.e[0], ray.e[1], ray.e[2]);
            bt = h.t; bu = h.u; bv = h.v;                           // (the arithmetic that made the key: h.hit, and bits(h.t) are the key's)
        } else {
            best = ~0ull;
        }
        s = freespace_emit(i, best, bt, bu, bv, ray, tri, vert_alpha, A, tau, margin, records, psi_out);
    }
    const double tsum = dbw::block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tsum;
}

__global__ __launch_bounds__(MESH_BLOCK) void freespace_bwd_kernel(const float *__restrict__ ends, const int32_t *__restrict__ frame,
                                                                 const float *__restrict__ origins, uint32_t Nr, int Nf, int M, int draw, uint64_t seed,
                                                                 uint64_t step, const float4 *__restrict__ records, const float *__restrict__ tri,
                                                                 const int32_t *__restrict__ faces, const float *__restrict__ vert_alpha, int A, int F,
                                                                 int V, int seg_len, float tau, float margin, double *__restrict__ part) {
    // a record in front of its ray's end gives the corners of its face -a psi'(g) l wts_m n / (n . e)
    dbw::mesh_bwd_walk(records, tri, faces, M, F, V, seg_len, part, [](const float4 &) { return true; },
                       [&](int r, const float4 &rec, int f, const float *__restrict__ t, double wts, double acc[3]) {
        const FreespaceRay ray = freespace_ray(ends, frame, origins, Nr, Nf, draw, seed, step, (uint32_t)r);
        const float l = dbw::freespace_length(ray.e[0], ray.e[1], ray.e[2]);
        const float g = dbw::freespace_g(rec.x, l, margin);
        if (!(g > 0.f)) return;
        const double e1[3] = {(double)(t[3] - t[0]), (double)(t[4] - t[1]), (double)(t[5] - t[2])};
        const double e2[3] = {(double)(t[6] - t[0]), (double)(t[7] - t[1]), (double)(t[8] - t[2])};
        const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double ne = (n[0] * (double)ray.e[0] + n[1] * (double)ray.e[1]) + n[2] * (double)ray.e[2];
        if (ne == 0.0) return;
        int row;
        const double a = (double)freespace_face_alpha(tri, f, vert_alpha, A, row);
        const double coef = -(a * 2.0 * (double)(g < tau ? g : tau) * (double)l * wts) / ne;
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] += coef * n[k];
    });
}

// scale = weight / M, times grad_out[0] (1 without one)
__global__ __launch_bounds__(MESH_BLOCK) void freespace_bwd_finish_kernel(const double *__restrict__ part, int segs, int V, double scale,
                                                                        const float *__restrict__ grad_out, float *__restrict__ grad_verts) {
    const int v = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (v >= V) return;
    const double go = grad_out ? (double)grad_out[0] : 1.0;
    double s[3];
    dbw::mesh_segment_sum(part, segs, V, v, s);
#pragma unroll
    for (int c = 0; c < 3; ++c) grad_verts[(size_t)v * 3 + c] = (float)((s[c] * scale) * go);
}

__global__ __launch_bounds__(MESH_BLOCK) void freespace_alpha_kernel(const float4 *__restrict__ records, const float *__restrict__ psi,
                                                                   const float *__restrict__ tri, int M, int F, double scale,
                                                                   const float *__restrict__ grad_out, float *__restrict__ grad_alpha) {
    __shared__ double red[dbw::LOSS_WAVES][1];
    const int k = blockIdx.x;
    double s = 0.0;
    for (int r = threadIdx.x; r < M; r += MESH_BLOCK) {
        const int f = __float_as_int(records[r].y);
        if (f >= 0 && f < F && __float_as_int(tri[(size_t)f * MESH_TRI + 9]) == k) s += (double)psi[r];
    }
    const double t = dbw::block_sum(s, red);
    if (threadIdx.x == 0) grad_alpha[k] = (float)(t * scale * (grad_out ? (double)grad_out[0] : 1.0));
}

}  // namespace

extern "C" size_t dbw_eval_freespace_workspace_bytes(int64_t M, int F, int V, int G, int segment) {
    return freespace_sizes_ok(M, F, V, G, segment) ? FreespaceLayout(M, F, V, G, segment).total : 0;
}

#define FREESPACE_CHECKS                                                                                                                   \
    DBW_REQUIRE(Nr >= 1 && Nr < (1ll << 31), "Nr must be in [1, 2^31)");                                                                   \
    DBW_REQUIRE(Nf >= 1 && Nf <= FS_MAX_FRAMES, "Nf must be in [1, 2^20]");                                                                \
    DBW_REQUIRE(n_rays >= 0 && n_rays <= dbw::MESH_MAX_M && (n_rays > 0 || Nr <= dbw::MESH_MAX_M), "the rays of a step (n_rays, or Nr when it is 0) must be in [1, 2^24]"); \
    MESH_COMMON_CHECKS;                                                                                                                    \
    DBW_REQUIRE(margin >= 0.f && margin < INFINITY, "margin must be non-negative and finite");                                             \
    DBW_REQUIRE(A == 0 || vert_alpha, "A >= 1 needs vert_alpha")

extern "C" int dbw_eval_freespace_fwd(const float *ends, const int32_t *frame, const float *origins, int64_t Nr, int Nf, int64_t n_rays, int64_t seed,
                                      int64_t step, const float *verts, int V, const int32_t *faces, const int32_t *faces_host, int F,
                                      const int32_t *face_group, const int32_t *group_keep, const int32_t *group_alpha, int G, const float *vert_alpha,
                                      int A, float tau, float margin, int cull, int layout, void *workspace, void *records, double *value, dbw_stream_t stream) {
    DBW_REQUIRE(ends && frame && origins && verts && faces && face_group && group_alpha && workspace && records && value, "null pointer");
    FREESPACE_CHECKS;
    DBW_REQUIRE(cull == 0 || cull == 1, "cull must be 0 or 1");
    DBW_REQUIRE(layout >= 0 && layout <= 2, "layout must be 0, 1 or 2");
    DBW_REQUIRE(((uintptr_t)ends & 3) == 0 && ((uintptr_t)frame & 3) == 0 && ((uintptr_t)origins & 3) == 0 && ((uintptr_t)verts & 3) == 0 &&
                    ((uintptr_t)faces & 3) == 0 && ((uintptr_t)faces_host & 3) == 0 && ((uintptr_t)face_group & 3) == 0 &&
                    ((uintptr_t)group_keep & 3) == 0 && ((uintptr_t)group_alpha & 3) == 0 && ((uintptr_t)vert_alpha & 3) == 0 &&
                    ((uintptr_t)value & 7) == 0,
                "misaligned pointer");
    DBW_REQUIRE(!faces_host || dbw::mesh_faces_inside(faces_host, F, V), "a face index is outside [0, V)");
    const int64_t M = n_rays ? n_rays : Nr;
    const hipStream_t st = (hipStream_t)stream;
    const FreespaceLayout L(M, F, V, G, 0);   // (the backward's partials come last: the offsets before them do not depend on the segment)
    char *ws = (char *)workspace;
    float *boxes = (float *)(ws + L.boxes), *tri = (float *)(ws + L.tri), *psi = (float *)(ws + L.psi);
    double *fwd_part = (double *)(ws + L.fwd_part);

    int rc = dbw_surface_box_launch(verts, V, faces, F, face_group, group_keep, G, tri, boxes, st);
    if (rc) return rc;
    hipLaunchKernelGGL(freespace_tag_kernel, dim3((unsigned)G), dim3(MESH_BLOCK), 0, st, face_group, group_alpha, F, tri);
    if ((rc = dbw_check_launch("freespace_tag_kernel"))) return rc;
    if (layout == 1) {
        hipLaunchKernelGGL(freespace_fwd_kernel, dim3((unsigned)L.fwd_groups), dim3(MESH_BLOCK), 0, st, ends, frame, origins, (uint32_t)Nr, Nf, (int)M,
                           n_rays ? 1 : 0, (uint64_t)seed, (uint64_t)step, (const float *)tri, (const float *)boxes, face_group, group_keep, vert_alpha, A,
                           F, G, tau, margin, cull, (float4 *)records, psi, fwd_part);
        if ((rc = dbw_check_launch("freespace_fwd_kernel"))) return rc;
    } else {
        unsigned long long *keys = (unsigned long long *)(ws + L.keys);
        if (hipMemsetAsync(keys, 0xff, (size_t)M * sizeof(unsigned long long), st) != hipSuccess) {
            dbw_set_error("%s: hipMemsetAsync failed", __func__);
            return DBW_ERR_LAUNCH;
        }
        const unsigned chunks = (unsigned)((F + FS_CHUNK - 1) / FS_CHUNK);          // (F <= 2^20: at most 8192, within gridDim.y)
        hipLaunchKernelGGL(freespace_chunk_kernel, dim3((unsigned)L.fwd_groups, chunks), dim3(MESH_BLOCK), 0, st, ends, frame, origins, (uint32_t)Nr, Nf,
                           (int)M, n_rays ? 1 : 0, (uint64_t)seed, (uint64_t)step, (const float *)tri, (const float *)boxes, face_group, group_keep, F, G,
                           cull, keys);
        if ((rc = dbw_check_launch("freespace_chunk_kernel"))) return rc;
        hipLaunchKernelGGL(freespace_pick_kernel, dim3((unsigned)L.fwd_groups), dim3(MESH_BLOCK), 0, st, ends, frame, origins, (uint32_t)Nr, Nf, (int)M,
                           n_rays ? 1 : 0, (uint64_t)seed, (uint64_t)step, (const float *)tri, (const unsigned long long *)keys, vert_alpha, A, F, tau,
                           margin, (float4 *)records, psi, fwd_part);
        if ((rc = dbw_check_launch("freespace_pick_kernel"))) return rc;
    }
    return dbw::partials_finish(fwd_part, L.fwd_groups, 1.0, (double)M, value, st);
}

extern "C" int dbw_eval_freespace_bwd(const float *ends, const int32_t *frame, const float *origins, int64_t Nr, int Nf, int64_t n_rays, int64_t seed,
                                      int64_t step, const float *verts, int V, const int32_t *faces, int F, int G, const float *vert_alpha, int A,
                                      float tau, float margin, float weight, const float *grad_out, int segment, const void *records, void *workspace,
                                      float *grad_verts, float *grad_alpha, dbw_stream_t stream) {
    DBW_REQUIRE(ends && frame && origins && verts && faces && workspace && records && grad_verts, "null pointer");
    FREESPACE_CHECKS;
    DBW_REQUIRE(A == 0 || grad_alpha, "A >= 1 needs grad_alpha");
    DBW_REQUIRE(weight == weight && fabsf(weight) < INFINITY, "weight must be finite");
    DBW_REQUIRE(segment == 0 || (segment >= 64 && segment <= (1 << 20)), "segment must be 0 or in [64, 2^20]");
    DBW_REQUIRE(((uintptr_t)ends & 3) == 0 && ((uintptr_t)frame & 3) == 0 && ((uintptr_t)origins & 3) == 0 && ((uintptr_t)verts & 3) == 0 &&
                    ((uintptr_t)faces & 3) == 0 && ((uintptr_t)vert_alpha & 3) == 0 && ((uintptr_t)grad_out & 3) == 0 &&
                    ((uintptr_t)grad_verts & 3) == 0 && ((uintptr_t)grad_alpha & 3) == 0,
                "misaligned pointer");
    const int64_t M = n_rays ? n_rays : Nr;
    DBW_REQUIRE(freespace_sizes_ok(M, F, V, G, segment), "too many segments: raise segment");
    const hipStream_t st = (hipStream_t)stream;
    const FreespaceLayout L(M, F, V, G, segment);
    const int seg_len = segment ? segment : dbw::FREESPACE_SEGMENT;
    char *ws = (char *)workspace;
    const double scale = (double)weight / (double)M;
    double *part = (double *)(ws + L.bwd_part);
    const float *tri = (const float *)(ws + L.tri);

    hipLaunchKernelGGL(freespace_bwd_kernel, dim3((unsigned)L.segs, (unsigned)L.vert_groups), dim3(MESH_BLOCK), 0, st, ends, frame, origins, (uint32_t)Nr,
                       Nf, (int)M, n_rays ? 1 : 0, (uint64_t)seed, (uint64_t)step, (const float4 *)records, tri, faces, vert_alpha, A, F, V, seg_len, tau,
                       margin, part);
    int rc = dbw_check_launch("freespace_bwd_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(freespace_bwd_finish_kernel, dim3((unsigned)L.vert_groups), dim3(MESH_BLOCK), 0, st, (const double *)part, L.segs, V, scale, grad_out,
                       grad_verts);
    if ((rc = dbw_check_launch("freespace_bwd_finish_kernel"))) return rc;
    if (grad_alpha && A >= 1) {
        hipLaunchKernelGGL(freespace_alpha_kernel, dim3((unsigned)A), dim3(MESH_BLOCK), 0, st, (const float4 *)records, (const float *)(ws + L.psi), tri,
                           (int)M, F, scale, grad_out, grad_alpha);
        if ((rc = dbw_check_launch("freespace_alpha_kernel"))) return rc;
    }
    return 0;
}
