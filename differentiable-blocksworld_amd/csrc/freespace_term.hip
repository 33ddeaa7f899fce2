// The free-space term behind two calls (include/dbw_eval.h: dbw_eval_freespace_fwd / _bwd): depth rays, from a camera centre to the measured
// surface point, against the posed meshes -- the first face a ray meets before its end is penalised by the metric distance it lies in front
// of that end.  The arithmetic is csrc/freespace_math.h (also built by g++ for the host tests); this file is the schedule.  No MFMA, no
// floating-point atomics, no cross-workgroup waiting: plain launches on the caller's stream, kernel boundaries the only ordering, nothing
// read by the host.
//
// Forward launches
//   surface_box_kernel      (csrc/surface_term.hip, dbw_surface_box_launch) the kept faces gathered, 12 floats a face, and the groups' boxes
//   freespace_tag_kernel    one workgroup per group: float 9 of each of its faces' 12 gets the group's row of the opacities (-1: ground), so
//                           that a face index alone leads to its opacity
//   freespace_fwd_kernel    one ray per lane, drawn in the kernel (freespace_draw_index).  The groups are walked in order; group and face are
//                           wave-uniform, so box and face coordinates arrive by scalar loads and every lane runs freespace_hit on them.  A
//                           group is skipped when it is not kept or (cull) when NO lane's segment t in (0, best t so far) reaches the group's
//                           slackened box (freespace_slab_reaches): the records do not depend on `cull`.  One 16-byte record a ray, its psi
//                           (fp32) for the opacity gradient, and the workgroup's sum of a psi in fp64 through block_sum.
//   partials_finish         value[0] = sum a psi / M
// The forward has a second layout (layout 2, the default: profiles/freespace_term.md has both times).  At M = 16384 the layout above is 64
// workgroups on 256 CUs, each walking every face.
//   keys                    one 64-bit key a ray, set to all ones (hipMemsetAsync)
//   freespace_chunk_kernel  grid (ray tile of 256, face chunk of FS_CHUNK): a lane draws its ray as above and walks the faces of its chunk
//                           group by group (dropped groups and, with cull, groups no lane reaches are skipped); its best key goes into the
//                           ray's word with a 64-bit integer atomicMin -- the minimum of integers does not depend on the order of arrival
//   freespace_pick_kernel   one ray per lane: the winner's (t, u, v) formed again by freespace_hit on the same inputs (the same bytes; t is
//                           the key's), the record, psi and the workgroup's partial as the first layout writes them
//
// Backward launches
//   freespace_bwd_kernel    grid (segment, 256 vertices): a workgroup walks its segment of the records in index order, the record uniform
//                           across the workgroup; a thread whose vertex is a corner of the record's face adds
//                           -a psi'(g) l wts_m n / (n . e) to its own fp64 sum.  A wave none of whose vertices is a corner does no arithmetic
//                           for the record.  Partials [segment][V][3].
//   freespace_bwd_finish    one thread per vertex: the segments' partials added in segment order, scaled, rounded to fp32
//   freespace_alpha_kernel  one workgroup per opacity: the psi of the records that hit its block, added in a fixed order (thread t takes
//                           t, t + 256, ...; block_sum)
// The grids depend on the sizes alone and every sum has one order: the same call gives the same bytes.
#include "dbw_common.h"
#include "freespace_math.h"
#include "loss_reduce.h"
#include "surface_box.h"
#include "../../include/dbw_eval.h"

#include <math.h>

namespace {

constexpr int FS_BLOCK = dbw::LOSS_THREADS;
constexpr int FS_CHUNK = 128;                   // faces of a workgroup of the second forward layout
constexpr int FS_TRI = 12;                      // floats a gathered face takes (surface_box.h); float 9 is the tag
constexpr int FS_MAX_G = 4096, FS_MAX_F = 1 << 20, FS_MAX_V = 1 << 21, FS_MAX_M = 1 << 24, FS_MAX_SEGS = 65535, FS_MAX_FRAMES = 1 << 20;
static_assert(DBW_EVAL_FREESPACE_SEGMENT == dbw::FREESPACE_SEGMENT, "the header mirrors the segment length of freespace_math.h");

struct FreespaceLayout {          // byte offsets into the workspace
    size_t boxes, tri, fwd_part, psi, keys, bwd_part, total;
    int fwd_groups, vert_groups, segs;
};

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

inline bool freespace_sizes_ok(int64_t M, int F, int V, int G, int segment) {
    if (!(M >= 1 && M <= FS_MAX_M && F >= 1 && F <= FS_MAX_F && V >= 1 && V <= FS_MAX_V && G >= 1 && G <= FS_MAX_G)) return false;
    if (segment < 0) return false;
    const int64_t L = segment ? segment : dbw::FREESPACE_SEGMENT;
    return (M + L - 1) / L <= FS_MAX_SEGS;
}

inline FreespaceLayout freespace_layout(int64_t M, int F, int V, int G, int segment) {
    FreespaceLayout L;
    const int64_t seg = segment ? segment : dbw::FREESPACE_SEGMENT;
    L.fwd_groups = (int)((M + FS_BLOCK - 1) / FS_BLOCK);
    L.vert_groups = (V + FS_BLOCK - 1) / FS_BLOCK;
    L.segs = (int)((M + seg - 1) / seg);
    size_t o = 0;
    L.boxes = o; o = align16(o + (size_t)G * 8 * sizeof(float));
    L.tri = o; o = align16(o + (size_t)F * FS_TRI * sizeof(float));
    L.fwd_part = o; o = align16(o + (size_t)L.fwd_groups * sizeof(double));
    L.psi = o; o = align16(o + (size_t)M * sizeof(float));
    L.keys = o; o = align16(o + (size_t)M * sizeof(unsigned long long));
    L.bwd_part = o; o = align16(o + (size_t)L.segs * V * 3 * sizeof(double));
    L.total = o;
    return L;
}

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

__global__ __launch_bounds__(FS_BLOCK) void freespace_tag_kernel(const int32_t *__restrict__ face_group, const int32_t *__restrict__ group_alpha, int F,
                                                                 float *__restrict__ tri) {
    const int g = blockIdx.x;
    const int f0 = clampi(face_group[g], 0, F), f1 = clampi(face_group[g + 1], 0, F);
    const float tag = __int_as_float(group_alpha[g]);
    for (int f = f0 + (int)threadIdx.x; f < f1; f += FS_BLOCK) tri[(size_t)f * FS_TRI + 9] = tag;
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
    row = __float_as_int(tri[(size_t)f * FS_TRI + 9]);
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

__global__ __launch_bounds__(FS_BLOCK) void freespace_fwd_kernel(const float *__restrict__ ends, const int32_t *__restrict__ frame,
                                                                 const float *__restrict__ origins, uint32_t Nr, int Nf, int M, int draw, uint64_t seed,
                                                                 uint64_t step, const float *__restrict__ tri, const float *__restrict__ boxes,
                                                                 const int32_t *__restrict__ face_group, const int32_t *__restrict__ group_keep,
                                                                 const float *__restrict__ vert_alpha, int A, int F, int G, float tau, float margin,
                                                                 int cull, float4 *__restrict__ records, float *__restrict__ psi_out,
                                                                 double *__restrict__ partial) {
    __shared__ double red[dbw::LOSS_WAVES][1];
    const int i = blockIdx.x * FS_BLOCK + threadIdx.x;
    const bool live = i < M;
    FreespaceRay ray;
#pragma unroll
    for (int k = 0; k < 3; ++k) { ray.o[k] = 0.f; ray.e[k] = 0.f; }
    if (live) ray = freespace_ray(ends, frame, origins, Nr, Nf, draw, seed, step, (uint32_t)i);
    unsigned long long best = ~0ull;
    float best_t = 1.f, bu = 0.f, bv = 0.f;
    for (int g = 0; g < G; ++g) {
        if (group_keep && !group_keep[g]) continue;
        if (cull) {
            const float *b = boxes + g * 8;
            const float lo[3] = {b[0], b[1], b[2]}, hi[3] = {b[4], b[5], b[6]};
            const bool want = live && dbw::freespace_slab_reaches(lo, hi, ray.o, ray.e, best_t);
            if (__ballot(want) == 0ull) continue;
        }
        const int f0 = clampi(face_group[g], 0, F), f1 = clampi(face_group[g + 1], 0, F);
#pragma unroll 2
        for (int f = f0; f < f1; ++f) {
            const float *t = tri + (size_t)f * FS_TRI;              // wave-uniform address: scalar loads
            const float tt[9] = {t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]};
            const dbw::FreespaceHit h = dbw::freespace_hit(tt, ray.o[0], ray.o[1], ray.o[2], ray.e[0], ray.e[1], ray.e[2]);
            if (h.hit) {
                const unsigned long long key = dbw::freespace_key(h.t, (uint32_t)f);
                if (key < best) { best = key; best_t = h.t; bu = h.u; bv = h.v; }
            }
        }
    }
    double s = 0.0;
    if (live) s = freespace_emit(i, best, best_t, bu, bv, ray, tri, vert_alpha, A, tau, margin, records, psi_out);
    const double tsum = dbw::block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tsum;
}

__global__ __launch_bounds__(FS_BLOCK) void freespace_chunk_kernel(const float *__restrict__ ends, const int32_t *__restrict__ frame,
                                                                   const float *__restrict__ origins, uint32_t Nr, int Nf, int M, int draw,
                                                                   uint64_t seed, uint64_t step, const float *__restrict__ tri,
                                                                   const float *__restrict__ boxes, const int32_t *__restrict__ face_group,
                                                                   const int32_t *__restrict__ group_keep, int F, int G, int cull,
                                                                   unsigned long long *__restrict__ keys) {
    const int i = blockIdx.x * FS_BLOCK + threadIdx.x;
    const bool live = i < M;
    const int c0 = blockIdx.y * FS_CHUNK, c1 = c0 + FS_CHUNK < F ? c0 + FS_CHUNK : F;
    FreespaceRay ray;
#pragma unroll
    for (int k = 0; k < 3; ++k) { ray.o[k] = 0.f; ray.e[k] = 0.f; }
    if (live) ray = freespace_ray(ends, frame, origins, Nr, Nf, draw, seed, step, (uint32_t)i);
    unsigned long long best = ~0ull;
    float best_t = 1.f;
    for (int g = 0; g < G; ++g) {
        int f0 = clampi(face_group[g], 0, F), f1 = clampi(face_group[g + 1], 0, F);
        if (f0 >= c1) break;                                        // (face_group ascends: no later group reaches the chunk)
        f0 = f0 > c0 ? f0 : c0;
        f1 = f1 < c1 ? f1 : c1;
        if (f0 >= f1) continue;
        if (group_keep && !group_keep[g]) continue;
        if (cull) {
            const float *b = boxes + g * 8;
            const float lo[3] = {b[0], b[1], b[2]}, hi[3] = {b[4], b[5], b[6]};
            const bool want = live && dbw::freespace_slab_reaches(lo, hi, ray.o, ray.e, best_t);
            if (__ballot(want) == 0ull) continue;
        }
#pragma unroll 2
        for (int f = f0; f < f1; ++f) {
            const float *t = tri + (size_t)f * FS_TRI;              // wave-uniform address: scalar loads
            const float tt[9] = {t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]};
            const dbw::FreespaceHit h = dbw::freespace_hit(tt, ray.o[0], ray.o[1], ray.o[2], ray.e[0], ray.e[1], ray.e[2]);
            if (h.hit) {
                const unsigned long long key = dbw::freespace_key(h.t, (uint32_t)f);
                if (key < best) { best = key; best_t = h.t; }
            }
        }
    }
    if (live && best != ~0ull) atomicMin(keys + i, best);
}

__global__ __launch_bounds__(FS_BLOCK) void freespace_pick_kernel(const float *__restrict__ ends, const int32_t *__restrict__ frame,
                                                                  const float *__restrict__ origins, uint32_t Nr, int Nf, int M, int draw,
                                                                  uint64_t seed, uint64_t step, const float *__restrict__ tri,
                                                                  const unsigned long long *__restrict__ keys, const float *__restrict__ vert_alpha,
                                                                  int A, int F, float tau, float margin, float4 *__restrict__ records,
                                                                  float *__restrict__ psi_out, double *__restrict__ partial) {
    __shared__ double red[dbw::LOSS_WAVES][1];
    const int i = blockIdx.x * FS_BLOCK + threadIdx.x;
    double s = 0.0;
    if (i < M) {
        const FreespaceRay ray = freespace_ray(ends, frame, origins, Nr, Nf, draw, seed, step, (uint32_t)i);
        unsigned long long best = keys[i];
        float bt = 1.f, bu = 0.f, bv = 0.f;
        const uint32_t f = (uint32_t)(best & 0xffffffffull);
        if (best != ~0ull && f < (uint32_t)F) {
            const float *t = tri + (size_t)f * FS_TRI;
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

__global__ __launch_bounds__(FS_BLOCK) void freespace_bwd_kernel(const float *__restrict__ ends, const int32_t *__restrict__ frame,
                                                                 const float *__restrict__ origins, uint32_t Nr, int Nf, int M, int draw, uint64_t seed,
                                                                 uint64_t step, const float4 *__restrict__ records, const float *__restrict__ tri,
                                                                 const int32_t *__restrict__ faces, const float *__restrict__ vert_alpha, int A, int F,
                                                                 int V, int seg_len, float tau, float margin, double *__restrict__ part) {
    const int v = blockIdx.y * FS_BLOCK + threadIdx.x;
    const long long r0 = (long long)blockIdx.x * seg_len;
    const int r1 = (int)(r0 + seg_len < M ? r0 + seg_len : M);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int r = (int)r0; r < r1; ++r) {
        const float4 rec = records[r];                              // uniform across the workgroup
        const int f = __float_as_int(rec.y);
        if (f < 0 || f >= F) continue;
        int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
        i0 = (i0 >= 0 && i0 < V) ? i0 : 0; i1 = (i1 >= 0 && i1 < V) ? i1 : 0; i2 = (i2 >= 0 && i2 < V) ? i2 : 0;      // (as surface_box_kernel reads them)
        const bool m0 = v == i0, m1 = v == i1, m2 = v == i2;
        if (__ballot(m0 || m1 || m2) == 0ull) continue;
        const FreespaceRay ray = freespace_ray(ends, frame, origins, Nr, Nf, draw, seed, step, (uint32_t)r);
        const float l = dbw::freespace_length(ray.e[0], ray.e[1], ray.e[2]);
        const float g = dbw::freespace_g(rec.x, l, margin);
        if (!(g > 0.f)) continue;
        const float *t = tri + (size_t)f * FS_TRI;
        const double e1[3] = {(double)(t[3] - t[0]), (double)(t[4] - t[1]), (double)(t[5] - t[2])};
        const double e2[3] = {(double)(t[6] - t[0]), (double)(t[7] - t[1]), (double)(t[8] - t[2])};
        const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double ne = (n[0] * (double)ray.e[0] + n[1] * (double)ray.e[1]) + n[2] * (double)ray.e[2];
        if (ne == 0.0) continue;
        int row;
        const double a = (double)freespace_face_alpha(tri, f, vert_alpha, A, row);
        const double wts = (m0 ? (double)((1.f - rec.z) - rec.w) : 0.0) + (m1 ? (double)rec.z : 0.0) + (m2 ? (double)rec.w : 0.0);
        const double coef = -(a * 2.0 * (double)(g < tau ? g : tau) * (double)l * wts) / ne;
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] += coef * n[k];
    }
    if (v < V) {
        double *o = part + ((size_t)blockIdx.x * V + v) * 3;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
    }
}

// scale = weight / M, times grad_out[0] (1 without one)
__global__ __launch_bounds__(FS_BLOCK) void freespace_bwd_finish_kernel(const double *__restrict__ part, int segs, int V, double scale,
                                                                        const float *__restrict__ grad_out, float *__restrict__ grad_verts) {
    const int v = blockIdx.x * FS_BLOCK + threadIdx.x;
    if (v >= V) return;
    const double go = grad_out ? (double)grad_out[0] : 1.0;
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < segs; ++b) {
        const double *p = part + ((size_t)b * V + v) * 3;
        s[0] += p[0]; s[1] += p[1]; s[2] += p[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) grad_verts[(size_t)v * 3 + c] = (float)((s[c] * scale) * go);
}

__global__ __launch_bounds__(FS_BLOCK) void freespace_alpha_kernel(const float4 *__restrict__ records, const float *__restrict__ psi,
                                                                   const float *__restrict__ tri, int M, int F, double scale,
                                                                   const float *__restrict__ grad_out, float *__restrict__ grad_alpha) {
    __shared__ double red[dbw::LOSS_WAVES][1];
    const int k = blockIdx.x;
    double s = 0.0;
    for (int r = threadIdx.x; r < M; r += FS_BLOCK) {
        const int f = __float_as_int(records[r].y);
        if (f >= 0 && f < F && __float_as_int(tri[(size_t)f * FS_TRI + 9]) == k) s += (double)psi[r];
    }
    const double t = dbw::block_sum(s, red);
    if (threadIdx.x == 0) grad_alpha[k] = (float)(t * scale * (grad_out ? (double)grad_out[0] : 1.0));
}

}  // namespace

extern "C" size_t dbw_eval_freespace_workspace_bytes(int64_t M, int F, int V, int G, int segment) {
    return freespace_sizes_ok(M, F, V, G, segment) ? freespace_layout(M, F, V, G, segment).total : 0;
}

#define FREESPACE_COMMON_CHECKS                                                                                                            \
    DBW_REQUIRE(Nr >= 1 && Nr < (1ll << 31), "Nr must be in [1, 2^31)");                                                                   \
    DBW_REQUIRE(Nf >= 1 && Nf <= FS_MAX_FRAMES, "Nf must be in [1, 2^20]");                                                                \
    DBW_REQUIRE(n_rays >= 0 && n_rays <= FS_MAX_M && (n_rays > 0 || Nr <= FS_MAX_M), "the rays of a step (n_rays, or Nr when it is 0) must be in [1, 2^24]"); \
    DBW_REQUIRE(F >= 1 && F <= FS_MAX_F, "F must be in [1, 2^20]");                                                                        \
    DBW_REQUIRE(V >= 1 && V <= FS_MAX_V, "V must be in [1, 2^21]");                                                                        \
    DBW_REQUIRE(G >= 1 && G <= FS_MAX_G, "G must be in [1, 4096]");                                                                        \
    DBW_REQUIRE(tau > 0.f && tau < INFINITY, "tau must be positive and finite");                                                           \
    DBW_REQUIRE(margin >= 0.f && margin < INFINITY, "margin must be non-negative and finite");                                             \
    DBW_REQUIRE(A >= 0 && A <= V, "A must be in [0, V]");                                                                                  \
    DBW_REQUIRE(A == 0 || vert_alpha, "A >= 1 needs vert_alpha");                                                                          \
    DBW_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace is not 16-byte aligned");                                                     \
    DBW_REQUIRE(((uintptr_t)records & 15) == 0, "records are not 16-byte aligned")

extern "C" int dbw_eval_freespace_fwd(const float *ends, const int32_t *frame, const float *origins, int64_t Nr, int Nf, int64_t n_rays, int64_t seed,
                                      int64_t step, const float *verts, int V, const int32_t *faces, const int32_t *faces_host, int F,
                                      const int32_t *face_group, const int32_t *group_keep, const int32_t *group_alpha, int G, const float *vert_alpha,
                                      int A, float tau, float margin, int cull, int layout, void *workspace, void *records, double *value, dbw_stream_t stream) {
    DBW_REQUIRE(ends && frame && origins && verts && faces && face_group && group_alpha && workspace && records && value, "null pointer");
    FREESPACE_COMMON_CHECKS;
    DBW_REQUIRE(cull == 0 || cull == 1, "cull must be 0 or 1");
    DBW_REQUIRE(layout >= 0 && layout <= 2, "layout must be 0, 1 or 2");
    DBW_REQUIRE(((uintptr_t)ends & 3) == 0 && ((uintptr_t)frame & 3) == 0 && ((uintptr_t)origins & 3) == 0 && ((uintptr_t)verts & 3) == 0 &&
                    ((uintptr_t)faces & 3) == 0 && ((uintptr_t)faces_host & 3) == 0 && ((uintptr_t)face_group & 3) == 0 &&
                    ((uintptr_t)group_keep & 3) == 0 && ((uintptr_t)group_alpha & 3) == 0 && ((uintptr_t)vert_alpha & 3) == 0 &&
                    ((uintptr_t)value & 7) == 0,
                "misaligned pointer");
    if (faces_host) {
        for (int64_t k = 0; k < (int64_t)F * 3; ++k) DBW_REQUIRE(faces_host[k] >= 0 && faces_host[k] < V, "a face index is outside [0, V)");
    }
    const int64_t M = n_rays ? n_rays : Nr;
    const hipStream_t st = (hipStream_t)stream;
    const FreespaceLayout L = freespace_layout(M, F, V, G, 0);   // (the backward's partials come last: the offsets before them do not depend on the segment)
    char *ws = (char *)workspace;
    float *boxes = (float *)(ws + L.boxes), *tri = (float *)(ws + L.tri), *psi = (float *)(ws + L.psi);
    double *fwd_part = (double *)(ws + L.fwd_part);

    int rc = dbw_surface_box_launch(verts, V, faces, F, face_group, group_keep, G, tri, boxes, st);
    if (rc) return rc;
    hipLaunchKernelGGL(freespace_tag_kernel, dim3((unsigned)G), dim3(FS_BLOCK), 0, st, face_group, group_alpha, F, tri);
    if ((rc = dbw_check_launch("freespace_tag_kernel"))) return rc;
    if (layout == 1) {
        hipLaunchKernelGGL(freespace_fwd_kernel, dim3((unsigned)L.fwd_groups), dim3(FS_BLOCK), 0, st, ends, frame, origins, (uint32_t)Nr, Nf, (int)M,
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
        hipLaunchKernelGGL(freespace_chunk_kernel, dim3((unsigned)L.fwd_groups, chunks), dim3(FS_BLOCK), 0, st, ends, frame, origins, (uint32_t)Nr, Nf,
                           (int)M, n_rays ? 1 : 0, (uint64_t)seed, (uint64_t)step, (const float *)tri, (const float *)boxes, face_group, group_keep, F, G,
                           cull, keys);
        if ((rc = dbw_check_launch("freespace_chunk_kernel"))) return rc;
        hipLaunchKernelGGL(freespace_pick_kernel, dim3((unsigned)L.fwd_groups), dim3(FS_BLOCK), 0, st, ends, frame, origins, (uint32_t)Nr, Nf, (int)M,
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
    FREESPACE_COMMON_CHECKS;
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
    const FreespaceLayout L = freespace_layout(M, F, V, G, segment);
    const int seg_len = segment ? segment : dbw::FREESPACE_SEGMENT;
    char *ws = (char *)workspace;
    const double scale = (double)weight / (double)M;
    double *part = (double *)(ws + L.bwd_part);
    const float *tri = (const float *)(ws + L.tri);

    hipLaunchKernelGGL(freespace_bwd_kernel, dim3((unsigned)L.segs, (unsigned)L.vert_groups), dim3(FS_BLOCK), 0, st, ends, frame, origins, (uint32_t)Nr,
                       Nf, (int)M, n_rays ? 1 : 0, (uint64_t)seed, (uint64_t)step, (const float4 *)records, tri, faces, vert_alpha, A, F, V, seg_len, tau,
                       margin, part);
    int rc = dbw_check_launch("freespace_bwd_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(freespace_bwd_finish_kernel, dim3((unsigned)L.vert_groups), dim3(FS_BLOCK), 0, st, (const double *)part, L.segs, V, scale, grad_out,
                       grad_verts);
    if ((rc = dbw_check_launch("freespace_bwd_finish_kernel"))) return rc;
    if (grad_alpha && A >= 1) {
        hipLaunchKernelGGL(freespace_alpha_kernel, dim3((unsigned)A), dim3(FS_BLOCK), 0, st, (const float4 *)records, (const float *)(ws + L.psi), tri,
                           (int)M, F, scale, grad_out, grad_alpha);
        if ((rc = dbw_check_launch("freespace_alpha_kernel"))) return rc;
    }
    return 0;
}
