// The schedule that the terms on the posed meshes share (csrc/surface_term.hip, csrc/freespace_term.hip): HIP only.  A term measures M
// samples (points, rays) against F gathered faces in G groups and leaves one 16-byte record a sample (x: the term's measure, y: the face,
// z, w: the barycentrics u, v of the hit); its backward turns the records into vertex gradients.  What is here exists once:
//   MeshLayout         the workspace: boxes (G, 8 floats), tri (F, MESH_TRI floats: surface_box.h), the forward's partials (one double a
//                      workgroup of MESH_BLOCK samples), whatever regions the term adds, and LAST the backward's partials [segment][V][3]
//                      (their size alone depends on the segment length), with the three grid sizes
//   mesh_group_walk    forward: a lane holds a sample, the groups are walked in order; group and face are wave-uniform, so box and face
//                      coordinates arrive by scalar loads.  The visitor tests a group's box and takes every face of the range.
//   mesh_bwd_walk      backward, grid (segment, MESH_BLOCK vertices): a workgroup walks its segment of the records in index order, the record
//                      uniform across the workgroup; a thread whose vertex is a corner of the record's face lets the term add to its fp64
//                      sum.  A wave none of whose vertices is a corner does no arithmetic for the record.
//   mesh_segment_sum   the segments' partials of a vertex added in segment order
//   MESH_COMMON_CHECKS, mesh_faces_inside: what the entry points of every term refuse
// No MFMA, no floating-point atomics, no cross-workgroup waiting: plain launches on the caller's stream, kernel boundaries the only
// ordering, nothing read by the host.  The grids depend on the sizes alone and every sum has one order: the same call gives the same bytes.
#pragma once
#include "dbw_common.h"
#include "loss_reduce.h"

namespace dbw {

constexpr int MESH_BLOCK = LOSS_THREADS;
constexpr int MESH_TRI = 12;                    // floats a gathered face takes
constexpr int MESH_MAX_G = 4096, MESH_MAX_F = 1 << 20, MESH_MAX_V = 1 << 21, MESH_MAX_M = 1 << 24, MESH_MAX_SEGS = 65535;

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

inline bool mesh_sizes_ok(int64_t M, int F, int V, int G, int segment, int default_segment) {
    if (!(M >= 1 && M <= MESH_MAX_M && F >= 1 && F <= MESH_MAX_F && V >= 1 && V <= MESH_MAX_V && G >= 1 && G <= MESH_MAX_G)) return false;
    if (segment < 0) return false;
    const int64_t L = segment ? segment : default_segment;
    return (M + L - 1) / L <= MESH_MAX_SEGS;
}

struct MeshLayout {             // byte offsets into the workspace
    size_t boxes, tri, fwd_part, bwd_part, total;
    int fwd_groups, vert_groups, segs;

    MeshLayout(int64_t M, int F, int V, int G, int segment, int default_segment) : total(0) {
        const int64_t seg = segment ? segment : default_segment;
        fwd_groups = (int)((M + MESH_BLOCK - 1) / MESH_BLOCK);
        vert_groups = (V + MESH_BLOCK - 1) / MESH_BLOCK;
        segs = (int)((M + seg - 1) / seg);
        boxes = add((size_t)G * 8 * sizeof(float));
        tri = add((size_t)F * MESH_TRI * sizeof(float));
        fwd_part = add((size_t)fwd_groups * sizeof(double));
        bwd_part = 0;
    }
    size_t add(size_t bytes) {  // a term's own region, 16-byte aligned -> its offset
        const size_t at = total;
        total = align16(total + bytes);
        return at;
    }
    void close(int V) { bwd_part = add((size_t)segs * V * 3 * sizeof(double)); }       // after the term's regions
};

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// The faces [c0, c1) (the whole mesh: [0, F)) group by group.  A group is skipped when the range holds none of its faces, when it is not
// kept, or (cull) when NO live lane's vis.reaches(lo, hi) holds for its box; face_group ascends, so no group after one that begins at or
// beyond c1 reaches the range.  Visitor: bool reaches(const float lo[3], const float hi[3]) const; void face(const float tt[9], int f).
template <class Visitor>
__device__ __forceinline__ void mesh_group_walk(const float *__restrict__ tri, const float *__restrict__ boxes, const int32_t *__restrict__ face_group,
                                                const int32_t *__restrict__ group_keep, int F, int G, int c0, int c1, int cull, bool live,
                                                Visitor &vis) {
    for (int g = 0; g < G; ++g) {
        int f0 = clampi(face_group[g], 0, F), f1 = clampi(face_group[g + 1], 0, F);
        if (f0 >= c1) break;
        f0 = f0 > c0 ? f0 : c0;
        f1 = f1 < c1 ? f1 : c1;
        if (f0 >= f1) continue;
        if (group_keep && !group_keep[g]) continue;
        if (cull) {
            const float *b = boxes + g * 8;
            const float lo[3] = {b[0], b[1], b[2]}, hi[3] = {b[4], b[5], b[6]};
            const bool want = live && vis.reaches(lo, hi);
            if (__ballot(want) == 0ull) continue;
        }
#pragma unroll 2
        for (int f = f0; f < f1; ++f) {
            const float *t = tri + (size_t)f * MESH_TRI;            // wave-uniform address: scalar loads
            const float tt[9] = {t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]};
            vis.face(tt, f);
        }
    }
}

// Segment blockIdx.x of the records against the vertices of blockIdx.y; partials [segment][V][3].  A face's vertex indices are clamped to
// [0, V), read as vertex 0, as the gather read them.  The term gives two functions: bool gate(rec), false for a record it skips unseen,
// and void add(int r, rec, int f, const float *t, double wts, double acc[3]) with t the gathered face and wts the barycentric weight of
// the thread's corner(s).
template <class Gate, class Add>
__device__ __forceinline__ void mesh_bwd_walk(const float4 *__restrict__ records, const float *__restrict__ tri, const int32_t *__restrict__ faces,
                                              int M, int F, int V, int seg_len, double *__restrict__ part, Gate gate, Add add) {
    const int v = blockIdx.y * MESH_BLOCK + threadIdx.x;
    const long long r0 = (long long)blockIdx.x * seg_len;
    const int r1 = (int)(r0 + seg_len < M ? r0 + seg_len : M);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int r = (int)r0; r < r1; ++r) {
        const float4 rec = records[r];                              // uniform across the workgroup
        if (!gate(rec)) continue;
        const int f = __float_as_int(rec.y);
        if (f < 0 || f >= F) continue;
        uint32_t i0 = (uint32_t)faces[f * 3], i1 = (uint32_t)faces[f * 3 + 1], i2 = (uint32_t)faces[f * 3 + 2];
        i0 = i0 < (uint32_t)V ? i0 : 0u; i1 = i1 < (uint32_t)V ? i1 : 0u; i2 = i2 < (uint32_t)V ? i2 : 0u;      // (as surface_box_kernel reads them: a negative index is a large one)
        const bool m0 = (uint32_t)v == i0, m1 = (uint32_t)v == i1, m2 = (uint32_t)v == i2;
        if (__ballot(m0 || m1 || m2) == 0ull) continue;
        const double wts = (m0 ? (double)((1.f - rec.z) - rec.w) : 0.0) + (m1 ? (double)rec.z : 0.0) + (m2 ? (double)rec.w : 0.0);
        add(r, rec, f, tri + (size_t)f * MESH_TRI, wts, acc);
    }
    if (v < V) {
        double *o = part + ((size_t)blockIdx.x * V + v) * 3;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
    }
}

__device__ __forceinline__ void mesh_segment_sum(const double *__restrict__ part, int segs, int V, int v, double s[3]) {
    s[0] = 0.0; s[1] = 0.0; s[2] = 0.0;
    for (int b = 0; b < segs; ++b) {
        const double *p = part + ((size_t)b * V + v) * 3;
        s[0] += p[0]; s[1] += p[1]; s[2] += p[2];
    }
}

inline bool mesh_faces_inside(const int32_t *faces_host, int F, int V) {
    int64_t k = 0;
    while (k < (int64_t)F * 3 && faces_host[k] >= 0 && faces_host[k] < V) ++k;
    return k == (int64_t)F * 3;
}

}  // namespace dbw

// F, V, G, tau, A, workspace, records of an entry point, by those names
#define MESH_COMMON_CHECKS                                                                                                                 \
    DBW_REQUIRE(F >= 1 && F <= dbw::MESH_MAX_F, "F must be in [1, 2^20]");                                                                 \
    DBW_REQUIRE(V >= 1 && V <= dbw::MESH_MAX_V, "V must be in [1, 2^21]");                                                                 \
    DBW_REQUIRE(G >= 1 && G <= dbw::MESH_MAX_G, "G must be in [1, 4096]");                                                                 \
    DBW_REQUIRE(tau > 0.f && tau < INFINITY, "tau must be positive and finite");                                                           \
    DBW_REQUIRE(A >= 0 && A <= V, "A must be in [0, V]");                                                                                  \
    DBW_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace is not 16-byte aligned");                                                     \
    DBW_REQUIRE(((uintptr_t)records & 15) == 0, "records are not 16-byte aligned")
