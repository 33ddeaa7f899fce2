// Host build (g++) of csrc/freespace_math.h for tests/test_host_freespace_math.py and tests/test_gpu_freespace.py: the same inline functions
// the kernels of csrc/freespace_term.hip compile, and host_freespace_records, the forward launch written as plain loops over them (HOST
// pointers, one ray at a time, the groups and faces in the kernel's order; `cull` is a ray's own slab test, which decides as a wave's does:
// never against a key that would win).
#include <math.h>
#include <string.h>

#include "../differentiable-blocksworld_amd/csrc/freespace_math.h"

using namespace dbw;

extern "C" {

// tri (n,9), o, e (n,3) -> out (n,4): hit (0 | 1), t, u, v
int host_freespace_hit(const float *tri, const float *o, const float *e, int64_t n, float *out) {
    for (int64_t i = 0; i < n; ++i) {
        const FreespaceHit h = freespace_hit(tri + i * 9, o[i * 3], o[i * 3 + 1], o[i * 3 + 2], e[i * 3], e[i * 3 + 1], e[i * 3 + 2]);
        out[i * 4] = h.hit ? 1.f : 0.f; out[i * 4 + 1] = h.t; out[i * 4 + 2] = h.u; out[i * 4 + 3] = h.v;
    }
    return 0;
}

// lo, hi, o, e (n,3), t_max (n) -> out (n): 1 where the slackened box is reached
int host_freespace_slab(const float *lo, const float *hi, const float *o, const float *e, const float *t_max, int64_t n, int32_t *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = freespace_slab_reaches(lo + i * 3, hi + i * 3, o + i * 3, e + i * 3, t_max[i]) ? 1 : 0;
    return 0;
}

uint32_t host_freespace_draw_index(uint64_t seed, uint64_t step, uint32_t i, uint32_t n_rays) { return freespace_draw_index(seed, step, i, n_rays); }

uint64_t host_freespace_key(float t, uint32_t face) { return freespace_key(t, face); }

float host_freespace_psi(float g, float tau) { return freespace_psi(g, tau); }

float host_freespace_g(float t, float l, float margin) { return freespace_g(t, l, margin); }

int host_freespace_segment(void) { return FREESPACE_SEGMENT; }

float host_freespace_graze(void) { return FREESPACE_GRAZE; }

// records (M,4) as 32-bit words: t, face, u, v -- what freespace_fwd_kernel writes.  psi (M) or NULL.
int host_freespace_records(const float *ends, const int32_t *frame, const float *origins, int64_t Nr, int Nf, int64_t n_rays, uint64_t seed,
                           uint64_t step, const float *verts, const int32_t *faces, const int32_t *face_group, const int32_t *group_keep, int G,
                           float tau, float margin, int cull, uint32_t *records, float *psi) {
    const int64_t M = n_rays ? n_rays : Nr;
    for (int64_t i = 0; i < M; ++i) {
        const int64_t j = n_rays ? (int64_t)freespace_draw_index(seed, step, (uint32_t)i, (uint32_t)Nr) : i;
        const float p[3] = {ends[j * 3], ends[j * 3 + 1], ends[j * 3 + 2]};
        const int fr = frame[j];
        float o[3] = {p[0], p[1], p[2]};
        if (fr >= 0 && fr < Nf)
            for (int k = 0; k < 3; ++k) o[k] = origins[(size_t)fr * 3 + k];
        const float e[3] = {p[0] - o[0], p[1] - o[1], p[2] - o[2]};
        uint64_t best = ~0ull;
        float best_t = 1.f, bu = 0.f, bv = 0.f;
        for (int g = 0; g < G; ++g) {
            if (group_keep && !group_keep[g]) continue;
            const int f0 = face_group[g], f1 = face_group[g + 1];
            if (cull) {
                float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
                for (int f = f0; f < f1; ++f)
                    for (int m = 0; m < 3; ++m)
                        for (int k = 0; k < 3; ++k) {
                            const float x = verts[(size_t)faces[f * 3 + m] * 3 + k];
                            lo[k] = x < lo[k] ? x : lo[k];
                            hi[k] = x > hi[k] ? x : hi[k];
                        }
                if (!freespace_slab_reaches(lo, hi, o, e, best_t)) continue;
            }
            for (int f = f0; f < f1; ++f) {
                float t[9];
                for (int m = 0; m < 3; ++m)
                    for (int k = 0; k < 3; ++k) t[m * 3 + k] = verts[(size_t)faces[f * 3 + m] * 3 + k];
                const FreespaceHit h = freespace_hit(t, o[0], o[1], o[2], e[0], e[1], e[2]);
                if (!h.hit) continue;
                const uint64_t key = freespace_key(h.t, (uint32_t)f);
                if (key < best) { best = key; best_t = h.t; bu = h.u; bv = h.v; }
            }
        }
        float ps = 0.f;
        if (best != ~0ull) {
            records[i * 4] = (uint32_t)(best >> 32);
            records[i * 4 + 1] = (uint32_t)(best & 0xffffffffull);
            memcpy(records + i * 4 + 2, &bu, 4);
            memcpy(records + i * 4 + 3, &bv, 4);
            ps = freespace_psi(freespace_g(best_t, freespace_length(e[0], e[1], e[2]), margin), tau);
        } else {
            records[i * 4] = 0x7fc00000u; records[i * 4 + 1] = 0xffffffffu; records[i * 4 + 2] = 0u; records[i * 4 + 3] = 0u;
        }
        if (psi) psi[i] = ps;
    }
    return 0;
}

}  // extern "C"
