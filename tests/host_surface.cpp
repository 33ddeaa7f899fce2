// Host build (g++) of csrc/surface_math.h for tests/test_host_surface_math.py and tests/test_gpu_surface.py: the same inline functions the
// kernels of csrc/surface_term.hip compile, and host_surface_records, the forward launch written as plain loops over them (HOST pointers, one
// point at a time, the groups and faces in the kernel's order; `cull` is a point's own box test, which decides as a wave's does: never against
// a key that would win).
#include <math.h>
#include <string.h>

#include "../differentiable-blocksworld_amd/csrc/surface_math.h"

using namespace dbw;

extern "C" {

// tri (n,9), p (n,3) -> out (n,3): d2, u, v
int host_surface_closest(const float *tri, const float *p, int64_t n, float *out) {
    for (int64_t i = 0; i < n; ++i) {
        const SurfaceHit h = surface_closest(tri + i * 9, p[i * 3], p[i * 3 + 1], p[i * 3 + 2]);
        out[i * 3] = h.d2; out[i * 3 + 1] = h.u; out[i * 3 + 2] = h.v;
    }
    return 0;
}

// lo, hi, p (n,3) -> out (n)
int host_surface_box_bound(const float *lo, const float *hi, const float *p, int64_t n, float *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = surface_box_bound(lo + i * 3, hi + i * 3, p[i * 3], p[i * 3 + 1], p[i * 3 + 2]);
    return 0;
}

uint32_t host_surface_draw_index(uint64_t seed, uint64_t step, uint32_t i, uint32_t n_cloud) { return surface_draw_index(seed, step, i, n_cloud); }

uint64_t host_surface_key(float d2, uint32_t face) { return surface_key(d2, face); }

float host_surface_rho(float d2, float tau2) { return surface_rho(d2, tau2); }

int host_surface_segment(void) { return SURFACE_SEGMENT; }

// records (M,4) as 32-bit words: d2, face, u, v -- what surface_fwd_kernel writes.  rho (M) or NULL.
int host_surface_records(const float *points, int64_t N, int64_t n_points, uint64_t seed, uint64_t step, const float *verts, int V,
                         const int32_t *faces, int F, const int32_t *face_group, const int32_t *group_keep, int G, float tau, int cull,
                         uint32_t *records, float *rho) {
    const int64_t M = n_points ? n_points : N;
    for (int64_t i = 0; i < M; ++i) {
        const int64_t j = n_points ? (int64_t)surface_draw_index(seed, step, (uint32_t)i, (uint32_t)N) : i;
        const float px = points[j * 3], py = points[j * 3 + 1], pz = points[j * 3 + 2];
        uint64_t best = ~0ull;
        float best_d2 = INFINITY, bu = 0.f, bv = 0.f;
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
                if (surface_box_bound(lo, hi, px, py, pz) > best_d2) continue;
            }
            for (int f = f0; f < f1; ++f) {
                float t[9];
                for (int m = 0; m < 3; ++m)
                    for (int k = 0; k < 3; ++k) t[m * 3 + k] = verts[(size_t)faces[f * 3 + m] * 3 + k];
                const SurfaceHit h = surface_closest(t, px, py, pz);
                const uint64_t key = surface_key(h.d2, (uint32_t)f);
                if (key < best) { best = key; best_d2 = h.d2; bu = h.u; bv = h.v; }
            }
        }
        const float d2 = surface_key_d2(best);
        records[i * 4] = (uint32_t)(best >> 32);
        records[i * 4 + 1] = (uint32_t)(best & 0xffffffffull);
        memcpy(records + i * 4 + 2, &bu, 4);
        memcpy(records + i * 4 + 3, &bv, 4);
        if (rho) rho[i] = surface_rho(d2, tau * tau);
    }
    (void)V;
    return 0;
}

}  // extern "C"
