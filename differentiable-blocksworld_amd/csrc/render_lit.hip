// Lit visualisation renders (include/dbw_viz.h): a directional light fixed to the camera, flat or Phong shading (light_math.h), forward
// only.  The reference draws everything a user looks at through such a renderer (`renderer_light`, dbw.py:139-143; the eye_light variants
// of render_views / render_rotated_views), always at 4x the image size with a 4x4 box filter behind it (renderer.py:56-60,178-183).
//
// render_lit_kernel is the fused forward's generic path -- the same per-face set-up and bins (dbw_prepare_raster), the same raster_tile,
// decode_frag / footprint / fetch and layered blend, unchanged -- with two differences: the texel is multiplied by the light's gain in
// front of the blend, and NOTHING is kept for a backward: no fragments are stored, and with SSAA == 4 the 4x4 super-samples of an
// output pixel are averaged in registers, so that the pass writes 16 B per OUTPUT pixel and nothing else.
#include "raster_common.h"
#include "shade_common.h"
#include "light_math.h"
#include "../../include/dbw_viz.h"

#include <math.h>

using namespace dbw;

// implemented in raster.hip / shade_blend.hip
int dbw_prepare_raster(const float *face_verts, const int *first_idx, const int *num_faces, const int *neighbor, int N, long long F_total,
                       long long max_faces_per_view, int H, int W, float margin, int cull, void *workspace, size_t workspace_bytes,
                       dbw::CoarseBins &cb, hipStream_t s, bool launch, bool want_cells);
const dbw::FaceRec *dbw_workspace_recs(const void *workspace, long long F_total);
int dbw_fill_shade_args(ShadeArgs &A, const int32_t *pix_to_face, const float *bary, const float *dists, const int32_t *c2o,
                        const int32_t *clip_code, const float *clip_w, int Fc_stride, const float *face_uvs,
                        const int32_t *face_map, const int32_t *map_desc, const float *maps, const float *faces_alpha,
                        int alpha_len, int N, int H, int W, int K, int F, float sigma, const float *background3);

namespace {

struct LitArgs {
    const float4 *gain;       // (N, F): flat shading, the three gains of every (view, original face); nullptr: Phong
    const float4 *ldir;       // (N): the view's unit direction to the light
    const int *faces;         // (F, 3)
    const float *vn;          // (V, 3) vertex normals (Phong)
    float ka[3], kd[3];
};

// ---- vertex normals: a gather over the vertex -> (face, corner) adjacency ---------------------------------------------------------------
__global__ void vertex_normals_kernel(const float *__restrict__ verts, const int *__restrict__ faces, const int *__restrict__ adj_start,
                                      const int *__restrict__ adj, int V, int F, float *__restrict__ normals) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    f3 s{0.f, 0.f, 0.f};
    const int e0 = adj_start[v], e1 = adj_start[v + 1];
    for (int e = e0; e < e1; ++e) {
        const int a = adj[e], f = a >> 2, corner = a & 3;
        if (f < 0 || f >= F || corner > 2) continue;            // (a malformed entry contributes nothing and reads nothing)
        const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
        if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) continue;
        const f3 c = corner_cross(verts + i0 * 3, verts + i1 * 3, verts + i2 * 3, corner);
        s.x += c.x; s.y += c.y; s.z += c.z;
    }
    const f3 n = light_normalize(s);
    normals[v * 3] = n.x; normals[v * 3 + 1] = n.y; normals[v * 3 + 2] = n.z;
}

// ---- per (view, original face): the view's unit light direction and, for flat shading, the face's three gains --------------------------
__global__ void light_setup_kernel(const float *__restrict__ verts, const int *__restrict__ faces, const float *__restrict__ ldir_world, int N, int F,
                                   LitArgs L, float4 *__restrict__ ldir_out, float4 *__restrict__ gain_out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)N * F) return;
    const int n = (int)(idx / F), j = (int)(idx - (long long)n * F);
    f3 d{ldir_world[n * 3], ldir_world[n * 3 + 1], ldir_world[n * 3 + 2]};
    d = light_normalize(d);
    if (j == 0) ldir_out[n] = make_float4(d.x, d.y, d.z, 0.f);
    if (gain_out) {
        const int i0 = faces[j * 3], i1 = faces[j * 3 + 1], i2 = faces[j * 3 + 2];
        const f3 nf = face_normal(verts + (long long)i0 * 3, verts + (long long)i1 * 3, verts + (long long)i2 * 3);
        float g[3];
        light_gain(nf, d, L.ka, L.kd, g);
        gain_out[idx] = make_float4(g[0], g[1], g[2], 0.f);
    }
}

// ---- shading + blend of one pixel's list, lit ---------------------------------------------------------------------------------------------
template <int KMAX, int NT>
__device__ __forceinline__ void shade_lit(const ShadeArgs &A, const LitArgs &L, const TopK<KMAX> &q, const pay4 *home, int n, float (&px)[4]) {
    BlendFront bl;
    blend_front_init(bl);
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k < A.K) {
            float pzk = -1.f;
            int fik = -1;
            pay4 v{-1.f, -1.f, -1.f, -1.f};
            if (q.get(k, home, NT, threadIdx.x, pzk, fik, v)) {
                Frag fr;
                const float bc[3] = {v.y, v.z, v.w};
                decode_frag(A, n, fik, bc, v.x, fr);
                const float a = fr.e * fr.fa;
                if (a != 0.f) {
                    Sample s;
                    footprint(A, fr, s);
                    float c[3], g[3];
                    fetch(A.maps, s, c);
                    if (L.vn == nullptr) {          // flat: one 16 B record per (view, face)
                        const float4 g4 = L.gain[(long long)n * A.F + fr.j];
                        g[0] = g4.x; g[1] = g4.y; g[2] = g4.z;
                    } else {                        // Phong: the vertex normals at the fragment's barycentrics w.r.t. the original face
                        const int *fv = L.faces + (long long)fr.j * 3;
                        const float4 d4 = L.ldir[n];
                        const f3 nn = phong_normal(fr.bo, L.vn + (long long)fv[0] * 3, L.vn + (long long)fv[1] * 3, L.vn + (long long)fv[2] * 3);
                        light_gain(nn, f3{d4.x, d4.y, d4.z}, L.ka, L.kd, g);
                    }
                    c[0] *= g[0]; c[1] *= g[1]; c[2] *= g[2];
                    blend_front_step(bl, a, c);
                }
            }
        }
    }
    blend_front_finish(bl, A.bg, px);
}

// the sum over the 4x4 pixel block of this lane, in every lane of the block.  16x16 tiles: a wave owns 16x4 pixels (raster_common.h), lane
// = (y & 3) * 16 + (x & 15), so the block's other pixels are lanes ^ 1, ^ 2 (the quad: DPP) and ^ 16, ^ 32 (the rows: lane permutes).  No
// LDS memory, no barrier.
__device__ __forceinline__ float block4x4_sum(float v) {
    v = quad_sum(v);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// A.H, A.W: the RENDER size (SSAA times the image's)
template <int KMAX, int SSAA>
__global__ __launch_bounds__(KMAX == 1 ? 256 : 64, DBW_RASTER_WAVES(KMAX)) void render_lit_kernel(const FaceRec *__restrict__ recs, const float4 *__restrict__ bbox,
                                                             const int *__restrict__ first_idx, const int *__restrict__ num_faces, float blur,
                                                             int persp, long long total_blocks, ShadeArgs A, CoarseBins cb, LitArgs L,
                                                             float *__restrict__ image) {
    static_assert(SSAA == 1 || (SSAA == 4 && KMAX == 1), "the in-register 4x4 resolve belongs to the 16x16 tiles of the hard pass");
    constexpr int TW = KMAX == 1 ? 16 : 8, TH = TW, GROUP = KMAX == 1 ? 1 : 2;
    int n, xi, yi;
    TopK<KMAX> q;
    pay4 *home;
    // (dbg bit 3: a hard single-layer pass reads its distances for their sign only, like the fused forward's)
    if (!raster_tile<KMAX, TW, TH, GROUP, false>(recs, bbox, first_idx, num_faces, A.H, A.W, A.K, blur, persp, 1, total_blocks, cb,
                                                 (KMAX == 1 && A.sigma == 0.f) ? 8 : 0, n, xi, yi, q, home)) return;
    const bool in_img = xi < A.W && yi < A.H;
    float px[4] = {0.f, 0.f, 0.f, 0.f};
    if (in_img) shade_lit<KMAX, TW * TH>(A, L, q, home, n, px);
    if constexpr (SSAA == 1) {
        if (in_img) {
            const long long plane = (long long)A.H * A.W;
            float *out = image + (long long)n * 4 * plane + (long long)yi * A.W + xi;
            out[0] = px[0]; out[plane] = px[1]; out[2 * plane] = px[2]; out[3 * plane] = px[3];
        }
    } else {
        // 4H and 4W are multiples of 4: a block lies wholly inside or wholly outside the image, and one lane in 16 stores it
#pragma unroll
        for (int c = 0; c < 4; ++c) px[c] = block4x4_sum(px[c]) * 0.0625f;
        if (in_img && (threadIdx.x & 3) == 0 && (threadIdx.x & 48) == 0) {
            const int Ho = A.H >> 2, Wo = A.W >> 2;
            const long long plane = (long long)Ho * Wo;
            float *out = image + (long long)n * 4 * plane + (long long)(yi >> 2) * Wo + (xi >> 2);
            out[0] = px[0]; out[plane] = px[1]; out[2 * plane] = px[2]; out[3 * plane] = px[3];
        }
    }
}

template <int KMAX, int SSAA>
int launch_lit(const FaceRec *recs, const float4 *bbox, const int *first_idx, const int *num_faces, float blur, int persp, const ShadeArgs &A,
               const CoarseBins &cb, const LitArgs &L, float *image, hipStream_t s) {
    constexpr int T = KMAX == 1 ? 16 : 8;
    const long long total = (long long)A.N * ((A.W + T - 1) / T) * ((A.H + T - 1) / T);
    DBW_REQUIRE(total < (1LL << 31) - 8, "more than 2^31 tiles in one pass");
    hipLaunchKernelGGL((render_lit_kernel<KMAX, SSAA>), dim3(dbw_xcd_grid(total)), dim3(T * T), 0, s, recs, bbox, first_idx, num_faces, blur, persp,
                       total, A, cb, L, image);
    return dbw_check_launch("render_lit_kernel");
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

bool lit_sizes_ok(int64_t F_total, int N, int F, int H, int W, int ssaa) {
    return F_total >= 0 && N >= 0 && F > 0 && H > 0 && W > 0 && (ssaa == 1 || ssaa == 4) && (long long)H * ssaa < (1 << 24) && (long long)W * ssaa < (1 << 24) &&
           (long long)N * F < (1LL << 31);
}

}  // namespace

extern "C" int dbw_viz_abi_version(void) { return DBW_VIZ_ABI_VERSION; }      // (history: include/dbw_viz.h)

extern "C" int dbw_vertex_normals(const float *verts, const int32_t *faces, const int32_t *adj_start, const int32_t *adj, int V, int F, float *normals,
                                  dbw_stream_t stream) {
    DBW_REQUIRE(verts && faces && adj_start && adj && normals, "null pointer");
    DBW_REQUIRE(V > 0 && F > 0 && (long long)V * 3 < (1LL << 31) && (long long)F * 4 < (1LL << 31), "bad size");
    hipLaunchKernelGGL(vertex_normals_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, (hipStream_t)stream, verts, faces, adj_start, adj, V, F, normals);
    return dbw_check_launch("vertex_normals_kernel");
}

// workspace = [the rasteriser's binned workspace at the render size][unit light directions: N x 16 B][flat gains: N * F x 16 B]
extern "C" size_t dbw_render_lit_workspace_bytes(int64_t F_total, int N, int F, int H, int W, int ssaa) {
    if (!lit_sizes_ok(F_total, N, F, H, W, ssaa)) return 0;
    return dbw_rasterize_workspace_bytes_binned(F_total, N, H * ssaa, W * ssaa) + align256((size_t)(N > 0 ? N : 1) * sizeof(float4)) +
           align256((size_t)(N > 0 ? N : 1) * (size_t)F * sizeof(float4));
}

extern "C" int dbw_render_lit_fwd(const float *face_verts_c, const int32_t *first_idx, const int32_t *num_faces, const int32_t *neighbor,
                                  const int32_t *c2o, const int32_t *clip_code, const float *clip_w, int Fc_stride, const float *face_uvs,
                                  const int32_t *face_map, const int32_t *map_desc, const float *maps, const float *faces_alpha, int alpha_len,
                                  const float *verts_world, const int32_t *faces, const float *vert_normals, const float *light_dir_world,
                                  const float *ambient3, const float *diffuse3, int N, int64_t F_total, int H, int W, int K, int F, float sigma,
                                  float blur_radius, int perspective_correct, const float *background3, int ssaa, float *image, void *workspace,
                                  size_t workspace_bytes, dbw_stream_t stream) {
    DBW_REQUIRE(face_verts_c && first_idx && num_faces && verts_world && faces && light_dir_world && ambient3 && diffuse3 && image && workspace, "null pointer");
    DBW_REQUIRE(ssaa == 1 || ssaa == 4, "ssaa must be 1 or 4");
    DBW_REQUIRE(lit_sizes_ok(F_total, N, F, H, W, ssaa), "bad size");
    DBW_REQUIRE(blur_radius >= 0.f, "bad blur_radius");
    if (K > DBW_MAX_FACES_PER_PIXEL) {
        dbw_set_error("dbw_render_lit_fwd: faces_per_pixel=%d > %d", K, DBW_MAX_FACES_PER_PIXEL);
        return DBW_ERR_UNSUPPORTED;
    }
    if (ssaa == 4 && K != 1) {
        dbw_set_error("dbw_render_lit_fwd: ssaa == 4 resolves its 4x4 blocks on the 16x16 tiles of the single-layer pass: faces_per_pixel must be 1, got %d", K);
        return DBW_ERR_UNSUPPORTED;
    }
    const int rH = H * ssaa, rW = W * ssaa;
    DBW_REQUIRE(workspace_bytes >= dbw_render_lit_workspace_bytes(F_total, N, F, H, W, ssaa), "workspace too small");
    ShadeArgs A;
    // (the pass keeps no fragments: the three fragment pointers of ShadeArgs are never read by render_lit_kernel; the workspace stands in
    // for them where the shared argument check asks for non-null pointers)
    int rc = dbw_fill_shade_args(A, (const int32_t *)workspace, (const float *)workspace, (const float *)workspace, c2o, clip_code, clip_w, Fc_stride,
                                 face_uvs, face_map, map_desc, maps, faces_alpha, alpha_len, N, rH, rW, K, F, sigma, background3);
    if (rc) return rc;
    if (N == 0) return DBW_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t raster_bytes = dbw_rasterize_workspace_bytes_binned(F_total, N, rH, rW);
    float4 *ldir = (float4 *)((char *)workspace + raster_bytes);
    float4 *gain = (float4 *)((char *)ldir + align256((size_t)N * sizeof(float4)));
    LitArgs L;
    L.gain = vert_normals ? nullptr : gain; L.ldir = ldir; L.faces = faces; L.vn = vert_normals;
    for (int i = 0; i < 3; ++i) { L.ka[i] = ambient3[i]; L.kd[i] = diffuse3[i]; }
    CoarseBins cb;
    rc = dbw_prepare_raster(face_verts_c, first_idx, num_faces, neighbor, N, F_total, c2o ? (long long)Fc_stride : F_total, rH, rW,
                            (float)sqrt((double)blur_radius), 0, workspace, raster_bytes, cb, s, /*launch=*/true, /*want_cells: the 8x8-tile kernels*/ K > 1);
    if (rc) return rc;
    {
        const long long nthreads = (long long)N * F;
        hipLaunchKernelGGL(light_setup_kernel, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, s, verts_world, faces, light_dir_world, N, F, L, ldir,
                           vert_normals ? (float4 *)nullptr : gain);
        rc = dbw_check_launch("light_setup_kernel");
        if (rc) return rc;
    }
    const float4 *bbox = (const float4 *)workspace;
    const FaceRec *recs = dbw_workspace_recs(workspace, F_total);
#define DBW_LIT(KM, SS) launch_lit<KM, SS>(recs, bbox, first_idx, num_faces, blur_radius, perspective_correct, A, cb, L, image, s)
    if (K == 1) return ssaa == 4 ? DBW_LIT(1, 4) : DBW_LIT(1, 1);
    if (K <= 4) return DBW_LIT(4, 1);
    if (K <= 10) return DBW_LIT(10, 1);
    if (K <= 16) return DBW_LIT(16, 1);
    return DBW_LIT(25, 1);
#undef DBW_LIT
}
