// The hard single-layer pass's backward (sky + ground: K = 1, sigma = 0, no learned opacity): the body of render_bwd_hard_kernel
// (shade_blend.hip).  A kept pixel lies inside its face, its opacity is 1, nothing flows through the distance:
//   colour -> texels:  the footprint's texels, merged where they fall into one stored cell, the P pixels of a lane merged where they hit
//                      one cell, neighbouring pixels of one texel merged in registers (lane_merge), then the workgroup's LDS texel table
//                      (what does not fit goes straight to memory);
//   colour -> uv -> barycentrics -> vertices, only for faces whose vertices are variables (j >= geom_begin: the sky dome is a buffer),
//                      barycentrics rebuilt from the pixel position as the rasteriser backward does; gradient-only arithmetic on v_rcp_f32.
// Same mathematics as shade_blend_bwd_kernel<true, false, true>.
//
// A wave owns P 8x8 tiles (HardRegion: 2 x P/2 tiles per wave, 2 x 2 waves per workgroup), lane l pixel l of each.  The 7 P fragment and
// gradient loads of the wave are issued at its top, unconditionally and in one batch (every lane of a tile owns a slot in every plane; tiles
// outside the grid point at the view's first tile, pixels outside the image are masked on use with selects -- lanes without a fragment may
// read gradient words the forward never wrote, ShadeArgs::lean_grads), the map descriptors come from the workgroup's LDS copy
// (MapDescCache) instead of a per-lane gather, and the P pixels then go one after the other through the per-pixel backward.  The table
// clears, the barrier and the flush scans happen once per 4 P tiles.  Measured at config 2, epoch 0 (profiles/r07_experiments.md): alone
// 0.149 -> 0.116 ms with P = 2, step 0.770-0.795 -> 0.750-0.758 ms.  Batching the texel and face loads of the P pixels as well (two
// dependent memory levels per wave) needed 106-286 VGPRs -- 4 to 1 waves per SIMD instead of 8 -- and was slower at every P.
#pragma once
#include "shade_common.h"

namespace dbw {

// (a 64-slot texel table and a 32-slot face table: a 16x16-pixel tile of the magnified env maps touches a few cells and a handful of
// large faces; with the soft pass's 512 / 128 slots the clears, the flush scans and the lost residency cost a quarter of the kernel:
// 0.22 -> 0.16 ms with decimated maps, 0.31 -> 0.26 ms at full resolution; 16 slots and fewer overflow at full resolution (0.9 ms).
// Re-measured for the 32x16-pixel region of P = 2 (profiles/r07_experiments.md), alone at epoch 0 / epoch 800: 64 / 32 slots 115 / 213 us
// (parent 151 / 211), 128 / 32 119 / 199, 128 / 64 124 / 199, 256 / 64 125 / 204 -- the larger texel table pays at full resolution and
// costs as much on the decimated maps; the full-resolution phase's step is the parent's either way.  What does not fit goes straight to
// memory, as always)
#ifndef DBW_HARD_TEX_LOG2
#define DBW_HARD_TEX_LOG2 6
#endif
#ifndef DBW_HARD_FACE_LOG2
#define DBW_HARD_FACE_LOG2 5
#endif
typedef LdsAgg<3, DBW_HARD_TEX_LOG2> HardTexAgg;
typedef LdsAgg<9, DBW_HARD_FACE_LOG2> HardFaceAgg;      // a tile of the hard pass sees a handful of (large) faces

// 8x8 tiles per wave (1, 2 or 4)
#ifndef DBW_HARD_P
#define DBW_HARD_P 2
#endif
template <int P>
struct HardRegion {
    static_assert(P == 1 || P == 2 || P == 4, "tiles per wave: 1, 2 or 4");
    static constexpr int PX = P == 1 ? 1 : 2, PY = P / PX;      // a wave's block of tiles; tile p of it at (p % PX, p / PX)
    static constexpr int RX = 2 * PX, RY = 2 * PY;              // a workgroup's: 2 x 2 waves
    static long long blocks(int N, int H, int W) {
        const int tx = (W + 7) >> 3, ty = (H + 7) >> 3;
        return (long long)N * ((tx + RX - 1) / RX) * ((ty + RY - 1) / RY);
    }
};

// Backward of ONE pixel (valid: it holds a fragment -- clipped face fc, texture coordinates (u, v), jm = original face | map << 20 -- with
// colour gradient gc).  Wave-collective: every lane of the wave calls it
__device__ __forceinline__ void env_bwd_pixel(const ShadeArgs &A, const float *__restrict__ fv, float *__restrict__ gmaps, float *__restrict__ gfv,
                                              int want_bary, int persp, const MapDescCache &mdc, const int *s_md, HardTexAgg &tex_agg,
                                              HardFaceAgg &face_agg, bool valid, int fc, float u, float v, int jm, const float (&gc)[3], int xi, int yi) {
    const int j = jm & 0xfffff, map = jm >> 20;
    const bool tex = valid && (gc[0] != 0.f || gc[1] != 0.f || gc[2] != 0.f);
    Sample s;
    s.a00 = s.a01 = s.a10 = s.a11 = 0;
    s.w00 = s.w01 = s.w10 = s.w11 = 0.f;
    if (__ballot(tex) != 0ull) {
        int md[6];
        mdc.get(A, s_md, valid ? map : 0, md);
        footprint_desc(u, v, md[0], md[1], md[2], md[3], md[4], md[5], s);
        // colour -> texels: merge the footprint's texels that fall into the same stored cell
        float w00 = s.w00, w01 = s.w01, w10 = s.w10, w11 = s.w11;
        if (s.a01 == s.a00) { w00 += w01; w01 = 0.f; }
        if (s.a10 == s.a00) { w00 += w10; w10 = 0.f; }
        if (s.a11 == s.a00) { w00 += w11; w11 = 0.f; }
        else if (s.a11 == s.a01) { w01 += w11; w11 = 0.f; }
        else if (s.a11 == s.a10) { w10 += w11; w11 = 0.f; }
        const int ad[4] = {s.a00, s.a01, s.a10, s.a11};
        const float wt[4] = {w00, w01, w10, w11};
        // neighbouring pixels that hit the same texel (magnified maps: most of them) are merged in registers first (lane_merge, up to 16
        // lanes into one; full-resolution env maps 0.27 -> 0.24 ms, decimated ones unchanged)
        // (tap 0 and the lane's first other tap with weight as wave-wide passes; the rest -- footprints that cross a cell border in x AND y:
        // few lanes on magnified / decimated maps, every lane on full-resolution ones -- lane by lane or wave-wide accordingly.  See the uv
        // backward)
        const int f = wt[1] != 0.f ? 1 : (wt[2] != 0.f ? 2 : 3);
        const int a2[2] = {ad[0], f == 1 ? ad[1] : (f == 2 ? ad[2] : ad[3])};
        const float w2[2] = {wt[0], f == 1 ? wt[1] : (f == 2 ? wt[2] : wt[3])};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float val[3] = {gc[0] * w2[q], gc[1] * w2[q], gc[2] * w2[q]};
            const bool on = tex && w2[q] != 0.f;
            tex_agg.template add_wave_merged<4>(gmaps, (int)((unsigned)a2[q] / 3u), val, on);
        }
        const bool rest = tex && ((f == 1 && (wt[2] != 0.f || wt[3] != 0.f)) || (f == 2 && wt[3] != 0.f));
        const unsigned long long rm = __ballot(rest);
        if (rm != 0ull) {
            const bool wide = __popcll(rm) > 16;
#pragma unroll
            for (int q = 2; q < 4; ++q) {
                float val[3] = {gc[0] * wt[q], gc[1] * wt[q], gc[2] * wt[q]};
                const bool on = rest && q > f && wt[q] != 0.f;
                const int key = (int)((unsigned)ad[q] / 3u);
                if (wide) tex_agg.template add_wave_merged<4>(gmaps, key, val, on);
                else if (on) tex_agg.add(gmaps, key, val);
            }
        }
    }
    // colour -> uv -> barycentrics -> vertices, for the faces whose vertices are variables
    const bool geom = tex && want_bary != 0 && j >= A.geom_begin;
    float g9[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool has_g9 = false;
    if (__ballot(geom) != 0ull) {
        if (geom) {
            float gu, gv;
            sample_grad_uv(A.maps, s, gc, gu, gv);
            const float *uv = A.face_uvs + (long long)j * 6;
            const float go[3] = {gu * uv[0] + gv * uv[1], gu * uv[2] + gv * uv[3], gu * uv[4] + gv * uv[5]};
            int cd = -1;
            float w2 = 0.f, w3 = 0.f;
            if (A.c2o) {
                cd = A.code[fc]; w2 = A.cw[(long long)fc * 2]; w3 = A.cw[(long long)fc * 2 + 1];
            }
            float gb[3] = {0.f, 0.f, 0.f};
            convert_bary_bwd(cd, w2, w3, go, gb);
            if (gb[0] != 0.f || gb[1] != 0.f || gb[2] != 0.f) {
                has_g9 = true;
                f2 pndc;          // (same bits as pix_to_ndc: the shared-reciprocal division is exact for these operands, raster_math.h)
                pndc.x = pix_to_ndc_fast(A.W - 1 - xi, ndc_axis_given(A.W, A.ndc[0], A.ndc[1]));
                pndc.y = pix_to_ndc_fast(A.H - 1 - yi, ndc_axis_given(A.H, A.ndc[2], A.ndc[3]));
                const float *q = fv + (long long)fc * 9;
                const f2 a{q[0], q[1]}, b{q[3], q[4]}, c{q[6], q[7]};
                const float z0 = q[2], z1 = q[5], z2 = q[8];
                // (gradient-only arithmetic: v_rcp_f32 instead of ~15 IEEE divisions per pixel, as in the soft backward -- held at 1e-4)
                const f3 bary0 = bary_fwd<true>(pndc, a, b, c);
                const f3 bp = persp ? persp_fwd<true>(bary0, z0, z1, z2) : bary0;
                f3 gg3{gb[0], gb[1], gb[2]};
                gg3 = clip_bwd<true>(bp, gg3);
                float pz0 = 0.f, pz1 = 0.f, pz2 = 0.f;
                if (persp) gg3 = persp_bwd<true>(bary0, z0, z1, z2, gg3, pz0, pz1, pz2);
                f2 e0, e1, e2;
                bary_bwd<true>(pndc, a, b, c, gg3, e0, e1, e2);
                g9[0] = e0.x; g9[1] = e0.y; g9[2] = pz0;
                g9[3] = e1.x; g9[4] = e1.y; g9[5] = pz1;
                g9[6] = e2.x; g9[7] = e2.y; g9[8] = pz2;
            }
        }
        face_agg.add_wave(gfv, valid ? fc : 0, g9, has_g9);
    }
}


// The kernel body.  `lds`: HardTexAgg::BYTES + HardFaceAgg::BYTES of dynamic LDS; `s_md`: MD_CACHE_MAPS * 8 ints.  The grid is
// dbw_xcd_grid(HardRegion<P>::blocks(N, H, W)) workgroups of 256 threads, consecutive regions of one view on one XCD (xcd_remap).
// (pixel_of_block's strip remap, ShadeArgs::dbg & 32, does not apply: the region and its tiles are laid out here)
template <int P>
__device__ __forceinline__ void env_bwd_region(const ShadeArgs &A, long long total_blocks, const float *__restrict__ gimg,
                                               float *__restrict__ gmaps, const float *__restrict__ fv, float *__restrict__ gfv,
                                               int want_bary, int persp, void *lds, int *s_md) {
    typedef HardRegion<P> R;
    constexpr int NTH = 256;
    const long long logical = xcd_remap(blockIdx.x, total_blocks);
    if (logical < 0) return;
    HardTexAgg tex_agg;
    HardFaceAgg face_agg;
    tex_agg.bind(lds);
    face_agg.bind((char *)lds + HardTexAgg::BYTES);
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tiles_x = (A.W + 7) >> 3, tiles_y = (A.H + 7) >> 3;
    const int rx = (tiles_x + R::RX - 1) / R::RX, ry = (tiles_y + R::RY - 1) / R::RY;
    const int n = (int)(logical / (rx * ry)), t = (int)(logical % (rx * ry));
    const int tx0 = (t % rx) * R::RX + (wv & 1) * R::PX, ty0 = (t / rx) * R::RY + (wv >> 1) * R::PY;
    const long long view0 = (long long)n * tiles_y * tiles_x;
    const long long plane = (long long)A.H * A.W;
    const float gs = A.gscale ? *A.gscale : 1.f;
    // the fragments and image gradients of the wave's P tiles, 7 P loads in one batch.  The gradient image is 8x8-tile planar
    // (the training step) or (N, 4, H, W) planes, addressed at the pixel clamped into the image
    int rfc[P], xs[P], ys[P];
    float ru[P], rv[P], rjm[P], rg[P][3];
    bool inpx[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int tx = tx0 + p % R::PX, ty = ty0 + p / R::PX;
        const bool real = tx < tiles_x && ty < tiles_y;
        const long long tile = real ? view0 + (long long)ty * tiles_x + tx : view0;
        xs[p] = tx * 8 + (lane & 7);
        ys[p] = ty * 8 + (lane >> 3);
        inpx[p] = real && xs[p] < A.W && ys[p] < A.H;
        rfc[p] = ld_stream(A.p2f + (tile << 6) + lane);
        const float *b = A.bary + ((tile * 3) << 6) + lane;
        ru[p] = ld_stream(b); rv[p] = ld_stream(b + 64); rjm[p] = ld_stream(b + 128);
        const int xc = xs[p] < A.W ? xs[p] : A.W - 1, yc = ys[p] < A.H ? ys[p] : A.H - 1;
        const long long gb = A.img_tiled ? ((tile * 4) << 6) + lane : (long long)n * 4 * plane + (long long)yc * A.W + xc;
        const long long cs = A.img_tiled ? 64 : plane;
        rg[p][0] = ld_stream(gimg + gb); rg[p][1] = ld_stream(gimg + gb + cs); rg[p][2] = ld_stream(gimg + gb + 2 * cs);
    }
    // while they travel: the tables are cleared and the map descriptors copied to LDS
    tex_agg.clear(threadIdx.x, NTH);
    face_agg.clear(threadIdx.x, NTH);
    MapDescCache mdc;
    mdc.load(A, s_md, nullptr, threadIdx.x, NTH, true);
    __syncthreads();
    bool valid[P];
    int fc[P], jm[P];
    float gc[P][3];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        valid[p] = inpx[p] && rfc[p] >= 0;
        fc[p] = valid[p] ? rfc[p] : 0;
        jm[p] = valid[p] ? __float_as_int(rjm[p]) : 0;
        ru[p] = valid[p] ? ru[p] : 0.f;
        rv[p] = valid[p] ? rv[p] : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) gc[p][c] = valid[p] ? rg[p][c] * gs : 0.f;       // (blend weight of a hard fragment = 1)
    }
#pragma unroll 1
    for (int p = 0; p < P; ++p)
        env_bwd_pixel(A, fv, gmaps, gfv, want_bary, persp, mdc, s_md, tex_agg, face_agg, valid[p], fc[p], ru[p], rv[p], jm[p], gc[p], xs[p], ys[p]);
    __syncthreads();
    tex_agg.flush(gmaps, threadIdx.x, NTH);
    face_agg.flush(gfv, threadIdx.x, NTH);
}

}  // namespace dbw
