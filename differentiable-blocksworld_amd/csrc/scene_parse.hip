// Scene parsing maps (include/dbw_viz.h: dbw_viz_parse_fwd): per pixel of N views of a packed scene, the label of the nearest face, its
// depth, and the 64-bit word of ALL labels that cover the pixel -- occluded or not -- plus per view and label the amodal and the visible
// area.  Hard rasterisation (sigma = 0, blur_radius = 0), no culling, forward only.
//
// scene_parse_kernel is the hard single-layer pass: the same per-face set-up and bins (dbw_prepare_raster), the same raster_tile on the
// 16x16 tiles of the K = 1 instantiations, the same eval_pair -- with ParsePixel (parse_math.h) in the place of the top-K list: one nearest
// fragment in registers and the coverage word.  It writes 13 B per pixel (1 + 4 + 8) and nothing else but the counts, which are integers
// from the wave to global memory: two calls are bit-equal.
#include "raster_common.h"
#include "parse_math.h"
#include "../../include/dbw_viz.h"

using namespace dbw;

// implemented in raster.hip
int dbw_prepare_raster(const float *face_verts, const int *first_idx, const int *num_faces, const int *neighbor, int N, long long F_total,
                       long long max_faces_per_view, int H, int W, float margin, int cull, void *workspace, size_t workspace_bytes,
                       dbw::CoarseBins &cb, hipStream_t s, bool launch, bool want_cells);
const dbw::FaceRec *dbw_workspace_recs(const void *workspace, long long F_total);

static_assert(PARSE_MAX_LABELS == DBW_VIZ_MAX_LABELS && PARSE_NO_LABEL == DBW_VIZ_NO_LABEL, "parse_math.h and dbw_viz.h disagree");

namespace {

constexpr int PT = 16, PNT = PT * PT;          // the tile of the K = 1 instantiations

// ---- label of every clipped face: the c2o indirection is resolved once per pass, not once per (pixel, face) ------------------------------
__global__ void parse_label_kernel(const int32_t *__restrict__ face_label, const int32_t *__restrict__ c2o, long long F_total, int F,
                                   int32_t *__restrict__ lab) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F_total) return;
    lab[f] = parse_clipped_label(face_label, c2o, f, F);
}

__global__ __launch_bounds__(PNT, DBW_RASTER_WAVES(1)) void scene_parse_kernel(const FaceRec *__restrict__ recs, const float4 *__restrict__ bbox,
                                                                                const int *__restrict__ first_idx, const int *__restrict__ num_faces,
                                                                                int H, int W, int persp, long long total_blocks, CoarseBins cb,
                                                                                const int32_t *__restrict__ lab, uint8_t *__restrict__ label,
                                                                                float *__restrict__ depth, unsigned long long *__restrict__ cover,
                                                                                int *__restrict__ counts) {
    __shared__ int s_cnt[PARSE_MAX_LABELS * 2];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < PARSE_MAX_LABELS * 2) s_cnt[tid] = 0;
    int n, xi, yi;
    ParsePixel q;
    q.lab = lab;
    pay4 *home;
    // (clipped barycentrics and the full signed distance, as the K = 1 fragment pass evaluates them: the sibling rule compares distances)
    if (!raster_tile<1, PT, PT, 1>(recs, bbox, first_idx, num_faces, H, W, 1, 0.f, persp, 1, total_blocks, cb, 0, n, xi, yi, q, home)) return;
    __syncthreads();                              // s_cnt is zero for every wave (raster_tile has paths without a barrier)
    const bool in_img = xi < W && yi < H;
    int l = PARSE_NO_LABEL, face;
    float d;
    uint64_t cov = 0ull;
    if (in_img) {
        q.result(l, d, face);
        cov = q.cover;
        const long long o = ((long long)n * H + yi) * W + xi;
        label[o] = (uint8_t)l;
        depth[o] = d;
        cover[o] = cov;
    }
    // counts: one round per label present in the wave (a handful), not per label possible
    uint64_t rem = cov;
    while (true) {
        const unsigned long long m = __ballot(rem != 0ull);
        if (m == 0ull) break;
        const int src = __ffsll((long long)m) - 1;
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)rem, src), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(rem >> 32), src);
        uint64_t word = ((uint64_t)hi << 32) | lo;
        const int b = parse_pop_label(word);
        const int amodal = __popcll(__ballot(parse_covers(cov, b))), visible = __popcll(__ballot(l == b));
        if (lane == 0) {
            atomicAdd(&s_cnt[b * 2], amodal);
            if (visible) atomicAdd(&s_cnt[b * 2 + 1], visible);
        }
        rem &= ~parse_bit(b);
    }
    __syncthreads();
    if (tid < PARSE_MAX_LABELS * 2) {
        const int c = s_cnt[tid];
        if (c) atomicAdd(&counts[(long long)n * (PARSE_MAX_LABELS * 2) + tid], c);
    }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

bool parse_sizes_ok(int64_t F_total, int N, int F, int H, int W) {
    return F_total >= 0 && F_total < (1LL << TOPK_ID_BITS) && N > 0 && F > 0 && H > 0 && W > 0 && H < (1 << 24) && W < (1 << 24) &&
           (long long)N * PARSE_MAX_LABELS * 2 < (1LL << 31);
}

}  // namespace

// workspace = [the rasteriser's binned workspace][label of every clipped face: F_total x 4 B]
extern "C" size_t dbw_viz_parse_workspace_bytes(int64_t F_total, int N, int F, int H, int W) {
    if (!parse_sizes_ok(F_total, N, F, H, W)) return 0;
    return dbw_rasterize_workspace_bytes_binned(F_total, N, H, W) + align256((size_t)(F_total > 0 ? F_total : 1) * sizeof(int32_t));
}

extern "C" int dbw_viz_parse_fwd(const float *face_verts_c, const int32_t *first_idx, const int32_t *num_faces, const int32_t *neighbor,
                                 const int32_t *c2o, int Fc_stride, int N, int64_t F_total, int H, int W, int F, int perspective_correct,
                                 const int32_t *face_label, const int32_t *face_label_host, uint8_t *label, float *depth, int64_t *cover,
                                 int32_t *counts, void *workspace, size_t workspace_bytes, dbw_stream_t stream) {
    DBW_REQUIRE(face_verts_c && first_idx && num_faces && face_label && label && depth && cover && counts && workspace, "null pointer");
    DBW_REQUIRE(parse_sizes_ok(F_total, N, F, H, W), "bad size");
    DBW_REQUIRE(!c2o || Fc_stride > 0, "bad Fc_stride");
    DBW_REQUIRE(workspace_bytes >= dbw_viz_parse_workspace_bytes(F_total, N, F, H, W), "workspace too small");
    const long long total = (long long)N * ((W + PT - 1) / PT) * ((H + PT - 1) / PT);
    DBW_REQUIRE(total < (1LL << 31) - 8, "more than 2^31 tiles in one pass");
    if (face_label_host) {
        const long long bad = parse_first_bad_label(face_label_host, F);
        if (bad >= 0) {
            dbw_set_error("dbw_viz_parse_fwd: face_label[%lld] = %d is outside [0, %d)", bad, (int)face_label_host[bad], DBW_VIZ_MAX_LABELS);
            return DBW_ERR_INVALID;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t raster_bytes = dbw_rasterize_workspace_bytes_binned(F_total, N, H, W);
    int32_t *lab = (int32_t *)((char *)workspace + raster_bytes);
    if (hipMemsetAsync(counts, 0, (size_t)N * PARSE_MAX_LABELS * 2 * sizeof(int32_t), s) != hipSuccess) {
        dbw_set_error("dbw_viz_parse_fwd: hipMemsetAsync(counts) failed");
        return DBW_ERR_INVALID;
    }
    CoarseBins cb;
    int rc = dbw_prepare_raster(face_verts_c, first_idx, num_faces, neighbor, N, F_total, c2o ? (long long)Fc_stride : F_total, H, W, 0.f, 0, workspace,
                                raster_bytes, cb, s, /*launch=*/true, /*want_cells: the 8x8-tile kernels*/ false);
    if (rc) return rc;
    if (F_total > 0) {
        hipLaunchKernelGGL(parse_label_kernel, dim3((unsigned)((F_total + 255) / 256)), dim3(256), 0, s, face_label, c2o, (long long)F_total, F, lab);
        rc = dbw_check_launch("parse_label_kernel");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(scene_parse_kernel, dim3(dbw_xcd_grid(total)), dim3(PNT), 0, s, dbw_workspace_recs(workspace, F_total), (const float4 *)workspace, first_idx,
                       num_faces, H, W, perspective_correct, total, cb, (const int32_t *)lab, label, depth, (unsigned long long *)cover, counts);
    return dbw_check_launch("scene_parse_kernel");
}
