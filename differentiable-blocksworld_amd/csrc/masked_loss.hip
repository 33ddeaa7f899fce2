// The reconstruction term under a validity mask (include/dbw_monitor.h: dbw_monitor_masked_composite; the SSIM term under the mask is
// ssim_term.hip's).  masks (N,1,H,W) fp32 weights in [0, 1], count = 3 * sum(masks) a host number: no kernel reads a device scalar for
// it, and count == 0 gives 0 and a zero gradient without a division.
//
// composite + masked MSE.  rec = fg_rgb * alpha + (1 - alpha) * env_rgb as dbw_composite_mse forms it, and
//   value = scale * sum m (rec - img)^2,   scale = w_rgb / count.
// A streaming pass: a lane owns four adjacent pixels of a row (16-byte loads of every plane) where W % 4 == 0 and the pointers allow it,
// one pixel otherwise.  The forward writes rec and one fp64 partial per workgroup (lane sums in fp64 in the lane's own order, then
// loss_reduce.h: block_sums); a second launch of one workgroup adds the partials in a fixed order (partials_finish_kernel).  No atomics:
// two calls give the same bits.  The backward is one launch: per pixel d/d rec = 2 scale g m (rec - img) + grad_rec, g the upstream
// scalar of the term read from device memory, grad_rec the perceptual term's gradient (optional), taken through the composite into
// grad_fg and grad_env.  The arithmetic is loss_math.h: masked_composite_pixel.
#include "dbw_common.h"
#include "loss_math.h"
#include "loss_reduce.h"
#include "../../include/dbw_monitor.h"

namespace {

using namespace dbw;

constexpr int THREADS = LOSS_THREADS;
constexpr int COMP_MAX_BLOCKS = 1024;               // 256 CUs x 4 resident workgroups, grid-stride beyond that

struct CompArgs {
    const float *fg, *env, *img, *msk, *grad_rec, *upstream;
    float *rec, *gfg, *genv;
    double *partial;
    double scale;
    long long plane, units;                         // H * W; lanes' items: N * plane / PX
};

long long comp_blocks(int N, int H, int W, bool vec) {
    const long long units = (long long)N * H * W / (vec ? 4 : 1);
    const long long b = (units + THREADS - 1) / THREADS;
    return b < COMP_MAX_BLOCKS ? b : COMP_MAX_BLOCKS;
}

template <bool VEC, bool BWD>
__global__ void __launch_bounds__(THREADS) masked_composite_kernel(CompArgs A) {
    constexpr int PX = VEC ? 4 : 1;
    __shared__ double red[LOSS_WAVES][1];
    const long long plane = A.plane;
    float two_scale = 0.f;
    if constexpr (BWD) two_scale = (float)((2.0 * A.scale) * (double)A.upstream[0]);
    const bool has_extra = BWD && A.grad_rec != nullptr;
    double part = 0.0;
    for (long long u = (long long)blockIdx.x * THREADS + threadIdx.x; u < A.units; u += (long long)gridDim.x * THREADS) {
        const long long i = u * PX, n = i / plane, p = i % plane;          // (VEC: plane % 4 == 0, the four pixels lie in one image)
        float fc[3][PX], ec[3][PX], tc[3][PX], xc[3][PX], al[PX], mk[PX];
        load_layers_px<PX>(A.fg, A.env, A.img, A.grad_rec, A.msk, has_extra, true, n, p, plane, fc, ec, tc, xc, al, mk);
        float rc[3][PX], gf[4][PX], ge[4][PX];
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            const float f3[3] = {fc[0][k], fc[1][k], fc[2][k]}, e3[3] = {ec[0][k], ec[1][k], ec[2][k]};
            const float t3[3] = {tc[0][k], tc[1][k], tc[2][k]}, x3[3] = {xc[0][k], xc[1][k], xc[2][k]};
            float r3[3], gf3[3], ge3[3], gmask;
            part += (double)masked_composite_pixel(f3, al[k], e3, t3, mk[k], two_scale, r3, gf3, ge3, gmask, x3, has_extra);
#pragma unroll
            for (int c = 0; c < 3; ++c) { rc[c][k] = r3[c]; gf[c][k] = gf3[c]; ge[c][k] = ge3[c]; }
            gf[3][k] = gmask; ge[3][k] = 0.f;
        }
        if constexpr (BWD) {
            store_layer_grads_px<PX>(A.gfg, A.genv, n, p, plane, gf, ge);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) store_px<PX>(A.rec + n * 3 * plane + c * plane + p, rc[c]);
        }
    }
    if constexpr (!BWD) {
        const double t = block_sum(part, red);
        if (threadIdx.x == 0) A.partial[blockIdx.x] = t;
    }
}

}  // namespace

extern "C" size_t dbw_monitor_masked_composite_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || (long long)H * W >= (1LL << 31)) return 0;
    return (size_t)comp_blocks(N, H, W, false) * sizeof(double);          // (the element form has the most workgroups)
}

extern "C" int dbw_monitor_masked_composite(const float *fg, const float *env, const float *imgs, const float *masks, int N, int H, int W,
                                            double scale, void *workspace, float *rec, double *value, const float *upstream,
                                            const float *grad_rec, float *grad_fg, float *grad_env, dbw_stream_t stream) {
    DBW_REQUIRE(fg && env && imgs && masks, "null pointer");
    DBW_REQUIRE(N >= 0 && H > 0 && W > 0 && (long long)H * W < (1LL << 31), "bad size");
    DBW_REQUIRE((grad_fg && grad_env) || (!grad_fg && !grad_env), "grad_fg / grad_env: both or none");
    DBW_REQUIRE(scale - scale == 0.0, "scale is not finite");
    const bool bwd = grad_fg != nullptr;
    if (bwd) DBW_REQUIRE(upstream && !rec && !value, "backward: the upstream scalar, and neither rec nor value");
    else DBW_REQUIRE(rec && value && ((uintptr_t)value & 7) == 0 && !grad_rec, "forward: rec and an 8-byte aligned value, no grad_rec");
    if (N == 0) return DBW_OK;
    if (!bwd) DBW_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "workspace: null or not 8-byte aligned");
    DBW_REQUIRE(aligned4(fg) && aligned4(env) && aligned4(imgs) && aligned4(masks) && aligned4(rec) && aligned4(upstream) && aligned4(grad_rec)
                    && aligned4(grad_fg) && aligned4(grad_env), "misaligned pointer");
    const bool vec = W % 4 == 0 && aligned16(fg) && aligned16(env) && aligned16(imgs) && aligned16(masks) && aligned16(rec) && aligned16(grad_rec)
                     && aligned16(grad_fg) && aligned16(grad_env);
    CompArgs A;
    A.fg = fg; A.env = env; A.img = imgs; A.msk = masks; A.grad_rec = grad_rec; A.upstream = upstream;
    A.rec = rec; A.gfg = grad_fg; A.genv = grad_env; A.partial = (double *)workspace; A.scale = scale;
    A.plane = (long long)H * W; A.units = (long long)N * A.plane / (vec ? 4 : 1);
    const long long blocks = comp_blocks(N, H, W, vec);
    const dim3 g((unsigned)blocks), b(THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (bwd) {
        if (vec) hipLaunchKernelGGL((masked_composite_kernel<true, true>), g, b, 0, s, A);
        else hipLaunchKernelGGL((masked_composite_kernel<false, true>), g, b, 0, s, A);
        return dbw_check_launch("masked_composite_kernel");
    }
    if (vec) hipLaunchKernelGGL((masked_composite_kernel<true, false>), g, b, 0, s, A);
    else hipLaunchKernelGGL((masked_composite_kernel<false, false>), g, b, 0, s, A);
    const int rc = dbw_check_launch("masked_composite_kernel");
    if (rc != DBW_OK) return rc;
    return partials_finish((const double *)workspace, blocks, scale, 1.0, value, s);
}

