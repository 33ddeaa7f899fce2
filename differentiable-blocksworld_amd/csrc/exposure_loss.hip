// The reconstruction term under a per-view exposure (include/dbw_monitor.h: dbw_monitor_exposure_composite).
// theta (V,6) fp32 holds one row (g_r, g_g, g_b, b_r, b_g, b_b) per training view, ids (N) the batch's rows:
//   rec_c = exp(g_c) * comp_c + b_c,   comp = fg_rgb * alpha + (1 - alpha) * env_rgb,   value = scale * sum m (rec - img)^2.
// The arithmetic is exposure_math.h.  The streaming structure is masked_loss.hip's -- a lane owns four adjacent pixels of a row (16-byte
// loads of every plane) where W % 4 == 0 and the pointers allow it, one pixel otherwise -- with one difference: the grid's y is the view,
// so a workgroup never straddles two views.  theta and the id of the workgroup's view are read once per workgroup (thread 0..5 into LDS,
// the gains exponentiated there); an id outside [0, V) reads as theta = 0 and its gradient row is skipped.
//
// Forward: rec and one fp64 partial per workgroup (lane sums in fp64, then loss_reduce.h: block_sums), added in a fixed order by a second
// launch of one workgroup (partials_finish_kernel).  Backward: one image launch -- rec formed again from fg, env and theta,
// grad_fg and grad_env written through the composite, the six per-view sums reduced in the lane, the wave and the workgroup to six fp64
// partials -- and one finishing launch, a workgroup per view that adds the view's partials in a fixed order (thread t those of the
// workgroups t, t + 256, ... in index order, then wave and workgroup as above) and adds the result to the row ids[n] of grad_theta.
// No floating-point atomics: two calls on the same inputs give the same bytes.
#include "dbw_common.h"
#include "exposure_math.h"
#include "loss_reduce.h"
#include "../../include/dbw_monitor.h"

namespace {

using namespace dbw;

constexpr int THREADS = LOSS_THREADS;
constexpr int WAVES = LOSS_WAVES;
constexpr int VIEW_MAX_BLOCKS = 256;                // workgroups per view, grid-stride within the view beyond that
constexpr int MAX_VIEWS = 65535;                    // grid y

struct ExpArgs {
    const float *fg, *env, *img, *msk, *theta, *grad_rec, *upstream;
    const int32_t *ids;
    float *rec, *gfg, *genv;
    double *partial;                                // forward: [N][blocks]; backward: [N][blocks][6]
    double scale;
    long long plane, units;                         // H * W; lanes' items of ONE view: plane / PX
    int V;
};

int view_blocks(int H, int W, bool vec) {
    const long long units = (long long)H * W / (vec ? 4 : 1);
    const long long b = (units + THREADS - 1) / THREADS;
    return (int)(b < VIEW_MAX_BLOCKS ? b : VIEW_MAX_BLOCKS);
}

template <bool VEC, bool BWD>
__global__ void __launch_bounds__(THREADS) exposure_composite_kernel(ExpArgs A) {
    constexpr int PX = VEC ? 4 : 1;
    constexpr int NS = BWD ? 6 : 1;
    __shared__ double red[WAVES][NS];
    __shared__ float th[6];                         // the three gains, the three offsets of this workgroup's view
    const long long plane = A.plane;
    const long long n = blockIdx.y;
    if (threadIdx.x < 6) {
        const int id = A.ids[n];
        float t = 0.f;
        if (id >= 0 && id < A.V) t = A.theta[(long long)id * 6 + threadIdx.x];
        th[threadIdx.x] = threadIdx.x < 3 ? expf(t) : t;
    }
    __syncthreads();
    const float gain[3] = {th[0], th[1], th[2]}, bias[3] = {th[3], th[4], th[5]};
    float two_scale = 0.f;
    if constexpr (BWD) two_scale = (float)((2.0 * A.scale) * (double)A.upstream[0]);
    const bool has_extra = BWD && A.grad_rec != nullptr;
    const bool has_mask = A.msk != nullptr;
    double part[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) part[k] = 0.0;
    for (long long u = (long long)blockIdx.x * THREADS + threadIdx.x; u < A.units; u += (long long)gridDim.x * THREADS) {
        const long long p = u * PX;                                        // (VEC: W % 4 == 0, the four pixels lie in one row)
        float fc[3][PX], ec[3][PX], tc[3][PX], xc[3][PX], al[PX], mk[PX];
        load_layers_px<PX>(A.fg, A.env, A.img, A.grad_rec, A.msk, has_extra, has_mask, n, p, plane, fc, ec, tc, xc, al, mk);
        float rc[3][PX], gf[4][PX], ge[4][PX];
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            const float f3[3] = {fc[0][k], fc[1][k], fc[2][k]}, e3[3] = {ec[0][k], ec[1][k], ec[2][k]};
            const float t3[3] = {tc[0][k], tc[1][k], tc[2][k]};
            if constexpr (BWD) {
                const float x3[3] = {xc[0][k], xc[1][k], xc[2][k]};
                float gf3[3], ge3[3], galpha, s6[6];
                exposure_backward_pixel(f3, al[k], e3, t3, mk[k], gain, bias, two_scale, x3, has_extra, gf3, ge3, galpha, s6);
#pragma unroll
                for (int c = 0; c < 3; ++c) { gf[c][k] = gf3[c]; ge[c][k] = ge3[c]; }
                gf[3][k] = galpha; ge[3][k] = 0.f;
#pragma unroll
                for (int j = 0; j < 6; ++j) part[j] += (double)s6[j];
            } else {
                float r3[3];
                part[0] += (double)exposure_forward_pixel(f3, al[k], e3, t3, mk[k], gain, bias, r3);
#pragma unroll
                for (int c = 0; c < 3; ++c) rc[c][k] = r3[c];
            }
        }
        if constexpr (BWD) {
            store_layer_grads_px<PX>(A.gfg, A.genv, n, p, plane, gf, ge);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) store_px<PX>(A.rec + n * 3 * plane + c * plane + p, rc[c]);
        }
    }
    const double total = block_sums<NS>(part, red);
    if (threadIdx.x < NS) A.partial[(n * gridDim.x + blockIdx.x) * NS + threadIdx.x] = total;
}

// a workgroup per view n of the batch: thread t takes the partials of the view's workgroups t, t + 256, ... in index order, the workgroup
// adds the threads' sums as the image launch does (block_sums), and threads 0..5 add the six results to grad_theta[ids[n]]
__global__ void __launch_bounds__(THREADS) exposure_theta_kernel(const double *__restrict__ partial, const int32_t *__restrict__ ids, int blocks,
                                                                 int V, float *__restrict__ grad_theta) {
    __shared__ double red[WAVES][6];
    const long long n = blockIdx.x;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < blocks; b += THREADS) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] += partial[(n * blocks + b) * 6 + k];
    }
    const double t = block_sums<6>(s, red);
    const int id = ids[n];
    if (threadIdx.x < 6 && id >= 0 && id < V) grad_theta[(long long)id * 6 + threadIdx.x] += (float)t;
}

bool size_ok(int N, int H, int W) { return N >= 0 && N <= MAX_VIEWS && H > 0 && W > 0 && (long long)H * W < (1LL << 31); }

}  // namespace

extern "C" size_t dbw_monitor_exposure_composite_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || !size_ok(N, H, W)) return 0;
    return (size_t)N * view_blocks(H, W, false) * 6 * sizeof(double);       // (the element form has the most workgroups, the backward six sums)
}

extern "C" int dbw_monitor_exposure_composite(const float *fg, const float *env, const float *imgs, const float *masks, const float *theta,
                                              const int32_t *ids, int N, int H, int W, int V, double scale, void *workspace, float *rec,
                                              double *value, const float *upstream, const float *grad_rec, float *grad_fg, float *grad_env,
                                              float *grad_theta, dbw_stream_t stream) {
    DBW_REQUIRE(fg && env && imgs && theta && ids, "null pointer");
    DBW_REQUIRE(size_ok(N, H, W), "bad size");
    DBW_REQUIRE(V > 0, "V below 1");
    DBW_REQUIRE((grad_fg && grad_env && grad_theta) || (!grad_fg && !grad_env && !grad_theta), "grad_fg / grad_env / grad_theta: all or none");
    DBW_REQUIRE(scale - scale == 0.0, "scale is not finite");
    const bool bwd = grad_fg != nullptr;
    if (bwd) DBW_REQUIRE(upstream && !rec && !value, "backward: the upstream scalar, and neither rec nor value");
    else DBW_REQUIRE(rec && value && ((uintptr_t)value & 7) == 0 && !grad_rec && !upstream, "forward: rec and an 8-byte aligned value, no upstream, no grad_rec");
    if (N == 0) return DBW_OK;
    DBW_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "workspace: null or not 8-byte aligned");
    DBW_REQUIRE(aligned4(fg) && aligned4(env) && aligned4(imgs) && aligned4(masks) && aligned4(theta) && aligned4(ids) && aligned4(rec)
                    && aligned4(upstream) && aligned4(grad_rec) && aligned4(grad_fg) && aligned4(grad_env) && aligned4(grad_theta),
                "misaligned pointer");
    const bool vec = W % 4 == 0 && aligned16(fg) && aligned16(env) && aligned16(imgs) && aligned16(masks) && aligned16(rec) && aligned16(grad_rec)
                     && aligned16(grad_fg) && aligned16(grad_env);
    ExpArgs A;
    A.fg = fg; A.env = env; A.img = imgs; A.msk = masks; A.theta = theta; A.grad_rec = grad_rec; A.upstream = upstream; A.ids = ids;
    A.rec = rec; A.gfg = grad_fg; A.genv = grad_env; A.partial = (double *)workspace; A.scale = scale;
    A.plane = (long long)H * W; A.units = A.plane / (vec ? 4 : 1); A.V = V;
    const int blocks = view_blocks(H, W, vec);
    const dim3 g((unsigned)blocks, (unsigned)N), b(THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (bwd) {
        if (vec) hipLaunchKernelGGL((exposure_composite_kernel<true, true>), g, b, 0, s, A);
        else hipLaunchKernelGGL((exposure_composite_kernel<false, true>), g, b, 0, s, A);
        const int rc = dbw_check_launch("exposure_composite_kernel");
        if (rc != DBW_OK) return rc;
        hipLaunchKernelGGL(exposure_theta_kernel, dim3((unsigned)N), b, 0, s, (const double *)workspace, ids, blocks, V, grad_theta);
        return dbw_check_launch("exposure_theta_kernel");
    }
    if (vec) hipLaunchKernelGGL((exposure_composite_kernel<true, false>), g, b, 0, s, A);
    else hipLaunchKernelGGL((exposure_composite_kernel<false, false>), g, b, 0, s, A);
    const int rc = dbw_check_launch("exposure_composite_kernel");
    if (rc != DBW_OK) return rc;
    return partials_finish((const double *)workspace, (long long)N * blocks, scale, 1.0, value, s);
}
