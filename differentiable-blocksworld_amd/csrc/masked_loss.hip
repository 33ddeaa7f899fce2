// The two image terms of the loss under a validity mask (include/dbw_monitor.h: dbw_monitor_masked_composite,
// dbw_monitor_masked_ssim_term).  masks (N,1,H,W) fp32 weights in [0, 1], count = 3 * sum(masks) a host number: no kernel reads a
// device scalar for it, and count == 0 gives 0 and a zero gradient without a division.
//
// 1. composite + masked MSE.  rec = fg_rgb * alpha + (1 - alpha) * env_rgb as dbw_composite_mse forms it, and
//      value = scale * sum m (rec - img)^2,   scale = w_rgb / count.
//    A streaming pass: a lane owns four adjacent pixels of a row (16-byte loads of every plane) where W % 4 == 0 and the pointers allow it,
//    one pixel otherwise.  The forward writes rec and one fp64 partial per workgroup (lane sums in fp64 in the lane's own order, the wave
//    through fixed-order butterflies, the waves in wave order); a second launch of one workgroup adds the partials in a fixed order.  No
//    atomics: two calls give the same bits.  The backward is one launch: per pixel d/d rec = 2 scale g m (rec - img) + grad_rec, g the
//    upstream scalar of the term read from device memory, grad_rec the perceptual term's gradient (optional), taken through the composite
//    into grad_fg and grad_env.  The arithmetic is loss_math.h: masked_composite_pixel.
//
// 2. the SSIM term under the mask: sum over n, c, p of m_p (1 - SSIM_p(m a, m b)) / count and its gradient in b, in the structure of
//    ssim_term.hip (a workgroup of 256 threads per 16 x 32 tile of one plane, the statistics and the derivative maps in LDS, the same
//    score_math.h functions in the same order).  The mask enters three times: the inputs are multiplied by m as they are loaded into the
//    tile; S's derivative maps A, B, C and 1 - S of the window centred at p are multiplied by m_p; the gradient at q is multiplied by m_q.
//    The mask is NOT kept in LDS: it is a third of an image plane, shared by the three channels, and each of the three uses reads it from
//    memory at the index the lane already has (the tile load beside a and b, 16 bytes at a time where they are; the 26 x 42 window
//    centres; the 16 x 32 outputs).  LDS stays at the 46.4 KB of the plain kernel, three workgroups per CU.  With a mask of ones every
//    product is exact: the gradient is dbw_monitor_ssim_term's bit for bit.
#include "dbw_common.h"
#include "loss_math.h"
#include "score_math.h"
#include "../../include/dbw_monitor.h"

namespace {

using namespace dbw;

constexpr int THREADS = 256;

// the sum over the wave (fixed-order butterflies), the waves in wave order; the result in thread 0
__device__ __forceinline__ double block_sum(double s, double *red) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, DBW_WAVE);
    if ((tid & (DBW_WAVE - 1)) == 0) red[tid / DBW_WAVE] = s;
    __syncthreads();
    double t = 0.0;
    if (tid == 0) {
        t = red[0];
        for (int w = 1; w < THREADS / DBW_WAVE; ++w) t += red[w];
    }
    return t;
}

// value[0] = (the partials added in a fixed order) * mul / div, 0 where div is not positive: thread t adds t, t + 256, ... in index order
__global__ void __launch_bounds__(THREADS) masked_finish_kernel(const double *__restrict__ partial, long long count, double mul, double div,
                                                                double *__restrict__ value) {
    __shared__ double red[THREADS / DBW_WAVE];
    double s = 0.0;
    for (long long i = threadIdx.x; i < count; i += THREADS) s += partial[i];
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) value[0] = div > 0.0 ? (t * mul) / div : 0.0;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
bool aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }

// ---- 1. composite + masked MSE ------------------------------------------------------------------------------------------------------------
constexpr int COMP_MAX_BLOCKS = 1024;               // 256 CUs x 4 resident workgroups, grid-stride beyond that

struct CompArgs {
    const float *fg, *env, *img, *msk, *grad_rec, *upstream;
    float *rec, *gfg, *genv;
    double *partial;
    double scale;
    long long plane, units;                         // H * W; lanes' items: N * plane / PX
};

template <int PX>
__device__ __forceinline__ void load_px(const float *p, float v[PX]) {
    if constexpr (PX == 4) {
        const float4 t = *(const float4 *)p;
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[0];
    }
}

template <int PX>
__device__ __forceinline__ void store_px(float *p, const float v[PX]) {
    if constexpr (PX == 4) *(float4 *)p = make_float4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}

long long comp_blocks(int N, int H, int W, bool vec) {
    const long long units = (long long)N * H * W / (vec ? 4 : 1);
    const long long b = (units + THREADS - 1) / THREADS;
    return b < COMP_MAX_BLOCKS ? b : COMP_MAX_BLOCKS;
}

template <bool VEC, bool BWD>
__global__ void __launch_bounds__(THREADS) masked_composite_kernel(CompArgs A) {
    constexpr int PX = VEC ? 4 : 1;
    __shared__ double red[THREADS / DBW_WAVE];
    const long long plane = A.plane;
    float two_scale = 0.f;
    if constexpr (BWD) two_scale = (float)((2.0 * A.scale) * (double)A.upstream[0]);
    const bool has_extra = BWD && A.grad_rec != nullptr;
    double part = 0.0;
    for (long long u = (long long)blockIdx.x * THREADS + threadIdx.x; u < A.units; u += (long long)gridDim.x * THREADS) {
        const long long i = u * PX, n = i / plane, p = i % plane;          // (VEC: plane % 4 == 0, the four pixels lie in one image)
        const float *f = A.fg + n * 4 * plane + p, *e = A.env + n * 4 * plane + p, *t = A.img + n * 3 * plane + p;
        float fc[3][PX], ec[3][PX], tc[3][PX], xc[3][PX], al[PX], mk[PX];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            load_px<PX>(f + c * plane, fc[c]);
            load_px<PX>(e + c * plane, ec[c]);
            load_px<PX>(t + c * plane, tc[c]);
#pragma unroll
            for (int k = 0; k < PX; ++k) xc[c][k] = 0.f;
            if (has_extra) load_px<PX>(A.grad_rec + n * 3 * plane + c * plane + p, xc[c]);
        }
        load_px<PX>(f + 3 * plane, al);
        load_px<PX>(A.msk + n * plane + p, mk);
        float rc[3][PX], gf[4][PX], ge[4][PX];
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            const float f3[3] = {fc[0][k], fc[1][k], fc[2][k]}, e3[3] = {ec[0][k], ec[1][k], ec[2][k]}, t3[3] = {tc[0][k], tc[1][k], tc[2][k]};
            const float x3[3] = {xc[0][k], xc[1][k], xc[2][k]};
            float r3[3], gf3[3], ge3[3], gmask;
            part += (double)masked_composite_pixel(f3, al[k], e3, t3, mk[k], two_scale, r3, gf3, ge3, gmask, x3, has_extra);
#pragma unroll
            for (int c = 0; c < 3; ++c) { rc[c][k] = r3[c]; gf[c][k] = gf3[c]; ge[c][k] = ge3[c]; }
            gf[3][k] = gmask; ge[3][k] = 0.f;
        }
        if constexpr (BWD) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                store_px<PX>(A.gfg + n * 4 * plane + c * plane + p, gf[c]);
                store_px<PX>(A.genv + n * 4 * plane + c * plane + p, ge[c]);
            }
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

// ---- 2. the SSIM term under the mask: the tile geometry of ssim_term.hip ------------------------------------------------------------------
constexpr int TW = 32, TH = 16;                     // gradient outputs per workgroup
constexpr int RAD = SSIM_TAPS / 2;                  // 5
constexpr int DW = TW + SSIM_HALO, DH = TH + SSIM_HALO;       // 42 x 26 windows: tile + 5
constexpr int IN_H = TH + 2 * SSIM_HALO;            // 36 input rows
constexpr int IN_W = 56;                            // input columns kept: 12 (10 of halo, rounded to 4) + 32 + 10, rounded to 4
constexpr int IN_X0 = 12, SH = IN_X0 - SSIM_HALO;   // tile column 0 in the input tile; first column the row pass reads
constexpr int PER_THREAD = (DH * DW + THREADS - 1) / THREADS;           // 5 windows per thread
static_assert(3 * DH * DW + 3 * DH * TW <= 5 * IN_H * DW, "the derivative maps and their row pass share the space of rs");
static_assert(SH >= 0 && DW - 1 + SH + SSIM_HALO < IN_W && IN_W % 4 == 0, "input tile too narrow");

struct TermArgs {
    const float *a, *b, *msk;
    float *grad;
    double *partial;
    SsimWindow win;
    double scale;                                   // -1 / count (0 where count is 0)
    int H, W, tiles_x, tiles_y;
};

template <bool VEC, bool GRAD>
__global__ void __launch_bounds__(THREADS) masked_ssim_term_kernel(TermArgs A) {
    __shared__ __align__(16) float sa[IN_H * IN_W];
    __shared__ __align__(16) float sb[IN_H * IN_W];
    __shared__ float rs[5 * IN_H * DW];
    __shared__ double red[THREADS / DBW_WAVE];
    float *const dm = rs;                           // [3][DH][DW], once rs has been read
    float *const br = rs + 3 * DH * DW;             // [3][DH][TW]
    const int tid = threadIdx.x;
    const int tx = (int)(blockIdx.x % A.tiles_x), ty = (int)((blockIdx.x / A.tiles_x) % A.tiles_y);
    const long long plane = blockIdx.x / ((unsigned)A.tiles_x * A.tiles_y);          // n * 3 + channel
    const int x0 = tx * TW, y0 = ty * TH;
    const int xs = x0 - IN_X0, ys = y0 - SSIM_HALO;
    const float *pa = A.a + plane * A.H * A.W, *pb = A.b + plane * A.H * A.W, *pm = A.msk + (plane / 3) * A.H * A.W;

    if constexpr (VEC) {
        for (int i = tid; i < IN_H * (IN_W / 4); i += THREADS) {
            const int r = i / (IN_W / 4), q = i % (IN_W / 4);
            const int y = ys + r, x = xs + 4 * q;
            float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
            if (y >= 0 && y < A.H && x >= 0 && x < A.W) {              // (W % 4 == 0 and x % 4 == 0: the four are inside together)
                va = *(const float4 *)(pa + (long long)y * A.W + x);
                vb = *(const float4 *)(pb + (long long)y * A.W + x);
                const float4 vm = *(const float4 *)(pm + (long long)y * A.W + x);
                va.x *= vm.x; va.y *= vm.y; va.z *= vm.z; va.w *= vm.w;
                vb.x *= vm.x; vb.y *= vm.y; vb.z *= vm.z; vb.w *= vm.w;
            }
            *(float4 *)(sa + r * IN_W + 4 * q) = va;
            *(float4 *)(sb + r * IN_W + 4 * q) = vb;
        }
    } else {
        for (int i = tid; i < IN_H * IN_W; i += THREADS) {
            const int r = i / IN_W, c = i % IN_W;
            const int y = ys + r, x = xs + c;
            float va = 0.f, vb = 0.f;
            if (y >= 0 && y < A.H && x >= 0 && x < A.W) {
                const float vm = pm[(long long)y * A.W + x];
                va = pa[(long long)y * A.W + x] * vm;
                vb = pb[(long long)y * A.W + x] * vm;
            }
            sa[i] = va;
            sb[i] = vb;
        }
    }
    __syncthreads();

    // the five statistics along the rows.  Without a gradient only the own windows are formed: their rows RAD .. RAD + TH + 10, columns
    // RAD .. RAD + TW
    for (int i = tid; i < IN_H * DW; i += THREADS) {
        const int r = i / DW, c = i % DW;
        if (!GRAD && (r < RAD || r >= IN_H - RAD || c < RAD || c >= RAD + TW)) continue;
        float t[5][SSIM_TAPS];
#pragma unroll
        for (int k = 0; k < SSIM_TAPS; ++k) {
            float s[5];
            ssim_stats(sa[r * IN_W + c + SH + k], sb[r * IN_W + c + SH + k], s);
#pragma unroll
            for (int j = 0; j < 5; ++j) t[j][k] = s[j];
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) rs[(j * IN_H + r) * DW + c] = ssim_filter(A.win.w, t[j]);
    }
    __syncthreads();

    // along the columns, then the window: S and the derivative maps times the window's own weight m_p, kept in registers until every
    // thread has read rs
    float dA[PER_THREAD], dB[PER_THREAD], dC[PER_THREAD];
    double ss = 0.0;
#pragma unroll
    for (int it = 0; it < PER_THREAD; ++it) {
        const int i = tid + it * THREADS;
        dA[it] = dB[it] = dC[it] = 0.f;
        if (i >= DH * DW) continue;
        const int dy = i / DW, dx = i % DW;
        const int y = y0 - RAD + dy, x = x0 - RAD + dx;
        const bool own = dy >= RAD && dy < RAD + TH && dx >= RAD && dx < RAD + TW;
        if (y < 0 || y >= A.H || x < 0 || x >= A.W || (!GRAD && !own)) continue;
        const float mp = pm[(long long)y * A.W + x];
        float m[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            float t[SSIM_TAPS];
#pragma unroll
            for (int k = 0; k < SSIM_TAPS; ++k) t[k] = rs[(j * IN_H + dy + k) * DW + dx];
            m[j] = ssim_filter(A.win.w, t);
        }
        const SsimDeriv d = ssim_deriv(m);
        dA[it] = d.A * mp; dB[it] = d.B * mp; dC[it] = d.C * mp;
        if (own) ss += (double)mp * ssim_loss_pixel(m);
    }

    const double total = block_sum(ss, red);         // (its barrier: every read of rs lies before it, too)
    if (tid == 0) A.partial[blockIdx.x] = total;
    if constexpr (!GRAD) return;

#pragma unroll
    for (int it = 0; it < PER_THREAD; ++it) {
        const int i = tid + it * THREADS;
        if (i < DH * DW) { dm[i] = dA[it]; dm[DH * DW + i] = dB[it]; dm[2 * DH * DW + i] = dC[it]; }
    }
    __syncthreads();

    for (int i = tid; i < DH * TW; i += THREADS) {                       // A, B, C along the rows
        const int r = i / TW, c = i % TW;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float t[SSIM_TAPS];
#pragma unroll
            for (int k = 0; k < SSIM_TAPS; ++k) t[k] = dm[(j * DH + r) * DW + c + k];
            br[(j * DH + r) * TW + c] = ssim_filter(A.win.w, t);
        }
    }
    __syncthreads();

    for (int o = tid; o < TH * TW; o += THREADS) {                       // along the columns, then the gradient times m_q
        const int oy = o / TW, ox = o % TW;
        const int y = y0 + oy, x = x0 + ox;
        if (y < A.H && x < A.W) {
            float f[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                float t[SSIM_TAPS];
#pragma unroll
                for (int k = 0; k < SSIM_TAPS; ++k) t[k] = br[(j * DH + oy + k) * TW + ox];
                f[j] = ssim_filter(A.win.w, t);
            }
            const int q = (oy + SSIM_HALO) * IN_W + ox + IN_X0;
            const float mq = pm[(long long)y * A.W + x];
            A.grad[(plane * A.H + y) * A.W + x] = ssim_grad_pixel(f[0], f[1], f[2], sa[q], sb[q], A.scale) * mq;
        }
    }
}

// -> the number of workgroups (0: refused or N == 0) and the tile counts
long long term_tiles(int N, int H, int W, int *tiles_x, int *tiles_y) {
    if (N < 0 || H <= 0 || W <= 0 || (long long)H * W >= (1LL << 31)) return 0;
    *tiles_x = (W + TW - 1) / TW;
    *tiles_y = (H + TH - 1) / TH;
    return (long long)N * 3 * *tiles_x * *tiles_y;
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
    hipLaunchKernelGGL(masked_finish_kernel, dim3(1), dim3(THREADS), 0, s, (const double *)workspace, blocks, scale, 1.0, value);
    return dbw_check_launch("masked_finish_kernel");
}

extern "C" size_t dbw_monitor_masked_ssim_term_workspace_bytes(int N, int H, int W) {
    int tiles_x, tiles_y;
    const long long blocks = term_tiles(N, H, W, &tiles_x, &tiles_y);
    return blocks > 0 && blocks < (1LL << 31) ? (size_t)blocks * sizeof(double) : 0;
}

extern "C" int dbw_monitor_masked_ssim_term(const float *target, const float *rec, const float *masks, int N, int H, int W, double count,
                                            void *workspace, float *grad, double *value, dbw_stream_t stream) {
    DBW_REQUIRE(target && rec && masks && value, "null pointer");
    DBW_REQUIRE(N >= 0 && H > 0 && W > 0 && (long long)H * W < (1LL << 31), "bad size");
    DBW_REQUIRE(count >= 0.0 && count - count == 0.0, "count is negative or not finite");
    TermArgs A;
    const long long blocks = term_tiles(N, H, W, &A.tiles_x, &A.tiles_y);
    DBW_REQUIRE(blocks < (1LL << 31), "more than 2^31 tiles");
    DBW_REQUIRE(((uintptr_t)value & 7) == 0, "value is not 8-byte aligned");
    if (N == 0) return DBW_OK;                      // (nothing is launched, value stays as it is)
    DBW_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "workspace: null or not 8-byte aligned");
    DBW_REQUIRE(aligned4(target) && aligned4(rec) && aligned4(masks) && aligned4(grad), "misaligned pointer");
    A.a = target; A.b = rec; A.msk = masks; A.grad = grad; A.partial = (double *)workspace; A.win = ssim_window();
    A.scale = count > 0.0 ? -1.0 / count : 0.0; A.H = H; A.W = W;
    const bool vec = W % 4 == 0 && aligned16(target) && aligned16(rec) && aligned16(masks);
    const dim3 g((unsigned)blocks), b(THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (grad) {
        if (vec) hipLaunchKernelGGL((masked_ssim_term_kernel<true, true>), g, b, 0, s, A);
        else hipLaunchKernelGGL((masked_ssim_term_kernel<false, true>), g, b, 0, s, A);
    } else {
        if (vec) hipLaunchKernelGGL((masked_ssim_term_kernel<true, false>), g, b, 0, s, A);
        else hipLaunchKernelGGL((masked_ssim_term_kernel<false, false>), g, b, 0, s, A);
    }
    const int rc = dbw_check_launch("masked_ssim_term_kernel");
    if (rc != DBW_OK) return rc;
    hipLaunchKernelGGL(masked_finish_kernel, dim3(1), dim3(THREADS), 0, s, (const double *)workspace, blocks, 1.0, count, value);
    return dbw_check_launch("masked_finish_kernel");
}
