// SSIM as the perceptual term, plain and under a validity mask (include/dbw_monitor.h: dbw_monitor_ssim_term, dbw_monitor_masked_ssim_term):
//   plain:   L = mean over n, c, y, x of (1 - SSIM(a, b)) with zero padding,
//   masked:  L = sum over n, c, p of m_p (1 - SSIM_p(m a, m b)) / count,   masks (N,1,H,W) fp32 weights in [0, 1], count = 3 * sum(masks),
// and dL/db, in one launch of ONE tile kernel, ssim_term_kernel<VEC, GRAD, MASKED>.  The arithmetic is score_math.h (host + device):
// ssim_stats, ssim_filter, ssim_deriv, ssim_loss_pixel, ssim_grad_pixel.
//
// A workgroup of 256 threads owns a 16 x 32 tile of gradient outputs of one plane (n * 3 + channel).  The gradient at q gathers the
// derivative maps A, B, C of the 11 x 11 windows around q, and each of those the statistics of the 11 x 11 pixels around it: a 10-pixel
// halo.  The workgroup
//   1. loads a and b over 36 x 52 (kept as 36 rows of 56 floats: the start rounded down to a multiple of 4 columns, so that a row moves
//      as 14 16-byte loads where W and the pointers allow it), zero outside the image;
//   2. filters the five statistics along the rows into rs (5 x 36 x 42), then along the columns into registers, for the 26 x 42 windows
//      of tile + 5, and forms S, A, B, C there (zero for a window centred outside the image); the 16 x 32 windows it owns add 1 - S, formed
//      in fp64, to the value;
//   3. writes A, B, C over rs (3 x 26 x 42), filters them along the rows (3 x 26 x 32, behind them in the same space) and along the
//      columns, combines with a_q, b_q from the input tile and stores the gradient once.
// No statistic or derivative plane goes to memory.  The value is reduced over the workgroup in a fixed order (loss_reduce.h: block_sums)
// and leaves as one fp64 partial per workgroup; a second launch of one workgroup adds the partials in a fixed order and divides
// (partials_finish_kernel).  No atomics: the bits do not depend on the schedule.  With grad == NULL step 3 and the windows outside the own
// tile are skipped; the own windows see the same operations in the same order: the same value bits.
//
// The mask enters three times, each under `if constexpr (MASKED)` -- the plain instantiations hold no mask load and no multiply:
//   a. the inputs are multiplied by m as they are loaded into the tile (16 bytes of the mask beside a and b where they move so);
//   b. S's derivative maps A, B, C and 1 - S of the window centred at p are multiplied by m_p;
//   c. the gradient at q is multiplied by m_q.
// The mask is NOT kept in LDS: it is a third of an image plane, shared by the three channels, and each of the three uses reads it from
// memory at the index the lane already has.  count is a host number: no kernel reads a device scalar for it, and count == 0 gives 0 and a
// zero gradient without a division.  With a mask of ones every product is exact: the masked gradient and value are the plain ones bit
// for bit.
//
// LDS: 2 x 36 x 56 + 5 x 36 x 42 floats = 46.4 KB per workgroup (three workgroups per CU), with and without the mask.  Row passes read
// consecutive columns of one or two rows per wave, column passes consecutive columns of a 42- or 32-float-wide plane.
#include "dbw_common.h"
#include "loss_reduce.h"
#include "score_math.h"
#include "../../include/dbw_monitor.h"

namespace {

using namespace dbw;

constexpr int TW = 32, TH = 16;                     // gradient outputs per workgroup
constexpr int RAD = SSIM_TAPS / 2;                  // 5
constexpr int DW = TW + SSIM_HALO, DH = TH + SSIM_HALO;       // 42 x 26 windows: tile + 5
constexpr int IN_H = TH + 2 * SSIM_HALO;            // 36 input rows
constexpr int IN_W = 56;                            // input columns kept: 12 (10 of halo, rounded to 4) + 32 + 10, rounded to 4
constexpr int IN_X0 = 12, SH = IN_X0 - SSIM_HALO;   // tile column 0 in the input tile; first column the row pass reads
constexpr int THREADS = LOSS_THREADS;
constexpr int PER_THREAD = (DH * DW + THREADS - 1) / THREADS;           // 5 windows per thread
static_assert(3 * DH * DW + 3 * DH * TW <= 5 * IN_H * DW, "the derivative maps and their row pass share the space of rs");
static_assert(SH >= 0 && DW - 1 + SH + SSIM_HALO < IN_W && IN_W % 4 == 0, "input tile too narrow");

struct TermArgs {
    const float *a, *b, *msk;                       // msk: read by the MASKED instantiations only
    float *grad;
    double *partial;
    SsimWindow win;
    double scale;                                   // -1 / M; masked: -1 / count (0 where count is 0)
    int H, W, tiles_x, tiles_y;
};

template <bool VEC, bool GRAD, bool MASKED>
__global__ void __launch_bounds__(THREADS) ssim_term_kernel(TermArgs A) {
    __shared__ __align__(16) float sa[IN_H * IN_W];
    __shared__ __align__(16) float sb[IN_H * IN_W];
    __shared__ float rs[5 * IN_H * DW];
    __shared__ double red[LOSS_WAVES][1];
    float *const dm = rs;                           // [3][DH][DW], once rs has been read
    float *const br = rs + 3 * DH * DW;             // [3][DH][TW]
    const int tid = threadIdx.x;
    const int tx = (int)(blockIdx.x % A.tiles_x), ty = (int)((blockIdx.x / A.tiles_x) % A.tiles_y);
    const long long plane = blockIdx.x / ((unsigned)A.tiles_x * A.tiles_y);          // n * 3 + channel
    const int x0 = tx * TW, y0 = ty * TH;
    const int xs = x0 - IN_X0, ys = y0 - SSIM_HALO;
    const float *pa = A.a + plane * A.H * A.W, *pb = A.b + plane * A.H * A.W;
    [[maybe_unused]] const float *pm = nullptr;      // the image's mask plane, shared by its three channels
    if constexpr (MASKED) pm = A.msk + (plane / 3) * A.H * A.W;

    if constexpr (VEC) {
        for (int i = tid; i < IN_H * (IN_W / 4); i += THREADS) {
            const int r = i / (IN_W / 4), q = i % (IN_W / 4);
            const int y = ys + r, x = xs + 4 * q;
            float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
            if (y >= 0 && y < A.H && x >= 0 && x < A.W) {              // (W % 4 == 0 and x % 4 == 0: the four are inside together)
                va = *(const float4 *)(pa + (long long)y * A.W + x);
                vb = *(const float4 *)(pb + (long long)y * A.W + x);
                if constexpr (MASKED) {
                    const float4 vm = *(const float4 *)(pm + (long long)y * A.W + x);
                    va.x *= vm.x; va.y *= vm.y; va.z *= vm.z; va.w *= vm.w;
                    vb.x *= vm.x; vb.y *= vm.y; vb.z *= vm.z; vb.w *= vm.w;
                }
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
                va = pa[(long long)y * A.W + x];
                vb = pb[(long long)y * A.W + x];
                if constexpr (MASKED) {
                    const float vm = pm[(long long)y * A.W + x];
                    va *= vm;
                    vb *= vm;
                }
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

    // along the columns, then the window: S and the derivative maps (MASKED: times the window's own weight m_p), kept in registers until
    // every thread has read rs
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
        [[maybe_unused]] float mp = 0.f;
        if constexpr (MASKED) mp = pm[(long long)y * A.W + x];
        float m[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            float t[SSIM_TAPS];
#pragma unroll
            for (int k = 0; k < SSIM_TAPS; ++k) t[k] = rs[(j * IN_H + dy + k) * DW + dx];
            m[j] = ssim_filter(A.win.w, t);
        }
        const SsimDeriv d = ssim_deriv(m);
        if constexpr (MASKED) {
            dA[it] = d.A * mp; dB[it] = d.B * mp; dC[it] = d.C * mp;
            if (own) ss += (double)mp * ssim_loss_pixel(m);
        } else {
            dA[it] = d.A; dB[it] = d.B; dC[it] = d.C;
            if (own) ss += ssim_loss_pixel(m);
        }
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

    for (int o = tid; o < TH * TW; o += THREADS) {                       // along the columns, then the gradient (MASKED: times m_q)
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
            if constexpr (MASKED) {
                const float mq = pm[(long long)y * A.W + x];
                A.grad[(plane * A.H + y) * A.W + x] = ssim_grad_pixel(f[0], f[1], f[2], sa[q], sb[q], A.scale) * mq;
            } else {
                A.grad[(plane * A.H + y) * A.W + x] = ssim_grad_pixel(f[0], f[1], f[2], sa[q], sb[q], A.scale);
            }
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

size_t term_workspace_bytes(int N, int H, int W) {
    int tiles_x, tiles_y;
    const long long blocks = term_tiles(N, H, W, &tiles_x, &tiles_y);
    return blocks > 0 && blocks < (1LL << 31) ? (size_t)blocks * sizeof(double) : 0;
}

template <bool GRAD, bool MASKED>
void launch_tiles(const TermArgs &A, bool vec, long long blocks, hipStream_t s) {
    const dim3 g((unsigned)blocks), b(THREADS);
    if (vec) hipLaunchKernelGGL((ssim_term_kernel<true, GRAD, MASKED>), g, b, 0, s, A);
    else hipLaunchKernelGGL((ssim_term_kernel<false, GRAD, MASKED>), g, b, 0, s, A);
}

// both entry points behind their checks: the tile launch of the instantiation that A asks for (msk, grad: there or null), then
// value[0] = (the sum of the partials) / div, 0 where div is 0
int term_launch(const TermArgs &A, long long blocks, bool vec, double div, double *value, dbw_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (A.msk) {
        if (A.grad) launch_tiles<true, true>(A, vec, blocks, s);
        else launch_tiles<false, true>(A, vec, blocks, s);
    } else {
        if (A.grad) launch_tiles<true, false>(A, vec, blocks, s);
        else launch_tiles<false, false>(A, vec, blocks, s);
    }
    const int rc = dbw_check_launch("ssim_term_kernel");
    if (rc != DBW_OK) return rc;
    return partials_finish(A.partial, blocks, 1.0, div, value, s);
}

}  // namespace

extern "C" size_t dbw_monitor_ssim_term_workspace_bytes(int N, int H, int W) { return term_workspace_bytes(N, H, W); }

extern "C" int dbw_monitor_ssim_term(const float *target, const float *rec, int N, int H, int W, void *workspace, float *grad, double *value,
                                     dbw_stream_t stream) {
    DBW_REQUIRE(target && rec && value, "null pointer");
    DBW_REQUIRE(N >= 0 && H > 0 && W > 0 && (long long)H * W < (1LL << 31), "bad size");
    TermArgs A;
    const long long blocks = term_tiles(N, H, W, &A.tiles_x, &A.tiles_y);
    DBW_REQUIRE(blocks < (1LL << 31), "more than 2^31 tiles");
    DBW_REQUIRE(((uintptr_t)value & 7) == 0, "value is not 8-byte aligned");
    if (N == 0) return DBW_OK;                      // (a mean over nothing: nothing is launched, value stays as it is)
    DBW_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "workspace: null or not 8-byte aligned");
    DBW_REQUIRE(aligned4(target) && aligned4(rec) && aligned4(grad), "misaligned pointer");
    const double M = (double)N * 3.0 * (double)H * (double)W;
    A.a = target; A.b = rec; A.msk = nullptr; A.grad = grad; A.partial = (double *)workspace; A.win = ssim_window();
    A.scale = -1.0 / M; A.H = H; A.W = W;
    return term_launch(A, blocks, W % 4 == 0 && aligned16(target) && aligned16(rec), M, value, stream);
}

extern "C" size_t dbw_monitor_masked_ssim_term_workspace_bytes(int N, int H, int W) { return term_workspace_bytes(N, H, W); }

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
    return term_launch(A, blocks, W % 4 == 0 && aligned16(target) && aligned16(rec) && aligned16(masks), count, value, stream);
}
