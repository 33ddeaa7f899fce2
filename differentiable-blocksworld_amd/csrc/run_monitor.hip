// Run monitor (include/dbw_monitor.h): image scores of rendered against held-out views, and the running loss table.  The arithmetic is
// score_math.h (host + device).
//
// dbw_image_scores: a workgroup of 256 threads owns a 16 x 32 tile of SSIM outputs of one channel of one image.  It loads the a and b
// tile with the 10-pixel halo into LDS once (26 rows of 48 floats each: the halo start rounded down to a multiple of 4 columns, so that a
// row moves as 12 16-byte loads where W and the pointers allow it), adds the squared error of the pixels it owns while they pass through
// registers, filters the five statistics along the rows into a second LDS array (5 x 26 x 32), then along the columns into registers, and
// forms the per-pixel SSIM there: no statistic plane goes to memory.  The two sums are reduced over the wave with fixed-order butterflies,
// over the four waves in wave order, and leave as one fp64 pair per workgroup; a second launch adds the pairs of each image in index
// order.  No atomics: the bits do not depend on the schedule.
//
// LDS: 2 x 26 x 48 + 5 x 26 x 32 floats = 26.6 KB per workgroup.  Row pass: a wave reads 2 rows x 32 consecutive columns per tap, column
// pass: 2 rows x 32 consecutive columns of a 32-float-wide plane -- consecutive banks within each 32-lane half, no conflicts.
#include "dbw_common.h"
#include "score_math.h"
#include "../../include/dbw_monitor.h"

namespace {

using namespace dbw;

constexpr int TW = 32, TH = 16;                     // outputs per workgroup
constexpr int IN_H = TH + SSIM_HALO;                // 26 input rows
constexpr int IN_W = 48;                            // input columns kept: 8 (padding: 5 of halo, rounded to 4) + 32 + 5 of halo, or 32 + 10
constexpr int THREADS = 256;

struct ScoreArgs {
    const float *a, *b;
    float *map;
    double *partial;
    SsimWindow win;
    int N, H, W, Hp, Wp, pad, tiles_x, tiles_y;
};

template <bool VEC>
__global__ void __launch_bounds__(THREADS) image_scores_kernel(ScoreArgs A) {
    __shared__ __align__(16) float sa[IN_H * IN_W];
    __shared__ __align__(16) float sb[IN_H * IN_W];
    __shared__ float rs[5][IN_H][TW];
    __shared__ double red[THREADS / DBW_WAVE][2];
    const int tid = threadIdx.x;
    const int tx = (int)(blockIdx.x % A.tiles_x), ty = (int)((blockIdx.x / A.tiles_x) % A.tiles_y);
    const long long plane = blockIdx.x / ((unsigned)A.tiles_x * A.tiles_y);          // n * 3 + channel
    const int x0 = tx * TW, y0 = ty * TH;
    const int xs = x0 - (A.pad ? 8 : 0), ys = y0 - (A.pad ? SSIM_HALO / 2 : 0), sh = A.pad ? 3 : 0;
    // the input pixels whose squared error this workgroup adds: its own 16 x 32, the last tile of a row / column takes what is left
    const int oy1 = ty == A.tiles_y - 1 ? A.H : y0 + TH, ox1 = tx == A.tiles_x - 1 ? A.W : x0 + TW;
    const float *pa = A.a + plane * A.H * A.W, *pb = A.b + plane * A.H * A.W;
    double se = 0.0, ss = 0.0;

    if constexpr (VEC) {
        for (int i = tid; i < IN_H * (IN_W / 4); i += THREADS) {
            const int r = i / (IN_W / 4), q = i % (IN_W / 4);
            const int y = ys + r, x = xs + 4 * q;
            float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
            if (y >= 0 && y < A.H && x >= 0 && x < A.W) {              // (W % 4 == 0 and x % 4 == 0: the four are inside together)
                va = *(const float4 *)(pa + (long long)y * A.W + x);
                vb = *(const float4 *)(pb + (long long)y * A.W + x);
                if (y >= y0 && y < oy1 && x >= x0 && x < ox1)         // (x0, ox1 multiples of 4 too)
                    se += sq_err(va.x, vb.x) + sq_err(va.y, vb.y) + sq_err(va.z, vb.z) + sq_err(va.w, vb.w);
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
                if (y >= y0 && y < oy1 && x >= x0 && x < ox1) se += sq_err(va, vb);
            }
            sa[i] = va;
            sb[i] = vb;
        }
    }
    __syncthreads();

    for (int i = tid; i < IN_H * TW; i += THREADS) {                    // rows
        const int r = i / TW, c = i % TW;
        float t[5][SSIM_TAPS];
#pragma unroll
        for (int k = 0; k < SSIM_TAPS; ++k) {
            float s[5];
            ssim_stats(sa[r * IN_W + c + sh + k], sb[r * IN_W + c + sh + k], s);
#pragma unroll
            for (int j = 0; j < 5; ++j) t[j][k] = s[j];
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) rs[j][r][c] = ssim_filter(A.win.w, t[j]);
    }
    __syncthreads();

    for (int o = tid; o < TH * TW; o += THREADS) {                      // columns, then the pixel
        const int oy = o / TW, ox = o % TW;
        const int y = y0 + oy, x = x0 + ox;
        if (y < A.Hp && x < A.Wp) {
            float m[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                float t[SSIM_TAPS];
#pragma unroll
                for (int k = 0; k < SSIM_TAPS; ++k) t[k] = rs[j][oy + k][ox];
                m[j] = ssim_filter(A.win.w, t);
            }
            const float v = ssim_pixel(m);
            if (A.map) A.map[(plane * A.Hp + y) * A.Wp + x] = v;
            ss += (double)v;
        }
    }

#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        se += __shfl_xor(se, off, DBW_WAVE);
        ss += __shfl_xor(ss, off, DBW_WAVE);
    }
    if ((tid & (DBW_WAVE - 1)) == 0) { red[tid / DBW_WAVE][0] = se; red[tid / DBW_WAVE][1] = ss; }
    __syncthreads();
    if (tid == 0) {
        double t0 = red[0][0], t1 = red[0][1];
        for (int w = 1; w < THREADS / DBW_WAVE; ++w) { t0 += red[w][0]; t1 += red[w][1]; }
        A.partial[2 * (long long)blockIdx.x] = t0;
        A.partial[2 * (long long)blockIdx.x + 1] = t1;
    }
}

// out[n] = the pairs of image n added in index order; one thread per image
__global__ void __launch_bounds__(DBW_WAVE) image_scores_finish_kernel(const double *__restrict__ partial, int N, int per_image, double *__restrict__ out) {
    const int n = blockIdx.x * DBW_WAVE + threadIdx.x;
    if (n >= N) return;
    const double *p = partial + 2 * (long long)n * per_image;
    double se = 0.0, ss = 0.0;
    for (int i = 0; i < per_image; ++i) { se += p[2 * i]; ss += p[2 * i + 1]; }
    out[2 * n] = se;
    out[2 * n + 1] = ss;
}

struct MeterArgs {
    const float *vals[DBW_METER_MAX_VALUES];
};

__global__ void __launch_bounds__(DBW_WAVE) meter_add_kernel(double *__restrict__ table, MeterArgs A, int n, double weight, double step) {
    const int i = threadIdx.x;
    bool bad = false;
    if (i < n) {
        const float v = *A.vals[i];
        bad = !meter_finite(v);
        table[i] = meter_add(table[i], v, weight);
    }
    const bool any_bad = __ballot(bad) != 0ull;
    if (i == 0) {
        table[n] = table[n] + weight;
        if (any_bad && table[n + 1] < 0.0) table[n + 1] = step;
    }
}

__global__ void __launch_bounds__(DBW_WAVE) meter_reset_kernel(double *__restrict__ table, int n) {
    const int i = threadIdx.x;
    if (i <= n) table[i] = 0.0;
    if (i == n + 1) table[i] = -1.0;
}

// -> the number of workgroups (0: refused), the output size and the tile counts
long long score_tiles(int N, int H, int W, int padding, int *Hp, int *Wp, int *tiles_x, int *tiles_y) {
    if (N < 0 || H <= 0 || W <= 0 || (padding != 0 && padding != 1) || (long long)H * W >= (1LL << 31)) return 0;
    if (!padding && (H < SSIM_TAPS || W < SSIM_TAPS)) return 0;
    *Hp = padding ? H : H - SSIM_HALO;
    *Wp = padding ? W : W - SSIM_HALO;
    *tiles_x = (*Wp + TW - 1) / TW;
    *tiles_y = (*Hp + TH - 1) / TH;
    return (long long)N * 3 * *tiles_x * *tiles_y;
}

}  // namespace

extern "C" int dbw_monitor_abi_version(void) { return DBW_MONITOR_ABI_VERSION; }      // (history: include/dbw_monitor.h)

extern "C" size_t dbw_image_scores_workspace_bytes(int N, int H, int W, int padding) {
    int Hp, Wp, tiles_x, tiles_y;
    const long long blocks = score_tiles(N, H, W, padding, &Hp, &Wp, &tiles_x, &tiles_y);
    return blocks > 0 && blocks < (1LL << 31) ? (size_t)blocks * 2 * sizeof(double) : 0;
}

extern "C" int dbw_image_scores(const float *a, const float *b, int N, int H, int W, int padding, void *workspace, float *ssim_map, double *out,
                                dbw_stream_t stream) {
    DBW_REQUIRE(a && b && out, "null pointer");
    DBW_REQUIRE(N >= 0 && H > 0 && W > 0 && (long long)H * W < (1LL << 31), "bad size");
    DBW_REQUIRE(padding == 0 || padding == 1, "padding must be 0 or 1");
    DBW_REQUIRE(padding || (H >= SSIM_TAPS && W >= SSIM_TAPS), "without padding an image must hold one 11 x 11 window: H >= 11 and W >= 11");
    ScoreArgs A;
    const long long blocks = score_tiles(N, H, W, padding, &A.Hp, &A.Wp, &A.tiles_x, &A.tiles_y);
    DBW_REQUIRE(blocks < (1LL << 31), "more than 2^31 tiles");
    if (N == 0) return DBW_OK;
    DBW_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "workspace: null or not 8-byte aligned");
    DBW_REQUIRE(((uintptr_t)a & 3) == 0 && ((uintptr_t)b & 3) == 0 && ((uintptr_t)ssim_map & 3) == 0 && ((uintptr_t)out & 7) == 0, "misaligned pointer");
    A.a = a; A.b = b; A.map = ssim_map; A.partial = (double *)workspace; A.win = ssim_window();
    A.N = N; A.H = H; A.W = W; A.pad = padding;
    const bool vec = W % 4 == 0 && aligned16(a) && aligned16(b);
    if (vec) hipLaunchKernelGGL(image_scores_kernel<true>, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(image_scores_kernel<false>, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, A);
    const int rc = dbw_check_launch("image_scores_kernel");
    if (rc != DBW_OK) return rc;
    hipLaunchKernelGGL(image_scores_finish_kernel, dim3((unsigned)((N + DBW_WAVE - 1) / DBW_WAVE)), dim3(DBW_WAVE), 0, (hipStream_t)stream,
                       (const double *)workspace, N, 3 * A.tiles_x * A.tiles_y, out);
    return dbw_check_launch("image_scores_finish_kernel");
}

extern "C" int dbw_meter_add(double *table, const float *const *vals, int n, double weight, int64_t step, dbw_stream_t stream) {
    DBW_REQUIRE(table && vals, "null pointer");
    DBW_REQUIRE(n >= 1 && n <= DBW_METER_MAX_VALUES, "n must be in 1 .. 16");
    DBW_REQUIRE(((uintptr_t)table & 7) == 0, "table is not 8-byte aligned");
    DBW_REQUIRE(step >= 0, "step must not be negative");
    MeterArgs A;
    for (int i = 0; i < DBW_METER_MAX_VALUES; ++i) {
        A.vals[i] = i < n ? vals[i] : nullptr;
        DBW_REQUIRE(i >= n || (vals[i] && ((uintptr_t)vals[i] & 3) == 0), "vals: null or misaligned value pointer");
    }
    hipLaunchKernelGGL(meter_add_kernel, dim3(1), dim3(DBW_WAVE), 0, (hipStream_t)stream, table, A, n, weight, (double)step);
    return dbw_check_launch("meter_add_kernel");
}

extern "C" int dbw_meter_reset(double *table, int n, dbw_stream_t stream) {
    DBW_REQUIRE(table, "null pointer");
    DBW_REQUIRE(n >= 1 && n <= DBW_METER_MAX_VALUES, "n must be in 1 .. 16");
    DBW_REQUIRE(((uintptr_t)table & 7) == 0, "table is not 8-byte aligned");
    hipLaunchKernelGGL(meter_reset_kernel, dim3(1), dim3(DBW_WAVE), 0, (hipStream_t)stream, table, n);
    return dbw_check_launch("meter_reset_kernel");
}
