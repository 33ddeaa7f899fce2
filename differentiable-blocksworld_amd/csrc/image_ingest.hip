// Image ingest (include/dbw_ingest.h): raw (N,Hin,Win,3) uint8 frames -> the training targets (N,3,Hout,Wout) fp32 and / or resized uint8
// frames, with Pillow's antialiased BILINEAR resample restated bit for bit.  The arithmetic is resample_math.h (host + device).
//
// Two forms, the same bytes:
//  * general: resample_h_kernel writes the horizontally resampled rows the vertical pass reads as an 8-bit intermediate into the workspace,
//    resample_v_kernel resamples it vertically and converts.  One thread per output pixel, its table row read per lane: any ratio.
//  * fused (tables of at most DBW_RESAMPLE_FUSED_MAX_KSIZE weights): one workgroup of 4 waves owns a tile of FT_H x FT_W output pixels.
//    It copies the source rectangle the tile reads into LDS -- dwords where the row's address allows it, put together from bytes at the
//    ragged ends, each row at its own offset so that global and LDS dwords line up; four loads in flight per thread --, runs the
//    horizontal pass out of it into a planar 8-bit LDS tile and the vertical pass out of that.  In both passes a wave works on ONE output
//    column (row) at a time, lanes across the rows (columns): the table row is wave-uniform and comes through scalar loads, all of its
//    weights requested before the first is used, and the fp32 planes are written 64 consecutive floats per store.  The kernel is compiled
//    per table width (3 .. 11) and runs that many taps for every sample without a branch, the ones past a sample's own count with
//    weight 0: its LDS reads are in flight together (with a loop over the sample's own count, one scalar load and one LDS read were
//    waited for per tap, and the kernel took 0.74 ms instead of 0.50 ms for a DTU scan, profiles/ingest.md).
//    No scratch; LDS row strides are an odd number of dwords.
#include "dbw_common.h"
#include "resample_math.h"
#include "../../include/dbw_ingest.h"

namespace {

using namespace dbw;

constexpr int FT_H = 8, FT_W = 64;      // output tile of the fused form
constexpr int FT_WP = FT_W + 4;         // bytes per row of the intermediate planes: 17 dwords
constexpr int FUSED_LDS_MAX = 64 * 1024;

// (the pointers are kernel parameters of their own, __restrict__: the table reads then are provably untouched by the kernel's stores, and a
// wave-uniform one becomes a scalar load)
struct ResampleArgs {
    int N, Hin, Win, Hout, Wout, kx, ky;
    int rows_max, cols_max, src_stride; // fused form: the largest source rectangle of a tile, bytes per LDS source row
};

__device__ const int32_t IDENTITY_K[1] = {RESAMPLE_ONE};

// The taps of output sample i of one axis: input samples [lo, lo + n), weights k.  Clamped to the axis and the table's width, so that no
// table content can send a read out of bounds.
struct Taps {
    int lo, n, width;                   // width: the weights that may be read at k (the table's ksize; 1 for the identity)
    const int32_t *k;
};
__device__ __forceinline__ Taps taps(const int32_t *__restrict__ table, int ksize, int i, int in_size) {
    Taps t;
    if (!table) {
        t.lo = i < in_size ? i : in_size - 1; t.n = 1; t.width = 1; t.k = IDENTITY_K;
        return t;
    }
    const int32_t *row = table + (long long)i * (ksize + 2);
    const int lo = row[0], n = row[1];
    t.lo = lo < 0 ? 0 : (lo > in_size - 1 ? in_size - 1 : lo);
    const int room = in_size - t.lo, nn = n < ksize ? n : ksize;
    t.n = nn < room ? nn : room;
    t.width = ksize;
    t.k = row + 2;
    return t;
}

// ---- general form -------------------------------------------------------------------------------------------------------------------------
// rows [y_first, y_first + n_rows) of every image, horizontally resampled: tmp (N, n_rows, Wout, 3)
__global__ void __launch_bounds__(256) resample_h_kernel(ResampleArgs A, const uint8_t *__restrict__ src, const int32_t *__restrict__ tx, int y_first, int n_rows,
                                                         uint8_t *__restrict__ tmp, long long total) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int xo = (int)(g % A.Wout);
    const long long row = g / A.Wout;                     // n * n_rows + (y - y_first)
    const long long n = row / n_rows;
    const int y = y_first + (int)(row % n_rows);
    const Taps t = taps(tx, A.kx, xo, A.Win);
    const uint8_t *px = src + ((n * A.Hin + y) * A.Win + t.lo) * 3;
    uint8_t *dst = tmp + g * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c] = resample_dot(px + c, 3, t.k, t.n);
}

// in (N, n_rows, Wout, 3), holding the rows from y_first on, vertically resampled and converted
__global__ void __launch_bounds__(256) resample_v_kernel(ResampleArgs A, const uint8_t *__restrict__ in, const int32_t *__restrict__ ty, int y_first, int n_rows,
                                                         float *__restrict__ out_f32, uint8_t *__restrict__ out_u8, long long total) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int xo = (int)(g % A.Wout);
    const long long row = g / A.Wout;                     // n * Hout + yo
    const long long n = row / A.Hout;
    const int yo = (int)(row % A.Hout);
    const Taps t = taps(ty, A.ky, yo, A.Hin);
    int lo = t.lo - y_first;
    lo = lo < 0 ? 0 : (lo > n_rows - 1 ? n_rows - 1 : lo);
    const int cn = t.n < n_rows - lo ? t.n : n_rows - lo;
    const uint8_t *px = in + ((n * n_rows + lo) * A.Wout + xo) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint8_t v = resample_dot(px + c, (long long)A.Wout * 3, t.k, cn);
        if (out_u8) out_u8[g * 3 + c] = v;
        if (out_f32) out_f32[((n * 3 + c) * A.Hout + yo) * A.Wout + xo] = resample_to_float(v);
    }
}

// ---- fused form ---------------------------------------------------------------------------------------------------------------------------
// The first K weights of a wave-uniform table row, all requested at once (scalar loads whose latencies overlap) and without a branch: the
// index is clamped to the row's width, and a weight past the cn taps in use is 0.
template <int K>
__device__ __forceinline__ void load_weights(const Taps &t, int cn, int32_t (&k)[K]) {
#pragma unroll
    for (int x = 0; x < K; ++x) {
        const int32_t w = t.k[x < t.width ? x : t.width - 1];
        k[x] = x < cn ? w : 0;
    }
}
// The tap a weight of 0 multiplies: the last one in use (any address inside the tile would do).
__device__ __forceinline__ int tap_index(int x, int cn) { return x < cn ? x : (cn > 0 ? cn - 1 : 0); }

// K: the wider of the two tables' widths (3, 5, 7, 9 or 11).  Every output sample runs K taps without a branch -- the LDS reads of a
// sample are independent and in flight together --, the ones past its own count with weight 0.
template <int K>
__global__ void __launch_bounds__(256) resample_fused_kernel(ResampleArgs A, const uint8_t *__restrict__ src, const int32_t *__restrict__ tx,
                                                             const int32_t *__restrict__ ty, float *__restrict__ out_f32, uint8_t *__restrict__ out_u8,
                                                             int tiles_x, int tiles_y) {
    extern __shared__ __align__(16) uint8_t lds[];
    uint8_t *lsrc = lds;                                              // [rows_max][src_stride]: the source rectangle, interleaved rgb
    uint8_t *lmid = lds + (size_t)A.rows_max * A.src_stride;          // [3][rows_max][FT_WP]: after the horizontal pass, planar
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int tile_x = blockIdx.x % tiles_x, tile_y = (blockIdx.x / tiles_x) % tiles_y;
    const long long n = blockIdx.x / (tiles_x * tiles_y);
    const int ox0 = tile_x * FT_W, oy0 = tile_y * FT_H;
    const int ow = A.Wout - ox0 < FT_W ? A.Wout - ox0 : FT_W, oh = A.Hout - oy0 < FT_H ? A.Hout - oy0 : FT_H;
    // the source rectangle: first tap of the first output sample to last tap of the last one (both bounds grow with the sample)
    const Taps xf = taps(tx, A.kx, ox0, A.Win), xl = taps(tx, A.kx, ox0 + ow - 1, A.Win);
    const Taps yf = taps(ty, A.ky, oy0, A.Hin), yl = taps(ty, A.ky, oy0 + oh - 1, A.Hin);
    const int x0 = xf.lo, y0 = yf.lo;
    int cols = xl.lo + xl.n - x0, rows = yl.lo + yl.n - y0;
    cols = cols < 0 ? 0 : (cols > A.cols_max ? A.cols_max : cols);
    rows = rows < 0 ? 0 : (rows > A.rows_max ? A.rows_max : rows);
    const int len = cols * 3;
    const uint8_t *base = src + ((n * A.Hin + y0) * A.Win + x0) * 3;
    const long long row_bytes = (long long)A.Win * 3;

    // 1. source rectangle -> LDS.  Byte i of row r sits at lsrc[r * src_stride + a + i], a = the row's address mod 4: aligned global
    //    dwords land on aligned LDS dwords.  One unit = one LDS dword; a thread has four units' loads in flight before it stores them.
    //    A dword that lies inside the row is one load, one at a ragged end is put together from its bytes (the bytes of the LDS dword
    //    outside the row are never read).
    const int spr = A.src_stride >> 2, units = rows * spr;
    for (int u0 = threadIdx.x; u0 < units; u0 += 4 * 256) {
        uint32_t v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = u0 + i * 256;
            v[i] = 0u;
            if (u < units) {
                const int r = u / spr, s = u - r * spr;
                const uint8_t *g = base + r * row_bytes;
                const int b0 = 4 * s - (int)((uintptr_t)g & 3);
                if (b0 >= 0 && b0 + 4 <= len) {
                    v[i] = *(const uint32_t *)(g + b0);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (b0 + j >= 0 && b0 + j < len) v[i] |= (uint32_t)g[b0 + j] << (8 * j);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (u0 + i * 256 < units) ((uint32_t *)lsrc)[u0 + i * 256] = v[i];
    }
    __syncthreads();

    // 2. horizontal pass: a wave per output column, lanes across (source row, channel)
    for (int xo = wave; xo < ow; xo += 4) {
        const Taps t = taps(tx, A.kx, ox0 + xo, A.Win);
        int off = t.lo - x0;
        off = off > cols - 1 ? cols - 1 : off;
        off = off < 0 ? 0 : off;
        const int cn = t.n < cols - off ? t.n : cols - off;
        int32_t k[K];
        load_weights<K>(t, cn, k);
        for (int p = lane; p < rows * 3; p += 64) {
            const int r = p / 3, c = p - 3 * r;
            const int a = (int)((uintptr_t)(base + r * row_bytes) & 3);
            const uint8_t *px = lsrc + r * A.src_stride + a + off * 3 + c;
            int32_t acc = RESAMPLE_HALF;
#pragma unroll
            for (int x = 0; x < K; ++x) acc += (int32_t)px[3 * tap_index(x, cn)] * k[x];
            lmid[(c * A.rows_max + r) * FT_WP + xo] = resample_clip8(acc);
        }
    }
    __syncthreads();

    // 3. vertical pass and conversion: a wave per output row, lanes across the columns
    for (int yo = wave; yo < oh; yo += 4) {
        const Taps t = taps(ty, A.ky, oy0 + yo, A.Hin);
        int off = t.lo - y0;
        off = off > rows - 1 ? rows - 1 : off;
        off = off < 0 ? 0 : off;
        const int cn = t.n < rows - off ? t.n : rows - off;
        int32_t k[K];
        load_weights<K>(t, cn, k);
        if (lane < ow) {
            const long long opix = (n * A.Hout + oy0 + yo) * A.Wout + ox0 + lane;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint8_t *px = lmid + (c * A.rows_max + off) * FT_WP + lane;
                int32_t acc = RESAMPLE_HALF;
#pragma unroll
                for (int x = 0; x < K; ++x) acc += (int32_t)px[tap_index(x, cn) * FT_WP] * k[x];
                const uint8_t v = resample_clip8(acc);
                if (out_u8) out_u8[opix * 3 + c] = v;
                if (out_f32) out_f32[((n * 3 + c) * A.Hout + oy0 + yo) * A.Wout + ox0 + lane] = resample_to_float(v);
            }
        }
    }
}

// the input rows the vertical pass reads: [*first, *first + n)
int rows_read(int Hin, int Hout, int *first) {
    if (Hin == Hout) { *first = 0; return Hin; }
    int lo;
    const int n = resample_bounds(Hin, Hout, Hout - 1, &lo);
    resample_bounds(Hin, Hout, 0, first);
    return lo + n - *first;
}

// the largest source extent of a tile of T output samples
int extent_max(int in, int out, int T) {
    int m = 0;
    for (int t0 = 0; t0 < out; t0 += T) {
        const int last = (t0 + T < out ? t0 + T : out) - 1;
        int lo, lo_last;
        resample_bounds(in, out, t0, &lo);
        const int n = resample_bounds(in, out, last, &lo_last);
        if (lo_last + n - lo > m) m = lo_last + n - lo;
    }
    return m;
}

}  // namespace

extern "C" int dbw_ingest_abi_version(void) { return DBW_INGEST_ABI_VERSION; }      // (history: include/dbw_ingest.h)

extern "C" int dbw_resample_table(int in_size, int out_size, int32_t *table, size_t capacity_ints) {
    DBW_REQUIRE(in_size > 0 && out_size > 0, "bad size");
    const int ksize = resample_ksize(in_size, out_size);
    if (!table) return ksize;
    DBW_REQUIRE(capacity_ints >= (size_t)out_size * (size_t)(ksize + 2), "capacity_ints below out_size * (ksize + 2)");
    for (int xx = 0; xx < out_size; ++xx) resample_table_row(in_size, out_size, xx, ksize, table + (size_t)xx * (ksize + 2));
    return ksize;
}

extern "C" size_t dbw_images_resample_workspace_bytes(int N, int Hin, int Win, int Hout, int Wout) {
    if (N <= 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0 || Win == Wout) return 0;
    int first;
    return (size_t)N * (size_t)rows_read(Hin, Hout, &first) * (size_t)Wout * 3;
}

extern "C" int dbw_images_resample_u8(const uint8_t *src, int N, int Hin, int Win, int Hout, int Wout, const int32_t *table_x,
                                      const int32_t *table_y, float *out_f32, uint8_t *out_u8, void *workspace, size_t workspace_bytes, int form,
                                      dbw_stream_t stream) {
    DBW_REQUIRE(src, "null pointer");
    DBW_REQUIRE(out_f32 || out_u8, "at least one of out_f32 / out_u8");
    DBW_REQUIRE(N >= 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0 && (long long)Hin * Win < (1LL << 29) && (long long)Hout * Wout < (1LL << 29),
                "bad size");
    DBW_REQUIRE(table_x || Win == Wout, "table_x may be NULL only where Wout == Win");
    DBW_REQUIRE(table_y || Hin == Hout, "table_y may be NULL only where Hout == Hin");
    DBW_REQUIRE(form == DBW_RESAMPLE_AUTO || form == DBW_RESAMPLE_GENERAL || form == DBW_RESAMPLE_FUSED, "unknown form");
    ResampleArgs A;
    A.N = N; A.Hin = Hin; A.Win = Win; A.Hout = Hout; A.Wout = Wout;
    A.kx = resample_ksize(Win, Wout); A.ky = resample_ksize(Hin, Hout);
    A.rows_max = extent_max(Hin, Hout, FT_H); A.cols_max = extent_max(Win, Wout, FT_W);
    A.src_stride = (A.cols_max * 3 + 6 + 3) / 4 * 4;                         // the row, its offset of up to 3, whole dwords ...
    if ((A.src_stride / 4) % 2 == 0) A.src_stride += 4;                      // ... an odd number of them
    const size_t lds = (size_t)A.rows_max * A.src_stride + (size_t)3 * A.rows_max * FT_WP;
    const bool fits = A.kx <= DBW_RESAMPLE_FUSED_MAX_KSIZE && A.ky <= DBW_RESAMPLE_FUSED_MAX_KSIZE && lds <= (size_t)FUSED_LDS_MAX;
    if (form == DBW_RESAMPLE_FUSED && !fits) {
        dbw_set_error("dbw_images_resample_u8: the fused form takes tables of at most %d weights (ratios up to 5), these have %d and %d",
                      DBW_RESAMPLE_FUSED_MAX_KSIZE, A.kx, A.ky);
        return DBW_ERR_UNSUPPORTED;
    }
    const bool fused = form == DBW_RESAMPLE_FUSED || (form == DBW_RESAMPLE_AUTO && fits);
    const long long tiles_x = (Wout + FT_W - 1) / FT_W, tiles_y = (Hout + FT_H - 1) / FT_H;
    int y_first = 0;
    const int n_rows = rows_read(Hin, Hout, &y_first);
    if (fused) {
        DBW_REQUIRE((long long)N * tiles_x * tiles_y < (1LL << 31), "more than 2^31 tiles");
    } else {
        DBW_REQUIRE((long long)N * n_rows * Wout < (1LL << 31) * 256 && (long long)N * Hout * Wout < (1LL << 31) * 256, "more than 2^39 pixels");
        if (Win != Wout) {
            const size_t need = dbw_images_resample_workspace_bytes(N, Hin, Win, Hout, Wout);
            DBW_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "workspace below dbw_images_resample_workspace_bytes");
        }
    }
    if (N == 0) return DBW_OK;
    if (fused) {
        const int kw = (Win != Wout ? A.kx : 1) > (Hin != Hout ? A.ky : 1) ? (Win != Wout ? A.kx : 1) : (Hin != Hout ? A.ky : 1);
        const dim3 grid((unsigned)(N * tiles_x * tiles_y)), block(256);
#define DBW_LAUNCH_FUSED(K) \
    hipLaunchKernelGGL(resample_fused_kernel<K>, grid, block, lds, (hipStream_t)stream, A, src, table_x, table_y, out_f32, out_u8, (int)tiles_x, (int)tiles_y)
        if (kw <= 3) DBW_LAUNCH_FUSED(3);
        else if (kw <= 5) DBW_LAUNCH_FUSED(5);
        else if (kw <= 7) DBW_LAUNCH_FUSED(7);
        else if (kw <= 9) DBW_LAUNCH_FUSED(9);
        else DBW_LAUNCH_FUSED(11);
#undef DBW_LAUNCH_FUSED
        return dbw_check_launch("resample_fused_kernel");
    }
    const uint8_t *in = src;
    int in_first = 0, in_rows = Hin;
    if (Win != Wout) {
        const long long total = (long long)N * n_rows * Wout;
        hipLaunchKernelGGL(resample_h_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A, src, table_x,
                           y_first, n_rows, (uint8_t *)workspace, total);
        const int rc = dbw_check_launch("resample_h_kernel");
        if (rc != DBW_OK) return rc;
        in = (const uint8_t *)workspace; in_first = y_first; in_rows = n_rows;
    }
    const long long total = (long long)N * Hout * Wout;
    hipLaunchKernelGGL(resample_v_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A, in, table_y, in_first,
                       in_rows, out_f32, out_u8, total);
    return dbw_check_launch("resample_v_kernel");
}
