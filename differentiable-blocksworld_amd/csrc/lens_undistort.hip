// Lens rectification (include/dbw_lens.h): raw (N,H,W,3) uint8 frames of a custom capture -> the pinhole frames of the same size, before
// the image ingest resizes them.  The arithmetic is lens_math.h (host + device).
//
// The map is the same for every frame of a scene, and per frame a pixel costs a 12-byte gather and a 3-byte store.  So a lane owns
// LENS_PX = 4 adjacent output pixels of one row and walks frames with the corner offsets and weights of its pixels held in registers:
// the ~40 VALU operations of the map are paid once per lane, not once per frame.  A wave is 64 consecutive quads of ONE row (a block is
// four rows), so neighbouring lanes read neighbouring source pixels and a wave's 768 output bytes are contiguous.  The frames of a chunk
// are dealt over gridDim.z, LENS_FRAMES to a lane: at 540x960 one frame group alone is 2,160 waves, two per SIMD of the part, too few to
// hide the latency of the gather; four groups of four frames keep the map's cost at a quarter per frame and fill the machine.
//
// Stores: a lane's 12 bytes start at the row's address + 12 * quad, which shares its alignment with the whole row.  Where that address is
// h bytes short of a dword boundary, the lane stores the three dwords that START at the boundary -- its own bytes [h, 12) and the first h
// bytes of the next lane, fetched with one cross-lane read -- and the bytes nobody's dwords cover go out one by one: the first h of the
// first lane of a wave, the last 4 - h of the last lane of a wave or of a row, and a ragged last quad (W % 4 != 0) whole.  Any alignment
// of `out` and any W give the same bytes.  No LDS, no scratch.
#include "dbw_common.h"
#include "lens_math.h"
#include "../../include/dbw_lens.h"

namespace {

using namespace dbw;

constexpr int LENS_PX = 4;          // adjacent output pixels of a lane
constexpr int LENS_ROWS = 4;        // rows (waves) of a block
constexpr int LENS_FRAMES = 4;      // frames a lane walks (where the chunk has that many)

struct LensArgs {
    int N, H, W, quads;             // quads = ceil(W / LENS_PX)
    LensParams L;
};

__global__ void __launch_bounds__(64 * LENS_ROWS) lens_undistort_kernel(LensArgs A, const uint8_t *__restrict__ src, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x;                                   // blockDim = (64, LENS_ROWS): a wave is one row's 64 quads
    const int q = blockIdx.x * 64 + lane;
    const int i = blockIdx.y * LENS_ROWS + threadIdx.y;
    if (i >= A.H) return;                                           // (the whole wave)
    const int W = A.W, j0 = q * LENS_PX;
    const int npx = q < A.quads ? (W - j0 < LENS_PX ? W - j0 : LENS_PX) : 0;
    const bool full = npx == LENS_PX;
    // the quad after this one is a full one of the same wave: it takes this lane's dword across the boundary between them
    const bool next_full = lane < 63 && j0 + 2 * LENS_PX <= W;
    const bool prev_covers = lane > 0 && full;                      // ... and so does the one before (which then is full too)
    const int row_bytes = W * 3;

    int off[LENS_PX];
    float wx[LENS_PX], wy[LENS_PX];
#pragma unroll
    for (int p = 0; p < LENS_PX; ++p) {
        const int j = j0 + p < W ? j0 + p : W - 1;                  // (a pixel past the row is never loaded or stored)
        const LensTap t = lens_tap(A.L, i, j, A.H, W);
        off[p] = (t.y0 * W + t.x0) * 3;
        wx[p] = t.wx; wy[p] = t.wy;
    }

    const long long frame_bytes = (long long)A.H * row_bytes;
    const long long row_off = (long long)i * row_bytes + (long long)j0 * 3;
    for (int n = blockIdx.z; n < A.N; n += gridDim.z) {
        const uint8_t *s = src + n * frame_bytes;
        uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int p = 0; p < LENS_PX; ++p) {
            if (p < npx) {
                const uint8_t *c0 = s + off[p], *c1 = c0 + row_bytes;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint32_t v = lens_blend(c0[c], c0[3 + c], c1[c], c1[3 + c], wx[p], wy[p]);
                    const int k = 3 * p + c;
                    w[k >> 2] |= v << (8 * (k & 3));
                }
            }
        }
        const uint32_t next_w0 = (uint32_t)__shfl_down((int)w[0], 1);       // (every lane of the wave is here)
        if (npx == 0) continue;
        uint8_t *o = out + n * frame_bytes + row_off;
        if (!full) {
            for (int k = 0; k < 3 * npx; ++k) o[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
            continue;
        }
        const int h = (int)((0 - (uintptr_t)o) & 3);                        // bytes to the next dword boundary: the same for the whole row
        if (h == 0) {
            uint32_t *d = (uint32_t *)o;
            d[0] = w[0]; d[1] = w[1]; d[2] = w[2];
            continue;
        }
        const int lo = 8 * h, hi = 32 - lo;
        if (!prev_covers)
            for (int k = 0; k < h; ++k) o[k] = (uint8_t)(w[0] >> (8 * k));
        uint32_t *d = (uint32_t *)(o + h);
        d[0] = (w[0] >> lo) | (w[1] << hi);
        d[1] = (w[1] >> lo) | (w[2] << hi);
        if (next_full) {
            d[2] = (w[2] >> lo) | (next_w0 << hi);
        } else {
            for (int k = h; k < 4; ++k) o[8 + k] = (uint8_t)(w[2] >> (8 * k));
        }
    }
}

// The validity map of the rectified frame (dbw_lens_valid_u8): one byte per output pixel, once per scene -- a lane per pixel, rows of
// consecutive bytes per wave.
__global__ void __launch_bounds__(256) lens_valid_kernel(int H, int W, LensParams L, uint8_t *__restrict__ out) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long long)H * W) return;
    out[p] = lens_valid(L, (int)(p / W), (int)(p % W), H, W) ? 255 : 0;
}

bool finite_all(const float *v, int n) {
    for (int k = 0; k < n; ++k)
        if (!(v[k] - v[k] == 0.0f)) return false;
    return true;
}

}  // namespace

extern "C" int dbw_lens_abi_version(void) { return DBW_LENS_ABI_VERSION; }          // (history: include/dbw_lens.h)

extern "C" int dbw_images_undistort_u8(const uint8_t *src, int N, int H, int W, const float *lens, uint8_t *out, dbw_stream_t stream) {
    DBW_REQUIRE(src && lens && out, "null pointer");
    DBW_REQUIRE(N >= 1, "N below 1");
    DBW_REQUIRE(H >= 2 && W >= 2, "a frame below 2 x 2 has no bilinear cell");
    DBW_REQUIRE((long long)H * W < (1LL << 29) && H <= 65535 * LENS_ROWS, "bad size");
    const unsigned long long bytes = (unsigned long long)N * H * W * 3, a = (unsigned long long)(uintptr_t)src, b = (unsigned long long)(uintptr_t)out;
    DBW_REQUIRE(a + bytes <= b || b + bytes <= a, "src and out overlap");
    DBW_REQUIRE(finite_all(lens, LENS_N_PARAMS), "lens: a value that is not finite");
    static_assert(LENS_N_PARAMS == DBW_LENS_N_PARAMS, "lens_math.h and dbw_lens.h disagree");
    LensArgs A;
    A.N = N; A.H = H; A.W = W; A.quads = (W + LENS_PX - 1) / LENS_PX;
    A.L = lens_params(lens);
    const int groups = (N + LENS_FRAMES - 1) / LENS_FRAMES;
    const dim3 grid((unsigned)((A.quads + 63) / 64), (unsigned)((H + LENS_ROWS - 1) / LENS_ROWS), (unsigned)(groups < 65535 ? groups : 65535));
    hipLaunchKernelGGL(lens_undistort_kernel, grid, dim3(64, LENS_ROWS), 0, (hipStream_t)stream, A, src, out);
    return dbw_check_launch("lens_undistort_kernel");
}

extern "C" int dbw_lens_valid_u8(int H, int W, const float *lens, uint8_t *out, dbw_stream_t stream) {
    DBW_REQUIRE(lens && out, "null pointer");
    DBW_REQUIRE(H >= 1 && W >= 1 && (long long)H * W < (1LL << 29), "bad size");
    DBW_REQUIRE(finite_all(lens, LENS_N_PARAMS), "lens: a value that is not finite");
    const long long blocks = ((long long)H * W + 255) / 256;
    hipLaunchKernelGGL(lens_valid_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, H, W, lens_params(lens), out);
    return dbw_check_launch("lens_valid_kernel");
}
