// Rectification of frames with a camera each (include/dbw_lens.h: dbw_lens_rectify_u8, dbw_lens_rectify_valid_u8): raw (N,H,W,3) uint8
// frames, every one taken through its own lens -- radial-tangential or fisheye, its own focal lengths and principal point --, resampled
// into the ONE pinhole camera the scene is trained with.  The arithmetic is lens_math.h (host + device).
//
// The map differs from frame to frame, so nothing of it can be kept in registers across frames as lens_undistort.hip does: it is computed
// per frame and pixel, ~45 VALU operations for model 0 and ~70 with two divisions and a square root for the fisheye, next to the 12-byte
// gather and the 3-byte store of that pixel.  The frame is blockIdx.z: the model branch is uniform over a block, and the frame's row of
// the camera table is a uniform (scalar) load from the kernel-argument block.  The table travels BY VALUE: a row is 64 bytes, a launch
// takes LENS_RECT_GROUP = 32 frames (2 KiB of the 4 KiB a launch may carry), and the entry point loops over such groups.  No upload, no
// allocation, no synchronisation, and the host arrays are free again when the call returns.
//
// The output side is that of lens_undistort.hip: a lane owns LENS_PX = 4 adjacent pixels of a row, a wave 64 consecutive quads of ONE row,
// a block four rows.  A lane's 12 bytes leave as the three dwords that start at the next dword boundary, with the first bytes of the next
// lane fetched by one cross-lane read, and the bytes no dword covers go out one by one (the head of a wave's first lane, the tail of its
// last, a ragged last quad whole).  Any alignment of `out` and any W give the same bytes.  No LDS, no scratch.
#include "dbw_common.h"
#include "lens_math.h"
#include "../../include/dbw_lens.h"

namespace {

using namespace dbw;

constexpr int LENS_PX = 4;              // adjacent output pixels of a lane
constexpr int LENS_ROWS = 4;            // rows (waves) of a block
constexpr int LENS_RECT_GROUP = 32;     // frames of one launch: their rows of the table fill half of the kernel-argument block

struct RectArgs {
    int n, H, W, quads;                 // n: frames of this launch (<= LENS_RECT_GROUP), quads = ceil(W / LENS_PX)
    float target[4];
    float cams[LENS_RECT_GROUP][LENS_RECT_N_PARAMS];
};

__global__ void __launch_bounds__(64 * LENS_ROWS) lens_rectify_kernel(RectArgs A, const uint8_t *__restrict__ src, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x;                                   // blockDim = (64, LENS_ROWS): a wave is one row's 64 quads
    const int q = blockIdx.x * 64 + lane;
    const int i = blockIdx.y * LENS_ROWS + threadIdx.y;
    const int n = blockIdx.z;                                       // (gridDim.z == A.n)
    if (i >= A.H) return;                                           // (the whole wave)
    const int W = A.W, j0 = q * LENS_PX;
    const int npx = q < A.quads ? (W - j0 < LENS_PX ? W - j0 : LENS_PX) : 0;
    const bool full = npx == LENS_PX;
    // the quad after this one is a full one of the same wave: it takes this lane's dword across the boundary between them
    const bool next_full = lane < 63 && j0 + 2 * LENS_PX <= W;
    const bool prev_covers = lane > 0 && full;                      // ... and so does the one before (which then is full too)
    const int row_bytes = W * 3;
    const LensCam C = lens_cam(A.cams[n]);
    const LensTarget T = lens_target(A.target);

    const long long frame_bytes = (long long)A.H * row_bytes;
    const uint8_t *s = src + n * frame_bytes;
    uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int p = 0; p < LENS_PX; ++p) {
        if (p < npx) {
            const LensTap t = lens_rect_tap(C, T, i, j0 + p, A.H, W);
            const uint8_t *c0 = s + (t.y0 * W + t.x0) * 3, *c1 = c0 + row_bytes;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t v = lens_blend(c0[c], c0[3 + c], c1[c], c1[3 + c], t.wx, t.wy);
                const int k = 3 * p + c;
                w[k >> 2] |= v << (8 * (k & 3));
            }
        }
    }
    const uint32_t next_w0 = (uint32_t)__shfl_down((int)w[0], 1);           // (every lane of the wave is here)
    if (npx == 0) return;
    uint8_t *o = out + n * frame_bytes + (long long)i * row_bytes + (long long)j0 * 3;
    if (!full) {
        for (int k = 0; k < 3 * npx; ++k) o[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        return;
    }
    const int h = (int)((0 - (uintptr_t)o) & 3);                            // bytes to the next dword boundary: the same for the whole row
    if (h == 0) {
        uint32_t *d = (uint32_t *)o;
        d[0] = w[0]; d[1] = w[1]; d[2] = w[2];
        return;
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

// The validity maps of the rectified frames (dbw_lens_rectify_valid_u8): one byte per frame and output pixel, once per scene -- a lane per
// pixel, consecutive bytes per wave, the frame in blockIdx.z.
__global__ void __launch_bounds__(256) lens_rectify_valid_kernel(RectArgs A, uint8_t *__restrict__ out) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x, px = (long long)A.H * A.W;
    if (p >= px) return;
    const int n = blockIdx.z;
    out[n * px + p] = lens_rect_valid(lens_cam(A.cams[n]), lens_target(A.target), (int)(p / A.W), (int)(p % A.W), A.H, A.W) ? 255 : 0;
}

// The table and the target of a call, validated (0 or a negative DBW_ERR_*).
int check_cameras(int N, const float *cams, const float *target) {
    for (int k = 0; k < 4; ++k) DBW_REQUIRE(target[k] - target[k] == 0.0f, "target: a value that is not finite");
    DBW_REQUIRE(target[2] > 0.0f && target[3] > 0.0f, "target: a reciprocal focal length that is not positive");
    for (long long n = 0; n < N; ++n) {
        const float *row = cams + n * LENS_RECT_N_PARAMS;
        for (int k = 0; k < LENS_RECT_N_PARAMS; ++k) DBW_REQUIRE(row[k] - row[k] == 0.0f, "cams: a value that is not finite");
        DBW_REQUIRE(row[0] == (float)LENS_RECT_PINHOLE || row[0] == (float)LENS_RECT_FISHEYE, "cams: a model id that is neither 0 nor 1");
        DBW_REQUIRE(row[1] > 0.0f && row[2] > 0.0f, "cams: a focal length that is not positive");
    }
    return 0;
}

// The arguments of the launch of the frames [n0, n0 + n) of a call.
void fill_group(RectArgs *A, int n0, int n, int H, int W, const float *cams, const float *target) {
    A->n = n; A->H = H; A->W = W; A->quads = (W + LENS_PX - 1) / LENS_PX;
    for (int k = 0; k < 4; ++k) A->target[k] = target[k];
    for (int f = 0; f < LENS_RECT_GROUP; ++f)
        for (int k = 0; k < LENS_RECT_N_PARAMS; ++k)
            A->cams[f][k] = f < n ? cams[(long long)(n0 + f) * LENS_RECT_N_PARAMS + k] : 0.0f;
}

}  // namespace

extern "C" int dbw_lens_rectify_u8(const uint8_t *src, int N, int H, int W, const float *cams, const float *target, uint8_t *out,
                                   dbw_stream_t stream) {
    DBW_REQUIRE(src && cams && target && out, "null pointer");
    DBW_REQUIRE(N >= 1, "N below 1");
    DBW_REQUIRE(H >= 2 && W >= 2, "a frame below 2 x 2 has no bilinear cell");
    DBW_REQUIRE((long long)H * W < (1LL << 29) && H <= 65535 * LENS_ROWS, "bad size");
    const unsigned long long bytes = (unsigned long long)N * H * W * 3, a = (unsigned long long)(uintptr_t)src, b = (unsigned long long)(uintptr_t)out;
    DBW_REQUIRE(a + bytes <= b || b + bytes <= a, "src and out overlap");
    static_assert(LENS_RECT_N_PARAMS == DBW_LENS_RECT_N_PARAMS, "lens_math.h and dbw_lens.h disagree");
    static_assert(sizeof(RectArgs) + 2 * sizeof(void *) <= 4096, "the arguments of a launch do not fit its argument block");
    if (const int rc = check_cameras(N, cams, target)) return rc;
    const long long frame_bytes = (long long)H * W * 3;
    RectArgs A;
    for (int n0 = 0; n0 < N; n0 += LENS_RECT_GROUP) {
        const int n = N - n0 < LENS_RECT_GROUP ? N - n0 : LENS_RECT_GROUP;
        fill_group(&A, n0, n, H, W, cams, target);
        const dim3 grid((unsigned)((A.quads + 63) / 64), (unsigned)((H + LENS_ROWS - 1) / LENS_ROWS), (unsigned)n);
        hipLaunchKernelGGL(lens_rectify_kernel, grid, dim3(64, LENS_ROWS), 0, (hipStream_t)stream, A, src + n0 * frame_bytes, out + n0 * frame_bytes);
        if (const int rc = dbw_check_launch("lens_rectify_kernel")) return rc;
    }
    return 0;
}

extern "C" int dbw_lens_rectify_valid_u8(int N, int H, int W, const float *cams, const float *target, uint8_t *out, dbw_stream_t stream) {
    DBW_REQUIRE(cams && target && out, "null pointer");
    DBW_REQUIRE(N >= 1, "N below 1");
    DBW_REQUIRE(H >= 1 && W >= 1 && (long long)H * W < (1LL << 29), "bad size");
    if (const int rc = check_cameras(N, cams, target)) return rc;
    const long long px = (long long)H * W;
    RectArgs A;
    for (int n0 = 0; n0 < N; n0 += LENS_RECT_GROUP) {
        const int n = N - n0 < LENS_RECT_GROUP ? N - n0 : LENS_RECT_GROUP;
        fill_group(&A, n0, n, H, W, cams, target);
        hipLaunchKernelGGL(lens_rectify_valid_kernel, dim3((unsigned)((px + 255) / 256), 1, (unsigned)n), dim3(256), 0, (hipStream_t)stream, A,
                           out + n0 * px);
        if (const int rc = dbw_check_launch("lens_rectify_valid_kernel")) return rc;
    }
    return 0;
}
