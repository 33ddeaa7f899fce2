// 8-bit frame export (include/dbw_export.h): fp32 planes -> interleaved uint8 frames, with the optional background composite and edge
// blend in front of the quantisation.  The arithmetic is frame_math.h (host + device).
//
// A pure streaming pass: one thread takes 4 consecutive pixels of a row -- one 16-byte load per plane it needs, three dword stores --, no
// LDS, no scratch.  Rows that cannot be addressed that way (W not a multiple of 4, or a pointer off its alignment) go pixel by pixel
// through the same per-pixel function: same bytes.
#include "dbw_common.h"
#include "frame_math.h"
#include "../../include/dbw_export.h"

namespace {

using namespace dbw;

struct FrameArgs {
    const float *src, *bkg_img, *mask, *edge_img;
    uint8_t *out;
    float bkg3[3], edge3[3];
    int N, C, H, W, flags, has_bkg;
};

template <bool VEC>
__global__ void __launch_bounds__(256) frames_u8_kernel(FrameArgs A, long long groups) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    const int Wg = (A.W + 3) >> 2;
    const int x0 = (int)(g % Wg) << 2;
    const long long row = g / Wg;                        // n * H + y
    const int y = (int)(row % A.H);
    const long long n = row / A.H, P = (long long)A.H * A.W, in_row = (long long)y * A.W + x0;
    const bool hwc = A.flags & FRAME_HWC, has_bkg = A.has_bkg, has_mask = A.mask != nullptr;
    float px[4][4], bk[4][3], mk[4], ec[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        px[i][3] = 1.f; mk[i] = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) { bk[i][c] = A.bkg3[c]; ec[i][c] = A.edge3[c]; }
    }
    if constexpr (VEC) {
        if (hwc) {
            const float4 *p = (const float4 *)(A.src + (row * A.W + x0) * 3);
            const float4 a = p[0], b = p[1], c = p[2];
            const float v[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) px[i][ch] = v[i * 3 + ch];
        } else {
            const float *base = A.src + n * A.C * P + in_row;
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                if (ch == 3 && !(A.C == 4 && (has_bkg || (A.flags & FRAME_CLAMP_INPUT)))) break;
                const float4 v = *(const float4 *)(base + ch * P);
                px[0][ch] = v.x; px[1][ch] = v.y; px[2][ch] = v.z; px[3][ch] = v.w;
            }
        }
        if (A.bkg_img) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float4 v = *(const float4 *)(A.bkg_img + ch * P + in_row);
                bk[0][ch] = v.x; bk[1][ch] = v.y; bk[2][ch] = v.z; bk[3][ch] = v.w;
            }
        }
        if (has_mask) {
            const float4 m = *(const float4 *)(A.mask + n * P + in_row);
            mk[0] = m.x; mk[1] = m.y; mk[2] = m.z; mk[3] = m.w;
            if (A.edge_img) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float4 v = *(const float4 *)(A.edge_img + (n * 3 + ch) * P + in_row);
                    ec[0][ch] = v.x; ec[1][ch] = v.y; ec[2][ch] = v.z; ec[3][ch] = v.w;
                }
            }
        }
        uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint8_t o[3];
            frame_pixel(px[i], has_bkg, bk[i], has_mask, mk[i], ec[i], A.flags, o);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int byte = i * 3 + ch;
                w[byte >> 2] |= (uint32_t)o[ch] << ((byte & 3) * 8);
            }
        }
        uint32_t *dst = (uint32_t *)(A.out + (row * A.W + x0) * 3);
        dst[0] = w[0]; dst[1] = w[1]; dst[2] = w[2];
    } else {
        for (int i = 0; i < 4 && x0 + i < A.W; ++i) {
            const long long q = in_row + i;
            float p[4] = {0.f, 0.f, 0.f, 1.f}, b[3] = {A.bkg3[0], A.bkg3[1], A.bkg3[2]}, e[3] = {A.edge3[0], A.edge3[1], A.edge3[2]}, m = 0.f;
            if (hwc) {
                const float *s = A.src + (row * A.W + x0 + i) * 3;
                p[0] = s[0]; p[1] = s[1]; p[2] = s[2];
            } else {
                const float *s = A.src + n * A.C * P + q;
                p[0] = s[0]; p[1] = s[P]; p[2] = s[2 * P];
                if (A.C == 4) p[3] = s[3 * P];
            }
            if (A.bkg_img) { b[0] = A.bkg_img[q]; b[1] = A.bkg_img[P + q]; b[2] = A.bkg_img[2 * P + q]; }
            if (has_mask) {
                m = A.mask[n * P + q];
                if (A.edge_img) { const float *s = A.edge_img + n * 3 * P + q; e[0] = s[0]; e[1] = s[P]; e[2] = s[2 * P]; }
            }
            uint8_t o[3];
            frame_pixel(p, has_bkg, b, has_mask, m, e, A.flags, o);
            uint8_t *dst = A.out + (row * A.W + x0 + i) * 3;
            dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
        }
    }
}

}  // namespace

extern "C" int dbw_export_abi_version(void) { return DBW_EXPORT_ABI_VERSION; }      // (history: include/dbw_export.h)

extern "C" int dbw_frames_u8(const float *src, int N, int C, int H, int W, int flags, const float *bkg3, const float *bkg_img, const float *mask,
                             const float *edge3, const float *edge_img, uint8_t *out, dbw_stream_t stream) {
    DBW_REQUIRE(src && out, "null pointer");
    DBW_REQUIRE(N >= 0 && H > 0 && W > 0 && (long long)H * W < (1LL << 31), "bad size");
    DBW_REQUIRE(C == 3 || C == 4, "C must be 3 or 4");
    DBW_REQUIRE((flags & ~(DBW_FRAME_HWC | DBW_FRAME_EDGE_FIRST | DBW_FRAME_CLAMP_INPUT)) == 0, "unknown flag");
    DBW_REQUIRE(!(bkg3 && bkg_img), "bkg3 and bkg_img are exclusive");
    DBW_REQUIRE(!(bkg3 || bkg_img) || C == 4, "a background composite needs an alpha plane: C must be 4");
    DBW_REQUIRE(mask ? ((edge3 != nullptr) != (edge_img != nullptr)) : (!edge3 && !edge_img), "a mask takes exactly one of edge3 / edge_img, and they take a mask");
    if ((flags & DBW_FRAME_HWC) && (C != 3 || bkg3 || bkg_img || mask)) {
        dbw_set_error("dbw_frames_u8: the (N,H,W,3) layout takes C = 3, no background and no mask");
        return DBW_ERR_UNSUPPORTED;
    }
    const long long groups = (long long)N * H * ((W + 3) / 4);
    DBW_REQUIRE(groups < (1LL << 31) * 256, "more than 2^39 pixel groups");
    if (N == 0) return DBW_OK;
    FrameArgs A;
    A.src = src; A.bkg_img = bkg_img; A.mask = mask; A.edge_img = edge_img; A.out = out;
    for (int i = 0; i < 3; ++i) { A.bkg3[i] = bkg3 ? bkg3[i] : 0.f; A.edge3[i] = edge3 ? edge3[i] : 0.f; }
    A.N = N; A.C = C; A.H = H; A.W = W; A.flags = flags; A.has_bkg = bkg3 || bkg_img;
    const bool vec = W % 4 == 0 && aligned16(src) && aligned16(bkg_img) && aligned16(mask) && aligned16(edge_img) && ((uintptr_t)out & 3) == 0;
    const dim3 grid((unsigned)((groups + 255) / 256)), block(256);
    if (vec) hipLaunchKernelGGL(frames_u8_kernel<true>, grid, block, 0, (hipStream_t)stream, A, groups);
    else hipLaunchKernelGGL(frames_u8_kernel<false>, grid, block, 0, (hipStream_t)stream, A, groups);
    return dbw_check_launch("frames_u8_kernel");
}
