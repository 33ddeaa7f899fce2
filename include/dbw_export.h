/*
 * dbw_export.h -- C ABI of the frame export of libdbw_hip.so: rendered fp32 planes to the interleaved 8-bit frames that image and
 * video files hold, on the device (the reference converts on the host: convert_to_img / save_video, src/utils/image.py:34-53,90-105).
 * Python side: dbw_amd/ops.py (frames_u8), bound through _lib.EXPORT_SIGNATURES.  The arithmetic is csrc/frame_math.h.
 *
 * Conventions are those of dbw_hip.h: DEVICE pointers owned by the caller, contiguous, unless said otherwise; return 0 or a negative
 * DBW_ERR_*, the text in dbw_last_error(); arguments are validated before any launch; kernels are enqueued on `stream`, no host
 * synchronisation.
 */
#ifndef DBW_EXPORT_H
#define DBW_EXPORT_H
#include "dbw_hip.h"

/* ABI revision of this header (dbw_export_abi_version() returns the value the library was built with). */
#define DBW_EXPORT_ABI_VERSION 1

/* flags of dbw_frames_u8 */
#define DBW_FRAME_HWC 1         /* src is (N,H,W,3) fp32 -- the layout of the prepared texture maps -- instead of (N,C,H,W) */
#define DBW_FRAME_EDGE_FIRST 2  /* the edge blend in front of the composite (render_views paints edges on the premultiplied rgb) */
#define DBW_FRAME_CLAMP_INPUT 4 /* clamp the C input channels to [0, 1] first (render_rotated_views clamps before its composite) */

#ifdef __cplusplus
extern "C" {
#endif

int dbw_export_abi_version(void);

/* (N,C,H,W) fp32 planes, C = 3 or 4 (or (N,H,W,3) with DBW_FRAME_HWC, C = 3) -> out (N,H,W,3) uint8.  Per pixel, in this order, one
 * fp32 rounding per operation:
 *   1. composite, when a background is given (C = 4 only): rgb * alpha + (1 - alpha) * bkg, rgb PREMULTIPLIED as the renders are;
 *      bkg3: HOST pointer to 3 floats, or bkg_img: (3,H,W) fp32 shared by the N frames; at most one of the two;
 *   2. edge blend, when mask (N,1,H,W) fp32 is given: img * (1 - mask) + mask * colour; colour is edge3 (HOST pointer to 3 floats) or
 *      edge_img (N,3,H,W) fp32, exactly one of the two;
 *   3. quantise: clamp to [0, 1], times 255.0f, truncate toward zero; NaN -> 0.
 * Without a background the alpha plane of a C = 4 source is not read.  With DBW_FRAME_HWC neither a background nor a mask is taken
 * (DBW_ERR_UNSUPPORTED).  Rows whose W is a multiple of 4 and whose pointers are 16-byte aligned (out: 4-byte) move as 16-byte loads and
 * dword stores; any other shape goes pixel by pixel, same bytes. */
int dbw_frames_u8(const float *src, int N, int C, int H, int W, int flags, const float *bkg3, const float *bkg_img, const float *mask,
                  const float *edge3, const float *edge_img, uint8_t *out, dbw_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
