/*
 * dbw_lens.h -- C ABI of the lens rectification of libdbw_hip.so: raw 8-bit frames of a custom capture, resident on the device, resampled
 * from the distorted image of an OpenCV radial-tangential lens (the k1..k4, p1, p2 of a Nerfstudio transforms.json) into the pinhole frame
 * the renderer assumes, before the image ingest (dbw_ingest.h) resizes them.
 * Python side: dbw_amd/ops.py (undistort_u8), bound through _lib.LENS_SIGNATURES.  The arithmetic is csrc/lens_math.h.
 *
 * Conventions are those of dbw_hip.h: DEVICE pointers owned by the caller, contiguous, unless said otherwise; return 0 or a negative
 * DBW_ERR_*, the text in dbw_last_error(); arguments are validated before any launch; kernels are enqueued on `stream`, no host
 * synchronisation.
 */
#ifndef DBW_LENS_H
#define DBW_LENS_H
#include "dbw_hip.h"

/* ABI revision of this header (dbw_lens_abi_version() returns the value the library was built with). */
#define DBW_LENS_ABI_VERSION 1

/* Number of floats of the `lens` array. */
#define DBW_LENS_N_PARAMS 12

#ifdef __cplusplus
extern "C" {
#endif

int dbw_lens_abi_version(void);

/* src (N,H,W,3) uint8 -> out (N,H,W,3) uint8, both on the DEVICE; they must not overlap (DBW_ERR_INVALID).  N >= 1, H >= 2, W >= 2.
 * lens: a HOST array of DBW_LENS_N_PARAMS floats [fx, fy, cx, cy, inv_zfx, inv_zfy, k1, k2, k3, k4, p1, p2], read before the call
 * returns: focal lengths and principal point of the source frames in pixels (pixel centres at +0.5), the reciprocals 1 / (zoom * fx) and
 * 1 / (zoom * fy) of the output's focal lengths, and the distortion coefficients.  Output pixel (i, j) is the bilinear sample of its
 * frame at
 *   x = (j + 0.5 - cx) * inv_zfx, y = (i + 0.5 - cy) * inv_zfy, r2 = x*x + y*y, d = 1 + r2*(k1 + r2*(k2 + r2*(k3 + r2*k4))),
 *   u = (x*d + 2*p1*x*y + p2*(r2 + 2*x*x)) * fx + cx - 0.5,  v = (y*d + 2*p2*x*y + p1*(r2 + 2*y*y)) * fy + cy - 0.5,
 * clamped to the frame, in fp32 and rounded half up (csrc/lens_math.h has the order of the operations).  The same map serves all N
 * frames.  Output rows leave as dwords where their addresses allow it and byte by byte at their ends: any alignment of src and out and
 * any W give the same bytes. */
int dbw_images_undistort_u8(const uint8_t *src, int N, int H, int W, const float *lens, uint8_t *out, dbw_stream_t stream);

/* The validity map of a rectified frame, added under revision 1 of this header.  out (H,W) uint8 on the DEVICE: 255 where output pixel
 * (i, j) reads inside the source frame -- 0 <= u <= W - 1 and 0 <= v <= H - 1 for the (u, v) above, NOT clamped --, 0 elsewhere and for
 * a NaN coordinate.  lens: the HOST array of dbw_images_undistort_u8.  One map serves every frame of a scene: with it as a mask of the
 * loss the frames need no zoom that crops the border away.  H >= 1, W >= 1. */
int dbw_lens_valid_u8(int H, int W, const float *lens, uint8_t *out, dbw_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
