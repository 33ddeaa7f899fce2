/*
 * dbw_ingest.h -- C ABI of the image ingest of libdbw_hip.so: raw 8-bit frames, resident on the device, to the training targets the
 * reference's datasets make on the host with Compose([Resize(img_size), ToTensor()]) on a PIL image (src/dataset/dtu.py:70-72,
 * bmvs.py:61-63): Pillow's antialiased BILINEAR resample in 8-bit fixed point, then uint8 / 255 in fp32 -- the same bytes and floats.
 * Python side: dbw_amd/ops.py (resample_u8), bound through _lib.INGEST_SIGNATURES.  The arithmetic is csrc/resample_math.h.
 *
 * Conventions are those of dbw_hip.h: DEVICE pointers owned by the caller, contiguous, unless said otherwise; return 0 or a negative
 * DBW_ERR_*, the text in dbw_last_error(); arguments are validated before any launch; kernels are enqueued on `stream`, no host
 * synchronisation.
 */
#ifndef DBW_INGEST_H
#define DBW_INGEST_H
#include "dbw_hip.h"

/* ABI revision of this header (dbw_ingest_abi_version() returns the value the library was built with). */
#define DBW_INGEST_ABI_VERSION 1

/* `form` of dbw_images_resample_u8: which of the two kernel forms runs.  They give the same bytes. */
#define DBW_RESAMPLE_AUTO 0    /* the fused form where both tables are at most DBW_RESAMPLE_FUSED_MAX_KSIZE wide, the general form otherwise */
#define DBW_RESAMPLE_GENERAL 1 /* two launches through an 8-bit intermediate in the workspace: any ratio */
#define DBW_RESAMPLE_FUSED 2   /* one launch, the intermediate in LDS; DBW_ERR_UNSUPPORTED where a table is wider than the bound */

/* Widest table (weights per row) the fused form takes on either axis: ratios up to 5, which covers DTU (4), BlendedMVS (2), the identity
 * and every up-scaling.  At this bound an 8 x 64 output tile reads at most 9 * 5 + 1 = 46 source rows of at most 65 * 5 + 1 = 326 pixels:
 * 46 rows of 988 bytes of LDS for the source and 3 * 46 * 68 bytes for the intermediate, 54 KiB, under the 64 KiB a workgroup may take
 * (300x400 -> 60x80 takes 53,280 bytes; DTU's 1200x1600 -> 300x400 takes 35,712). */
#define DBW_RESAMPLE_FUSED_MAX_KSIZE 11

#ifdef __cplusplus
extern "C" {
#endif

int dbw_ingest_abi_version(void);

/* HOST function, HOST pointers: the coefficient table of one axis, in_size input samples to out_size output samples.  Returns the
 * number of weights per row, ksize = 2 * ceil(max(in_size / out_size, 1)) + 1 (> 0), and fills out_size rows of
 * [xmin, n, k_0 .. k_{ksize-1}] int32, zero padded: output sample i is clamp((2^21 + sum_{x<n} pixel[xmin + x] * k_x) >> 22, 0, 255).
 * With table == NULL it only returns ksize.  DBW_ERR_INVALID on a size below 1 or when capacity_ints < out_size * (ksize + 2). */
int dbw_resample_table(int in_size, int out_size, int32_t *table, size_t capacity_ints);

/* Bytes of workspace dbw_images_resample_u8 needs for these sizes in its general form (the fused form needs none; 0 on bad sizes). */
size_t dbw_images_resample_workspace_bytes(int N, int Hin, int Win, int Hout, int Wout);

/* src (N,Hin,Win,3) uint8 -> out_f32 (N,3,Hout,Wout) fp32 in [0, 1], the ToTensor layout, and / or out_u8 (N,Hout,Wout,3) uint8; at least
 * one of the two.  table_x: Wout rows of dbw_resample_table(Win, Wout), table_y: Hout rows of dbw_resample_table(Hin, Hout), both on the
 * DEVICE; the table of an axis that keeps its size may be NULL (that pass is skipped; it is the identity).  The horizontal pass runs
 * first and rounds to 8 bits, as Pillow does.  workspace: workspace_bytes >= dbw_images_resample_workspace_bytes(...), may be NULL where
 * that is 0 or the fused form runs.  Source rows move as dwords where their addresses allow it and byte by byte at their ends: any
 * alignment of src gives the same bytes. */
int dbw_images_resample_u8(const uint8_t *src, int N, int Hin, int Win, int Hout, int Wout, const int32_t *table_x, const int32_t *table_y,
                           float *out_f32, uint8_t *out_u8, void *workspace, size_t workspace_bytes, int form, dbw_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
