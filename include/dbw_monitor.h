/*
 * dbw_monitor.h -- C ABI of the run monitor of libdbw_hip.so: what a training run records between two host reads.  Image scores (squared
 * error and SSIM of rendered against held-out views, the reference's mse2psnr / SSIMLoss, src/model/loss.py:28-29,124-156) in one kernel per
 * batch, and a table of running loss sums that the step's device scalars are added to without the host reading them (the reference calls
 * .item() on every loss after every step, src/trainer.py:143).
 * Python side: dbw_amd/ops.py (image_scores) and dbw_amd/runlog.py (DeviceMeter), bound through _lib.MONITOR_SIGNATURES.  The arithmetic is
 * csrc/score_math.h.
 *
 * Conventions are those of dbw_hip.h: DEVICE pointers owned by the caller, contiguous, unless said otherwise; return 0 or a negative
 * DBW_ERR_*, the text in dbw_last_error(); arguments are validated before any launch; kernels are enqueued on `stream`, no host
 * synchronisation.
 */
#ifndef DBW_MONITOR_H
#define DBW_MONITOR_H
#include "dbw_hip.h"

/* ABI revision of this header (dbw_monitor_abi_version() returns the value the library was built with). */
#define DBW_MONITOR_ABI_VERSION 1

#define DBW_METER_MAX_VALUES 16 /* values per dbw_meter_add */
#define DBW_SSIM_WINDOW 11      /* taps of the Gaussian window (sigma 1.5) */

#ifdef __cplusplus
extern "C" {
#endif

int dbw_monitor_abi_version(void);

/* Bytes of `workspace` that dbw_image_scores needs for these sizes (one fp64 pair per workgroup); 0 for sizes it refuses. */
size_t dbw_image_scores_workspace_bytes(int N, int H, int W, int padding);

/* a, b (N,3,H,W) fp32 -> out (N,2) fp64:
 *   out[n][0] = sum over the 3*H*W elements of (a - b)^2, difference and square taken in fp64;
 *   out[n][1] = sum over the 3*H'*W' elements of the SSIM map of image n.
 * SSIM: 11 taps, sigma 1.5, the weights computed in fp64, normalised and rounded to fp32; rows filtered first, then columns, in fp32; the
 * five statistics a, b, a*a, b*b, a*b; C1 = 0.01^2, C2 = 0.03^2.  Each 11-tap filter is a COMPENSATED dot product (Dot2: an fmaf gives every
 * product's rounding error, a two-sum every partial sum's; csrc/score_math.h), i.e. the dot product rounded once -- not the left-to-right
 * separable sum a convolution makes: against dbw_amd.metrics.ssim_map the map differs in the last bits (about 1e-6 per pixel on noise, up
 * to 5e-4 where flat regions cancel in E[x^2] - mu^2), and is the closer of the two to the fp64 definition.  padding = 0 keeps the windows that lie inside
 * the image, H' = H - 10, W' = W - 10 (H < 11 or W < 11: DBW_ERR_INVALID); padding = 1 pads with zeros, H' = H, W' = W.
 * ssim_map, when not NULL: (N,3,H',W') fp32, receives the map.  workspace: dbw_image_scores_workspace_bytes(...) bytes, 8-byte aligned.
 * No atomics: the partial sums of an image are added in index order, two calls on the same inputs give the same bits.  Rows whose W is a
 * multiple of 4 and whose a / b are 16-byte aligned are read as 16-byte loads; any other shape element by element, same results. */
int dbw_image_scores(const float *a, const float *b, int N, int H, int W, int padding, void *workspace, float *ssim_map, double *out,
                     dbw_stream_t stream);

/* SSIM as a loss term (csrc/ssim_term.hip), added under revision 1 of this header.
 * Bytes of `workspace` that dbw_monitor_ssim_term needs for these sizes (one fp64 per workgroup); 0 for sizes it refuses and for N = 0. */
size_t dbw_monitor_ssim_term_workspace_bytes(int N, int H, int W);

/* target, rec (N,3,H,W) fp32 in [0, 1] ->
 *   value[0] = mean over the M = N*3*H*W elements of (1 - SSIM(target, rec)), fp64, on the device;
 *   grad, when not NULL: (N,3,H,W) fp32, d value / d rec.  NULL: the value only, the same bits.
 * SSIM is that of dbw_image_scores with padding = 1 (zero padding, the weights not renormalised: F.conv2d(padding=5)), the same compensated
 * filters in the same order: value[0] is 1 - (the sum of out[n][1] over n) / M up to the last bits of the fp64 additions.  With
 * m = (mu1, mu2, Eaa, Ebb, Eab) the filtered statistics of a window and S = n1 n2 / (d1 d2) its SSIM,
 *   A = dS/dmu2,  B = dS/dEbb = -S / d2,  C = dS/dEab = 2 n1 / (d1 d2)            (maps, zero outside the image)
 *   grad_q = -(1/M) [blur(A)_q + 2 rec_q blur(B)_q + target_q blur(C)_q]
 * with blur the same zero-padded filter (csrc/score_math.h: ssim_deriv, ssim_grad_pixel).  One kernel -- a workgroup per 16 x 32 tile of
 * one channel, the statistics and the three maps held in LDS -- and one that adds the workgroups' fp64 partial values in a fixed order:
 * no atomics, two calls on the same inputs give the same bits.  Rows whose W is a multiple of 4 and whose images are 16-byte aligned are
 * read as 16-byte loads; any other shape element by element, same results.  workspace: dbw_monitor_ssim_term_workspace_bytes(...) bytes,
 * 8-byte aligned, as value is.  N = 0: nothing is launched, value stays as it is.  H * W < 2^31. */
int dbw_monitor_ssim_term(const float *target, const float *rec, int N, int H, int W, void *workspace, float *grad, double *value,
                          dbw_stream_t stream);

/* The two image terms of the loss under a validity mask (csrc/masked_loss.hip), added under revision 1 of this header.
 * masks (N,1,H,W) fp32 weights in [0, 1], 1 = the pixel counts; count = 3 * sum(masks) over the batch is a HOST number.
 *
 * Bytes of `workspace` that the forward of dbw_monitor_masked_composite needs (one fp64 per workgroup); 0 for sizes it refuses, N = 0. */
size_t dbw_monitor_masked_composite_workspace_bytes(int N, int H, int W);

/* fg, env (N,4,H,W), imgs (N,3,H,W), masks (N,1,H,W) fp32; scale = w_rgb / count (0 for count = 0), from the host.
 * rec = fg_rgb * fg_a + (1 - fg_a) * env_rgb, the composite of dbw_composite_mse.
 * Forward (grad_fg == grad_env == NULL): writes rec (N,3,H,W) and value[0] = scale * sum of masks * (rec - imgs)^2 as one fp64 on the
 *   device, through per-workgroup fp64 partials in `workspace` added in a fixed order by a second launch: no atomics, two calls give the
 *   same bits.  upstream and grad_rec must be NULL.
 * Backward (grad_fg, grad_env (N,4,H,W) given; rec, value NULL; workspace unused): ONE launch.  upstream: one fp32 on the device, the
 *   gradient g of the loss with respect to value; grad_rec: (N,3,H,W) or NULL, the gradient with respect to rec that other terms (the
 *   perceptual one) send.  Per pixel and channel d/d rec = (2 scale g) masks (rec - imgs) + grad_rec, taken through the composite:
 *   grad_fg = [d * fg_a (3 channels), sum_c d_c (fg_c - env_c)], grad_env = [d * (1 - fg_a), 0]  (csrc/loss_math.h: masked_composite_pixel).
 * Rows whose W is a multiple of 4 and whose pointers are all 16-byte aligned move as 16-byte loads and stores; any other shape element by
 * element, same results.  value: 8-byte aligned, as workspace is.  N = 0: nothing is launched.  H * W < 2^31. */
int dbw_monitor_masked_composite(const float *fg, const float *env, const float *imgs, const float *masks, int N, int H, int W, double scale,
                                 void *workspace, float *rec, double *value, const float *upstream, const float *grad_rec, float *grad_fg,
                                 float *grad_env, dbw_stream_t stream);

/* Bytes of `workspace` that dbw_monitor_masked_ssim_term needs (one fp64 per workgroup); 0 for sizes it refuses and for N = 0. */
size_t dbw_monitor_masked_ssim_term_workspace_bytes(int N, int H, int W);

/* dbw_monitor_ssim_term under the mask: with a~ = masks * target and b~ = masks * rec,
 *   value[0] = sum over n, c, p of masks_p * (1 - SSIM_p(a~, b~)) / count      (0 for count = 0)
 *   grad, when not NULL: d value / d rec = masks_q * (-1 / count) [blur(masks A)_q + 2 b~_q blur(masks B)_q + a~_q blur(masks C)_q].
 * The invalid region reads as zero, like the outside of the frame, and a window centred in it is not counted: neither value nor gradient
 * depends on what target and rec hold where masks = 0 (finite values), and the gradient is exactly 0 there.  The same kernel structure,
 * filters and order as dbw_monitor_ssim_term; the mask is read from memory, not kept in LDS.  With masks of ones and count = 3 N H W the
 * gradient is dbw_monitor_ssim_term's bit for bit, the value too.  count >= 0 and finite. */
int dbw_monitor_masked_ssim_term(const float *target, const float *rec, const float *masks, int N, int H, int W, double count, void *workspace,
                                 float *grad, double *value, dbw_stream_t stream);

/* The reconstruction term under a per-view exposure (csrc/exposure_loss.hip), added under revision 1 of this header.
 * theta (V,6) fp32: one row (g_r, g_g, g_b, b_r, b_g, b_b) per training view of the scene; ids (N) int32: the batch's rows of theta,
 * distinct.  With comp = fg_rgb * fg_a + (1 - fg_a) * env_rgb, the composite of dbw_composite_mse,
 *   rec_c = exp(g_c) * comp_c + b_c        (no clamp; theta = 0: rec is the composite bit for bit)
 * An id outside [0, V) reads as theta = 0 and its row of grad_theta is skipped: no access outside theta or grad_theta.
 *
 * Bytes of `workspace` that dbw_monitor_exposure_composite needs, forward or backward (six fp64 per workgroup); 0 for sizes it refuses
 * and for N = 0. */
size_t dbw_monitor_exposure_composite_workspace_bytes(int N, int H, int W);

/* fg, env (N,4,H,W), imgs (N,3,H,W) fp32; masks (N,1,H,W) fp32 weights in [0, 1] or NULL = ones; scale = w_rgb / count from the host.
 * Forward (grad_fg == grad_env == grad_theta == NULL): writes rec (N,3,H,W) and value[0] = scale * sum of masks * (rec - imgs)^2 as one
 *   fp64 on the device, through per-workgroup fp64 partials in `workspace` added in index order by a second launch.  upstream and
 *   grad_rec must be NULL.
 * Backward (grad_fg, grad_env (N,4,H,W) and grad_theta (V,6) given; rec, value NULL): one image launch and one finishing launch.
 *   upstream: one fp32 on the device, the gradient g of the loss with respect to value; grad_rec: (N,3,H,W) or NULL, the gradient with
 *   respect to rec that other terms send.  rec is formed again from fg, env and theta; per pixel and channel
 *     d'_c = (2 scale g) masks (rec_c - imgs_c) + grad_rec_c,        d_c = exp(g_c) d'_c,
 *   grad_fg = [d * fg_a (3 channels), sum_c d_c (fg_c - env_c)], grad_env = [d * (1 - fg_a), 0] are WRITTEN, and the six sums of a view
 *     sum_p d'_c exp(g_c) comp_c   (c = r, g, b),      sum_p d'_c   (c = r, g, b)
 *   are ADDED to row ids[n] of grad_theta; the other rows are not touched (csrc/exposure_math.h).  A workgroup belongs to one view; the
 *   sums are reduced in fp64 in the lane, the wave and the workgroup, the workgroups' partials of a view added in a fixed order by one
 *   workgroup of the finishing launch.
 * No floating-point atomics: two calls on the same inputs give the same bytes.  Rows whose W is a multiple of 4 and whose image pointers
 * are all 16-byte aligned move as 16-byte loads and stores; any other shape element by element, same results.  value and workspace:
 * 8-byte aligned.  N = 0: nothing is launched.  N <= 65535, V >= 1, H * W < 2^31. */
int dbw_monitor_exposure_composite(const float *fg, const float *env, const float *imgs, const float *masks, const float *theta,
                                   const int32_t *ids, int N, int H, int W, int V, double scale, void *workspace, float *rec, double *value,
                                   const float *upstream, const float *grad_rec, float *grad_fg, float *grad_env, float *grad_theta,
                                   dbw_stream_t stream);

/* table: n + 2 doubles on the device; vals: HOST array of n <= DBW_METER_MAX_VALUES DEVICE pointers, each to one fp32.  One kernel:
 *   table[i] += (double)*vals[i] * weight  (i < n),   table[n] += weight,
 *   table[n + 1] = step if it is negative and any *vals[i] is not finite (the first such step stays). */
int dbw_meter_add(double *table, const float *const *vals, int n, double weight, int64_t step, dbw_stream_t stream);

/* table[0 .. n] = 0, table[n + 1] = -1. */
int dbw_meter_reset(double *table, int n, dbw_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
