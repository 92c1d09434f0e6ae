/*
 * openglottal_hip_classic.h — the training-free family of the C-ABI (third header; the conventions of openglottal_hip.h --
 * return codes, og_last_error, *_dev entry points, device restore -- all hold): guided-VFT and YOLO+Otsu over frames on the
 * device.  No network is involved, so the family has a handle of its own.
 *
 * References: openglottal/models/tracker.py:117-232 (YOLOGuidedVFT), openglottal/features.py:147-196, scripts/eval_girafe.py:162-171
 * ("yolo+otsu").  The motion map of YOLOGuidedVFT never reaches its output (process_frame updates self.lmap and never reads it), so
 * nothing here depends on cv2.GaussianBlur.  What the mask does depend on, per frame:
 *
 *   box         {x1, y1, x2, y2} int32 as utils.normalize_box leaves it: Python slice semantics already applied (negative
 *               coordinates counted from the far edge, clamped to the frame), x1 < 0 for None.  Empty or inverted: no ROI.
 *   gray        a BGR pixel goes through the 15-bit fixed point of og_bgr2gray_host, per pixel.
 *   histogram   h[256] of the gray bytes inside the box, n = sum h.
 *   percentile  numpy's default (linear) rule on the sorted ROI bytes in f64: v = (n - 1) * (q / 100.0), lo = floor(v), g = v - lo,
 *               a = sorted[lo], b = sorted[min(lo + 1, n - 1)]; a + (b - a) * g if g < 0.5, else b - (b - a) * (1 - g).
 *   recurrence  cur = percentile if n > 10 else thresh;  thresh = beta * thresh + (1 - beta) * cur in f64, two rounded products and
 *               one rounded sum, no FMA.  A frame without a box still runs it (0.7 t + 0.3 t is not always t).  The only thing
 *               sequential in frame order.
 *   raw mask    gray < cut inside the box, cut = ceil(thresh) clamped to 0..256.
 *   blob filter _nblobs (tracker.py:167-179) restated without cv2.  Candidates: the 8-connected components of the HOLE-FILLED raw
 *               mask (a hole: a 4-connected background component that does not touch the frame border; an island inside a hole
 *               belongs to the blob around it).  Key: twice the contour area = over all 2x2 windows of the frame padded by one
 *               background ring, 2 * #(windows with 4 filled pixels of the blob) + #(windows with exactly 3).  The n blobs with
 *               the greatest keys are kept; among equal keys the blob whose raster-first pixel comes LATER wins (UNPINNED:
 *               findContours' order from recall; one function, og_blob_rank in csrc/og_kernels.hpp).  Output: their filled pixels
 *               at 255; area = their count.
 *   Otsu        OpenCV's getThreshVal_Otsu_8u on the ROI histogram, f64 (UNPINNED as every cv2 row): scale = 1/n, mu = scale * sum
 *               i h[i]; for i = 0..255: p = h[i] * scale, mu1 *= q1, q1 += p, q2 = 1 - q1; skip i when min(q1, q2) < FLT_EPSILON or
 *               max(q1, q2) > 1 - FLT_EPSILON; else mu1 = (mu1 + i p) / q1, mu2 = (mu - q1 mu1) / q2, sigma = q1 q2 (mu1 - mu2)^2;
 *               the first i with strictly greater sigma; 0 when none qualifies.  Mask: 255 where gray <= T inside the box.
 *
 * Each rule is one inline function of csrc/og_kernels.hpp that the kernels and the *_host entries below both call.
 *
 * LIMITS (og_classic_limit): H * W <= 65 536 pixels (256 x 256, the largest frame the blob filter's kernel has been measured on: it
 * labels a frame with ONE workgroup); n_components 1..8; chunk 1..1024.
 * MEMORY: frames are processed in micro-batches of  nb = min(chunk, 64 MiB / (H * W * channels)), at least 1, frames.  The handle's
 * device workspace is that of ONE micro-batch -- nb * (H * W * (channels + 1 + 8) + 1060) + 8 bytes: source frames and mask (host
 * entries only), two int32 label arrays, histogram, boxes, thresh, cut, T, area -- plus two pinned host slots of
 * nb * (H * W * (channels + 1) + 32) bytes: independent of B.  A handle used with several frame sizes keeps, per buffer, the bytes
 * of the largest micro-batch it has run (never the product of the largest nb and the largest frame).  og_classic_plan reports the
 * device figure of one call.
 *
 * ALIGNMENT: int32 / uint32 buffers (boxes, box4, area, T, hist256) 4 bytes, double buffers (thresh) and the frame_ptrs array 8,
 * u8 buffers any address.  A violation is OG_EINVAL before anything is launched, copied or written.
 */
#ifndef OPENGLOTTAL_HIP_CLASSIC_H
#define OPENGLOTTAL_HIP_CLASSIC_H

#include "openglottal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct og_classic og_classic;

/* Host only, no handle, no device: the rules above by the very inline functions the kernels call ---------------------- */

/* which: 0 max H * W, 1 max n_components, 2 max chunk, 3 bytes of source frames per micro-batch (64 MiB) */
long long og_classic_limit(int which);

/* np.percentile(px, q) of the bytes a histogram stands for.  OG_EINVAL: an empty histogram, q outside 0..100. */
int og_percentile_host(const uint32_t* hist256, double q, double* out);

/* T of cv2.threshold(roi, 0, 255, THRESH_BINARY_INV | THRESH_OTSU).  OG_EINVAL: an empty histogram. */
int og_otsu_threshold_host(const uint32_t* hist256, int32_t* T);

/* hist256 of gray(frame [H,W,channels] u8) inside box4; all zero for no ROI. */
int og_box_hist_host(const uint8_t* frame, int H, int W, int channels, const int32_t* box4, uint32_t* hist256);

/* One frame of the recurrence: *thresh_out = beta * thresh + (1 - beta) * (percentile(hist256, q) if n > 10 else thresh),
 * *cut_out = ceil(*thresh_out) clamped to 0..256. */
int og_vft_step_host(double thresh, double beta, const uint32_t* hist256, double q, double* thresh_out, int32_t* cut_out);

/* _nblobs(mask, n): mask [H,W] u8 (nonzero = set) -> out_mask_or_null [H,W] u8 {0,255} (every byte written) and *area.  A
 * sequential union-find that shares the key and the order with the kernel. */
int og_blobs_host(const uint8_t* mask, int H, int W, int n_components, uint8_t* out_mask_or_null, int32_t* area);

/* The handle ------------------------------------------------------------------------------------------------------------ */

/* The device is the one current at the first call that touches it (og_init); the handle owns its stream and workspace.
 * A new handle has beta 0.7, percentile 30, n_components 2 (YGVFT_PARAMS), chunk 128, and no threshold yet. */
og_classic* og_classic_create(void);
void og_classic_destroy(og_classic* h);
int og_classic_sync(og_classic* h);
int og_classic_set_chunk(og_classic* h, int chunk);

/* New parameters; the running threshold is dropped (og_vft_guided_init_u8 or og_vft_guided_set_state must follow). */
int og_vft_guided_reset(og_classic* h, double beta, double percentile, int n_components);

/* YOLOGuidedVFT.initialize (tracker.py:183-203): frames [n,H,W,channels] u8 on the host, n >= 1; the threshold is seeded from
 * the LAST frame inside box4_or_null, over the whole frame when it is NULL, None or gives no ROI.  *thresh_out (may be NULL). */
int og_vft_guided_init_u8(og_classic* h, const uint8_t* frames, int n, int H, int W, int channels, const int32_t* box4_or_null,
                          double* thresh_out);

/* The running threshold, read (waits for the handle's stream) and written. */
int og_vft_guided_get_state(og_classic* h, double* thresh);
int og_vft_guided_set_state(og_classic* h, double thresh);

/* process_frame (tracker.py:205-232) over B frames on the HOST, in order, continuing from the running threshold: frames
 * [B,H,W,channels] u8, boxes [B,4] int32; mask_or_null [B,H,W] u8 {0,255}; area [B] int32; thresh_or_null [B] f64, the threshold
 * AFTER each frame's update (the one its mask was cut with).  Uploaded through two pinned slots, micro-batch by micro-batch.
 * Synchronous.  OG_ESTATE without a threshold.  On an error everything in flight is waited for and the handle stays usable; the
 * running threshold is then that of the last micro-batch that ran. */
int og_vft_guided_stream_u8(og_classic* h, const uint8_t* frames, int B, int H, int W, int channels, const int32_t* boxes,
                            uint8_t* mask_or_null, int32_t* area, double* thresh_or_null);

/* The same for a list of separately allocated frames, each of H * W * channels bytes. */
int og_vft_guided_stream_frames_u8(og_classic* h, const uint8_t* const* frame_ptrs, int B, int H, int W, int channels,
                                   const int32_t* boxes, uint8_t* mask_or_null, int32_t* area, double* thresh_or_null);

/* The same with frames, boxes and outputs resident on the device; asynchronous on the handle's stream. */
int og_vft_guided_u8_dev(og_classic* h, const uint8_t* frames_dev, int B, int H, int W, int channels, const int32_t* boxes_dev,
                         uint8_t* mask_dev_or_null, int32_t* area_dev, double* thresh_dev_or_null);

/* "yolo+otsu" (eval_girafe.py:162-171) over B frames: mask_or_null [B,H,W] u8 {0,255}, area [B] int32, T [B] int32 (0 for a frame
 * without a ROI, whose mask is all zero).  Independent per frame; needs no threshold state.  Host frames, synchronous. */
int og_otsu_in_box_u8(og_classic* h, const uint8_t* frames, int B, int H, int W, int channels, const int32_t* boxes,
                      uint8_t* mask_or_null, int32_t* area, int32_t* T);

/* Resident, asynchronous on the handle's stream. */
int og_otsu_in_box_u8_dev(og_classic* h, const uint8_t* frames_dev, int B, int H, int W, int channels, const int32_t* boxes_dev,
                          uint8_t* mask_dev_or_null, int32_t* area_dev, int32_t* T_dev);

/* Dry run of og_vft_guided_stream_u8 (mask asked for) without a device, as og_unet_plan_crops: one line per launch,
 * kernel|gx|gy|gz|block|lds|workspace|counters|writes (lds: DYNAMIC LDS, 0 here -- the kernels' static arrays, 1 KiB in k_box_hist
 * and under 256 bytes in k_blobs, are not in it; "mask=END;area=END": bytes from the start of the micro-batch's output
 * buffers to the end of the launch's writes, or "-").  Returns the number of launches; *workspace_bytes = the device workspace. */
int og_classic_plan(int B, int H, int W, int channels, int chunk, char* out, size_t cap, long long* workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
