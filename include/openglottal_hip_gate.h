/*
 * openglottal_hip_gate.h — the gated pipeline with the U-Net run ONLY on the frames the tracker kept (eighth header; the
 * conventions of openglottal_hip.h -- return codes, og_last_error, *_dev entry points, device restore -- all hold).  The reference's
 * clinical scripts segment a frame only if detector.detect returned a box (scripts/analyze_gaw.py:86-95, scripts/infer.py:250-263);
 * og_gated_stream_u8 (fourth header) follows features.py:236 instead, segments every frame and zeroes the area afterwards.  The
 * entries below skip that work exactly: a frame's mask and area are a function of the frame alone, so the areas are the same bits.
 *
 * THE RULE: frame i is KEPT iff boxes[i][0] >= 0 -- the tracker returned a box, `box is not None` after utils.normalize_box.  The
 * empty slice (0,0,0,0) is kept, as the reference keeps it.  One inline function of csrc/og_kernels.hpp (og_gate_keeps) that
 * k_gate_select and og_gate_select_host both call.
 *
 * THE SEQUENCE for B resident frames with their boxes (og_gated_segment_kept_dev; a micro-batch of the *_kept_* stream entries):
 *   k_gate_select     keep[0..n) = the kept frames' indices in ascending order, n into a device word
 *   4-byte copy       of n to a pinned word, an event after it.  THE HOST WAITS FOR THIS EVENT AND FOR NOTHING ELSE: it needs n to
 *                     size the launches that follow; everything after it is enqueued and left to run.
 *   n == B            og_unet_segment_resized_u8_dev in place on the caller's buffers: no gather, no scatter.
 *   n == 0            no network call; area (and mask) are zeroed.
 *   otherwise         k_gate_gather of the kept frames and of their boxes into dense buffers the handle owns; the UNCHANGED
 *                     og_unet_segment_resized_u8_dev on n frames; k_gate_scatter of the areas (and masks) back to frame order,
 *                     which zero-fills every other row in the same launch.
 * In the stream entries the wait for micro-batch k's count happens after the U-Net pass of micro-batch k - 1 has been enqueued, so the
 * card keeps working; the upload and the detector pass of k + 1 still run under the U-Net pass of k.  No stream is added to the
 * fourth header's four, and no graph is captured across streams.  The U-Net's own graph cache holds one graph per batch size
 * (DESIGN.md section 21): n varies from micro-batch to micro-batch, so up to cap - 1 further graphs per frame size are
 * instantiated, each on first use.
 * MEMORY, on top of og_gated_plan's, allocated when a *_kept_* entry is first used: per slot  cap * H * W * channels  (dense frames)
 * + cap * 24 (keep, kept boxes, kept areas) + 4 (count) + cap * H * W once a mask has been asked for, and 4 pinned bytes.
 * og_gated_segment_kept_dev has one such set of its own, sized by the largest B it has seen.
 * ALIGNMENT: int32 buffers (boxes, keep, count, area, n_kept) 4 bytes; u8 rows any address.  A violation is OG_EINVAL before
 * anything is launched, copied or written.
 */
#ifndef OPENGLOTTAL_HIP_GATE_H
#define OPENGLOTTAL_HIP_GATE_H

#include "openglottal_hip.h"
#include "openglottal_hip_gated.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, no handle, no device: boxes [B,4] int32 -> keep_out [count] (room for B), ascending.  Returns the count (>= 0) or a
 * negative code.  B 0..1048576. */
int og_gate_select_host(const int32_t* boxes, int B, int32_t* keep_out);

/* k_gate_select: ONE workgroup; per block of 256 frames an LDS prefix scan of the keep flags plus a running offset (the structure
 * of k_track_boxes), so the compaction is stable.  boxes_dev [B,4], keep_dev [B] (the first *count_dev entries are written),
 * count_dev [1].  B 0..1048576.  Asynchronous on the detector's stream. */
int og_gate_select_dev(og_gated* g, const int32_t* boxes_dev, int B, int32_t* keep_dev, int32_t* count_dev);

/* k_gate_gather: dst row j = src row keep[j] for j < n.  k_gate_scatter: dst row keep[j] = src row j, and every other of the B
 * rows of dst is zero-filled by the same launch (keep ascending, as k_gate_select leaves it).  Rows are row_bytes apart, 1 ..
 * 8192 * 8192 * 3; all offsets are 64-bit.  16 bytes per lane when row_bytes and both bases are multiples of 16, a byte per lane
 * otherwise.  n <= B <= 1048576; src and dst must not overlap.  Asynchronous on the U-Net's stream. */
int og_gate_gather_dev(og_gated* g, const uint8_t* src_dev, size_t row_bytes, const int32_t* keep_dev, int n, uint8_t* dst_dev);
int og_gate_scatter_dev(og_gated* g, const uint8_t* src_dev, size_t row_bytes, const int32_t* keep_dev, int n, int B, uint8_t* dst_dev);

/* THE SEQUENCE above on B resident frames src_dev [B,H,W,channels] with boxes_dev [B,4], everything on the U-Net's stream:
 * area_dev [B] int32 and mask_dev_or_null [B,H,W] u8 come out as og_unet_segment_resized_u8_dev leaves them on kept frames and
 * zero on the others; *n_kept_out (host, may be NULL) = n.  The call returns once n is known; the rest is asynchronous
 * (og_gated_sync / og_unet_sync wait for it).  boxes_dev must be complete when the call is made, as for the U-Net's own entry. */
int og_gated_segment_kept_dev(og_gated* g, const uint8_t* src_dev, int B, int H, int W, int channels, int net_h, int net_w, float threshold,
                              const int32_t* boxes_dev, uint8_t* mask_dev_or_null, int32_t* area_dev, int32_t* n_kept_out);

/* og_gated_stream_u8 / og_gated_stream_frames_u8 with each micro-batch's U-Net step replaced by THE SEQUENCE.  area, boxes, best
 * and the tracker's state are those of og_gated_stream_u8 bit for bit; mask is that of og_gated_stream_u8 on kept frames and ALL
 * ZERO on the others (the one difference: it is what infer.py:255-260 displays).  *n_kept_or_null (host) = kept frames of the call. */
int og_gated_stream_kept_u8(og_gated* g, const uint8_t* frames, int B, int H, int W, int channels, int imgsz, int net_h, int net_w,
                            float conf, float threshold, const uint8_t* resets_or_null, int32_t* area, int32_t* boxes_or_null,
                            float* best_or_null, uint8_t* mask_or_null, int32_t* n_kept_or_null);
int og_gated_stream_kept_frames_u8(og_gated* g, const uint8_t* const* frame_ptrs, int B, int H, int W, int channels, int imgsz, int net_h,
                                   int net_w, float conf, float threshold, const uint8_t* resets_or_null, int32_t* area,
                                   int32_t* boxes_or_null, float* best_or_null, uint8_t* mask_or_null, int32_t* n_kept_or_null);

/* Dry run without a device: og_gated_plan's lines; *engine_bytes (may be NULL) = the engine's device bytes in this mode, i.e.
 * 2 * cap * (H * W * (channels + with_mask) + 41) + 24  plus  2 * (cap * (H * W * (channels + with_mask) + 24) + 4).  with_mask 0 | 1. */
int og_gate_plan(int B, int H, int W, int channels, int stage_kib, int with_mask, char* out, size_t cap, long long* engine_bytes);

#ifdef __cplusplus
}
#endif
#endif
