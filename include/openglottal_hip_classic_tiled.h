/*
 * openglottal_hip_classic_tiled.h — the training-free family on frames of any size (fifth header; everything of
 * openglottal_hip_classic.h holds, and every function here works on the same og_classic handle): a blob filter that spreads ONE
 * frame over many workgroups, opted into per handle.
 *
 * k_blobs labels a frame with one workgroup, which bounds the family at 65 536 pixels (og_classic_limit(0)).  The tiled form cuts
 * the frame into tiles of T x T pixels (T = og_classic_tiled_limit(1)); a tile's workgroup labels its tile in LDS, and launch
 * boundaries on the handle's stream stand where workgroups must see each other's results (tile roots, seam merges, flattening,
 * border flags, hole fill, keys, top-n selection, paint and count).  It computes the SAME unique labelling as k_blobs -- the root of
 * a component is its raster-first pixel in the window, the key is og_window_key's, the order og_blob_rank's -- so masks and areas
 * are equal bit for bit, and so are the thresholds (the histogram's integer atomics do not depend on the block count).
 *
 * MODES (og_classic_set_tiled): 0 off, the default -- nothing changes, limit and messages included; 1 auto -- k_blobs up to
 * 65 536 pixels, tiled above; 2 always -- tiled at every size.
 * LIMITS (og_classic_tiled_limit): in modes 1 and 2, H * W <= og_classic_tiled_limit(0) pixels, the largest frame whose worst-case
 * masks (spiral, its transpose, serpentine, nested rings) have been launched and timed.
 * MEMORY: as openglottal_hip_classic.h, plus 36 bytes per frame of the micro-batch (the roots taken: 8 int32 and their count) once
 * a call has gone through the tiled filter: nb * (H * W * (channels + 1 + 8) + 1096) + 8 bytes of device workspace.  The label
 * arrays stay at 8 bytes per pixel.  og_classic_plan_tiled reports the figure of one call.
 */
#ifndef OPENGLOTTAL_HIP_CLASSIC_TILED_H
#define OPENGLOTTAL_HIP_CLASSIC_TILED_H

#include "openglottal_hip_classic.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mode 0 off (the default), 1 auto, 2 always; anything else is OG_EINVAL.  Touches no device.  In modes 1 and 2
 * og_vft_guided_init_u8, og_vft_guided_stream_u8, og_vft_guided_stream_frames_u8, og_vft_guided_u8_dev, og_otsu_in_box_u8 and
 * og_otsu_in_box_u8_dev accept frames up to og_classic_tiled_limit(0) pixels; their other rules are unchanged. */
int og_classic_set_tiled(og_classic* h, int mode);

/* which: 0 max H * W in modes 1 and 2, 1 the tile edge T; otherwise -1 */
long long og_classic_tiled_limit(int which);

/* og_blobs_host without its 65 536-pixel limit (H * W up to 2^30): the same sequential body. */
int og_blobs_host_any(const uint8_t* mask, int H, int W, int n_components, uint8_t* out_mask_or_null, int32_t* area);

/* og_classic_plan for mode 1 or 2: one line per launch with the kernels and grids that would run.  Tile kernels have grid
 * (tiles of the frame, frames of the micro-batch), per-pixel kernels (ceil(pixels / 256), frames).  In mode 1 at H * W <= 65 536
 * the text equals og_classic_plan's. */
int og_classic_plan_tiled(int B, int H, int W, int channels, int chunk, int mode, char* out, size_t cap, long long* workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
