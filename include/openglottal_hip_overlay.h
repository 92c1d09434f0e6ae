/*
 * openglottal_hip_overlay.h — annotated frames (sixth header; the conventions of openglottal_hip.h -- return codes, og_last_error,
 * *_dev entry points asynchronous on the handle's stream, device restore, a failed call leaves the handle usable -- all hold): the
 * picture scripts/infer.py:91-124 (_draw_overlay) burns into every frame, drawn on the device from what a pipeline's *_dev entry has
 * left there -- the source frame, the mask, the box.  No network is involved, so the family has a handle of its own.
 *
 * Per pixel, in this order; a later rule overwrites an earlier one:
 *
 *   source     a BGR pixel is copied; a one-channel pixel is replicated to B = G = R.
 *   which      with boxes == NULL (the unet-only pipeline) every frame draws its mask and no rectangle.  With boxes, a frame whose box
 *              has x1 < 0 (None as utils.normalize_box leaves it) draws neither.  masks == NULL draws no mask on any frame.
 *   fill       style fill only: where the mask byte is nonzero, G = min(255, G + 102); B and R unchanged.  cv2.addWeighted(out, 1.0,
 *              green, 0.4, 0) on u8: 0.4f * 255 is 102.0000015, G + 102.0000015 rounds to G + 102, no tie can occur.  Masks here
 *              are {0, 255}; ANY nonzero byte counts as 255.
 *   outline    styles fill and contour, colour (0, 255, 0): a pixel set in the mask that lies on the frame's edge or has a 4-neighbour
 *              in the OUTSIDE background, the union of the 4-connected background components that touch the frame's edge.  The
 *              same thing: a pixel of the hole-filled mask with a 4-neighbour off the hole-filled mask or off the frame.  It is what
 *              findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) + drawContours(thickness 1) paint: border following of an
 *              8-connected component visits its pixels 4-adjacent to the surrounding background; components inside a hole are not
 *              external and get none.  Checked against Moore border following (tests/test_overlay_host.py); UNPINNED against OpenCV,
 *              as every cv2 row of this project.
 *   rectangle  colour (0, 220, 255): x1 <= x <= x2 and y in {y1, y2}, or x in {x1, x2} and y1 <= y <= y2, both corners inclusive,
 *              clipped to the frame (the detector's x2 == W column is simply not there).
 *   label      NOT drawn: its glyphs are OpenCV's Hershey table.
 *
 * Each rule is one inline function of csrc/og_kernels.hpp that k_overlay and the *_host entries below both call.
 *
 * STYLES: 0 none (source and rectangle), 1 contour (outline), 2 fill (fill and outline).
 * LAUNCHES per micro-batch: style none, or masks == NULL: k_overlay alone.  Else the outside background is labelled first through the
 * tiled blob filter's path at EVERY frame size (openglottal_hip_classic_tiled.h): k_tblob_background_mask, k_tblob_seams<false>,
 * k_tblob_flatten, k_tblob_border over whole-frame windows, then k_overlay.
 * LIMITS (og_overlay_limit): H * W <= og_classic_tiled_limit(0) pixels, nothing larger has been labelled by these kernels; chunk
 * 1..1024.
 * MEMORY: frames are processed in micro-batches of nb = min(chunk, 64 MiB / (H * W * 3)), at least 1, frames.  The handle's device
 * workspace is that of ONE micro-batch, independent of B: nb * (H * W * 4 + 16) bytes for the outlined styles (one int32 label array,
 * the whole-frame boxes), and for the streamed entries nb * (H * W * (channels + 1 + 3) + 16) bytes more (frames, masks, out, boxes)
 * plus two pinned host slots of that size.  Per buffer the handle keeps the bytes of the largest micro-batch it has run.
 * og_overlay_plan reports the device figure of one streamed call.
 *
 * ALIGNMENT: int32 buffers (boxes, box4) 4 bytes, the frame_ptrs array 8, u8 buffers (frames, masks, out) any address.  A violation is
 * OG_EINVAL before anything is launched, copied or written.
 */
#ifndef OPENGLOTTAL_HIP_OVERLAY_H
#define OPENGLOTTAL_HIP_OVERLAY_H

#include "openglottal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct og_overlay og_overlay;

/* which: 0 max H * W, 1 the number of styles, 2 max chunk; otherwise -1 */
long long og_overlay_limit(int which);

/* Host only, no handle, no device: the rules above by the very inline functions the kernel calls, with a sequential labelling. */

/* mask [H,W] u8 (nonzero = set) -> out [H,W] u8: 255 on the outline, else 0; every byte written.  H * W <= og_overlay_limit(0). */
int og_outline_host(const uint8_t* mask, int H, int W, uint8_t* out);

/* One frame: frame [H,W,channels] u8, channels 1 or 3; mask_or_null [H,W] u8; box4_or_null {x1, y1, x2, y2} int32 as
 * utils.normalize_box leaves it; out_bgr [H,W,3] u8, every byte written. */
int og_overlay_host(const uint8_t* frame, int H, int W, int channels, const uint8_t* mask_or_null, const int32_t* box4_or_null, int style,
                    uint8_t* out_bgr);

/* The device is the one current at the first call that touches it; the handle owns its stream and workspace.  chunk 128. */
og_overlay* og_overlay_create(void);
void og_overlay_destroy(og_overlay* h);
int og_overlay_sync(og_overlay* h);
int og_overlay_set_chunk(og_overlay* h, int chunk);

/* Everything resident on the device: frames_dev [B,H,W,channels] u8, masks_dev_or_null [B,H,W] u8, boxes_dev_or_null [B,4] int32,
 * out_dev [B,H,W,3] u8, every byte written.  Asynchronous on the handle's stream. */
int og_overlay_u8_dev(og_overlay* h, const uint8_t* frames_dev, int B, int H, int W, int channels, const uint8_t* masks_dev_or_null,
                      const int32_t* boxes_dev_or_null, int style, uint8_t* out_dev);

/* Host in, host out, micro-batch by micro-batch through the two pinned slots.  Synchronous.  On an error everything in flight is
 * waited for and the handle stays usable. */
int og_overlay_stream_u8(og_overlay* h, const uint8_t* frames, int B, int H, int W, int channels, const uint8_t* masks_or_null,
                         const int32_t* boxes_or_null, int style, uint8_t* out);

/* The same for a list of separately allocated frames, each of H * W * channels bytes. */
int og_overlay_stream_frames_u8(og_overlay* h, const uint8_t* const* frame_ptrs, int B, int H, int W, int channels,
                                const uint8_t* masks_or_null, const int32_t* boxes_or_null, int style, uint8_t* out);

/* Dry run of og_overlay_stream_u8 (masks and boxes given) without a device: one line per launch in the columns of og_classic_plan,
 * kernel|gx|gy|gz|block|lds|workspace|counters|writes ("out=END": bytes from the start of the caller's out to the end of the
 * launch's writes, or "-").  Returns the number of launches; *workspace_bytes = the device workspace. */
int og_overlay_plan(int B, int H, int W, int channels, int chunk, int style, char* out, size_t cap, long long* workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
