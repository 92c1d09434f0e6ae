/*
 * openglottal_hip_gated.h — the detection-gated pipeline in one device pass (fourth header; the conventions of openglottal_hip.h --
 * return codes, og_last_error, *_dev entry points, device restore -- all hold): the temporal tracker of
 * openglottal/models/detector.py:61-96 on the device, and an engine that uploads each source frame ONCE and feeds it to the
 * detector and to the U-Net (features.py:234-245, `--pipeline unet` with a detector).
 *
 * THE TRACKER RULE, per frame, from the detector's `best` row {x1, y1, x2, y2, conf} (conf < 0: no detection; rows are finite, as
 * the detector leaves them: it clips to the frame) and the state {centre 2 x f32, size 2 x int32, misses, has-centre}.  All float
 * arithmetic is f32, as numpy 2 does it on np.float32 scalars:
 *
 *   measure   cx = (x1 + x2) / 2, cy = (y1 + y2) / 2;  w = (int)(x2 - x1) + 2 * padding, h likewise ((int): toward zero).
 *   jump      with a centre and a detection: hypot(cx - centre.x, cy - centre.y) > (float)max_shift_px makes the detection a miss.
 *             hypot = (float)sqrt((double)dx * dx + (double)dy * dy), no FMA.
 *   accept    a detection that is no jump becomes the state; misses = 0.
 *   hold      a miss with a centre: ++misses; above max_hold_frames the state is cleared.
 *   box       none without a centre.  Else hw = floor(w / 2), hh = floor(h / 2);
 *             bx = (int)min(max(centre.x, (float)hw), (float)(W - hw)) (np.clip: the upper bound where the bounds cross), by
 *             likewise; (bx - hw, by - hh, bx + hw, by + hh).
 *   normalise utils.normalize_box: Python slice semantics per axis (a negative end is counted from the far edge, then both are
 *             clamped to 0..W / 0..H); (0,0,0,0) for an empty slice, (-1,-1,-1,-1) for no box.
 *
 * One inline function of csrc/og_kernels.hpp (og_track_step) that k_track_boxes and og_track_host both call.
 *
 * THE ENGINE, per micro-batch of at most  cap = min(4096, max(1, stage_kib * 1024 / (H * W * channels)))  frames: one copy into a
 * slot of a two-slot pinned ring (skipped for caller-pinned frames) and up to the slot's device stage; on the detector's stream
 * og_yolo_detect_resized_u8_dev and k_track_boxes; on the U-Net's stream, after an event, og_unet_segment_resized_u8_dev on the SAME
 * device frames with those boxes; areas (and boxes / best / mask when asked for) come back through the slot.  The upload and the
 * detector pass of micro-batch k + 1 run under the U-Net pass of micro-batch k.  Streams are ordered by events only; no graph is
 * captured across them.
 * MEMORY: two slots of cap * (H * W * (channels + 1) + 41) bytes on the device (the mask's H * W only once a mask has been asked
 * for) and as many pinned, plus 24 bytes of tracker state: a function of the setting and the frame size, independent of B.  The
 * detector's and the U-Net's own workspaces are theirs (og_yolo_plan, og_unet_plan_resized).  og_gated_plan reports the engine's
 * device bytes, mask included.  The detector runs its batched kernels for every micro-batch, also one of a single frame, so a
 * frame's results do not depend on where the setting cuts the video.
 * ALIGNMENT: float / int32 buffers (best, boxes, area, og_track_state, og_track_params) 4 bytes, the frame_ptrs array 8, u8
 * buffers (frames, resets, mask) any address.  A violation is OG_EINVAL before anything is launched, copied or written.
 */
#ifndef OPENGLOTTAL_HIP_GATED_H
#define OPENGLOTTAL_HIP_GATED_H

#include "openglottal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct og_gated og_gated;

typedef struct og_track_state {
    float cx, cy;          /* centre of the last accepted detection */
    int32_t w, h;          /* its size, padding included */
    int32_t misses;
    int32_t has_centre;    /* 0: no centre; every other word is then 0 */
} og_track_state;

typedef struct og_track_params {
    float max_shift_px;    /* 30 */
    int32_t padding;       /* 8 */
    int32_t max_hold_frames; /* 3 */
} og_track_params;

/* Host only, no handle, no device: B frames through the rule, in order.  best [B,5] f32, resets_or_null [B] u8 (nonzero: the
 * state is cleared before that frame), boxes_out [B,4] int32.  *state_inout is read and left as after the last frame. */
int og_track_host(og_track_state* state_inout, const og_track_params* params, const float* best, const uint8_t* resets_or_null, int B,
                  int W, int H, int32_t* boxes_out);

/* Dry run of og_gated_stream_u8 without a device: one line "b0|nb" per micro-batch into out (cap bytes); returns their number;
 * *engine_bytes (may be NULL) = the engine's own device bytes.  stage_kib 1..16777216; below one frame each frame is staged alone. */
int og_gated_plan(int B, int H, int W, int channels, int stage_kib, char* out, size_t cap, long long* engine_bytes);

/* The handle.  Both network handles are BORROWED (they must outlive it and must not be driven by another thread during a call),
 * finalized (OG_ESTATE otherwise) and on one device (OG_EINVAL otherwise).  A new handle has the tracker's defaults (30, 8, 3), no
 * centre, stage_kib 65536.  NULL on an error (og_last_error). */
og_gated* og_gated_create(og_unet* unet, og_yolo* yolo);
void og_gated_destroy(og_gated* g);
int og_gated_sync(og_gated* g);   /* waits for everything the handle has enqueued; reports OG_ERANGE of either network */

/* "stage_kib" (1..16777216): KiB of source frames per micro-batch. */
int og_gated_set_option(og_gated* g, const char* name, int value);

/* The tracker's state.  og_gated_reset and og_gated_set_state are ordered after the work already enqueued; og_gated_get_state
 * waits for it.  og_gated_set_params takes effect with the next launch and leaves the state alone. */
int og_gated_reset(og_gated* g);
int og_gated_set_params(og_gated* g, const og_track_params* params);
int og_gated_get_state(og_gated* g, og_track_state* state);
int og_gated_set_state(og_gated* g, const og_track_state* state);

/* k_track_boxes over B resident rows, continuing from the handle's state: best_dev [B,5] f32, resets_dev_or_null [B] u8, boxes_dev
 * [B,4] int32.  Asynchronous on the detector's stream (og_gated_sync / og_gated_get_state wait for it). */
int og_track_boxes_dev(og_gated* g, const float* best_dev, const uint8_t* resets_dev_or_null, int B, int W, int H, int32_t* boxes_dev);

/* The gated frame loop over B frames on the HOST: frames [B,H,W,channels] u8 (channels 1 gray | 3 BGR) at their own size; the
 * detector letterboxes to imgsz, the U-Net resizes to net_h x net_w and back (at network size: the plain chain).  conf: the
 * detector's confidence threshold; threshold: the mask's.  resets_or_null [B] u8 as og_track_host.  Outputs: area [B] int32 (the
 * mask's pixels inside the frame's box; 0 without one), boxes_or_null [B,4] int32, best_or_null [B,5] f32 (source pixels),
 * mask_or_null [B,H,W] u8 {0,255}.  Synchronous.  The tracker continues from call to call until og_gated_reset.  On an error
 * nothing is left in flight, all three handles stay usable and the tracker's state is that after the last micro-batch that ran. */
int og_gated_stream_u8(og_gated* g, const uint8_t* frames, int B, int H, int W, int channels, int imgsz, int net_h, int net_w, float conf,
                       float threshold, const uint8_t* resets_or_null, int32_t* area, int32_t* boxes_or_null, float* best_or_null,
                       uint8_t* mask_or_null);

/* The same for a list of separately allocated frames, each of H * W * channels bytes. */
int og_gated_stream_frames_u8(og_gated* g, const uint8_t* const* frame_ptrs, int B, int H, int W, int channels, int imgsz, int net_h,
                              int net_w, float conf, float threshold, const uint8_t* resets_or_null, int32_t* area,
                              int32_t* boxes_or_null, float* best_or_null, uint8_t* mask_or_null);

#ifdef __cplusplus
}
#endif
#endif
