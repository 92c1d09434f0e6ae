/*
 * openglottal_hip_crops.h — the YOLO-Crop+UNet video pipeline of the C-ABI (second header; include it instead of, or next
 * to, openglottal_hip.h, whose conventions -- return codes, og_last_error, *_dev entry points, device restore -- all hold).
 *
 * Reference: the `yolo-crop+unet` branch of scripts/infer.py:222-248.  Per frame
 *     gray = cvtColor(frame, BGR2GRAY); box = detector.detect(frame)                        (:226-227)
 *     crop = gray[y1:y2, x1:x2]; boxed, geometry = letterbox_with_info(crop, 256, value=0)  (:232-237, utils.py:97-134)
 *     mask_cs = unet_segment_frame(boxed, crop_model, device)                               (:238)
 *     mask_orig = unletterbox(mask_cs, geometry, crop_h, crop_w, INTER_NEAREST)             (:239-242, utils.py:166-186)
 *     full[y1:y2, x1:x2] = mask_orig; area = sum(mask_orig > 0)                             (:243-246)
 * and area 0 / no mask for a frame without a box or with an empty crop (:228-233).  The detector stays with the caller
 * (og_yolo_detect_* and the temporal state machine): the boxes are an input here.
 *
 * Arithmetic (stated once, in csrc/og_kernels.hpp, as inline functions that the kernels and the *_host entries below both
 * call):
 *   geometry    scale = size / max(h, w) in double; content sides nh = rint(h * scale), nw = rint(w * scale) -- half to even,
 *               as Python's round() --; pad_top = (size - nh) / 2, pad_left = (size - nw) / 2.   geom4 = {pad_top, pad_left, nh, nw}
 *   usable box  0 <= x1 < x2 <= W, 0 <= y1 < y2 <= H and nh >= 1 and nw >= 1.  Anything else -- x1 < 0 ("no detection"), an
 *               empty or out-of-frame box, a sliver whose short side rounds to 0 (1 x 64 at size 32; cv2.resize raises on it)
 *               -- is "no detection": area 0, all-zero mask, and it does not end the call.
 *   tile pixel  gray(frame[y1 + nearest(ty - pad_top, y2 - y1, nh)][x1 + nearest(tx - pad_left, x2 - x1, nw)]) inside the content
 *               rectangle, 0 outside; nearest(d, src, dst) = min(floor(d * src / dst), src - 1) in double (INTER_NEAREST);
 *               gray() of a BGR pixel is the 15-bit fixed point of og_bgr2gray_host, so converting per tap equals converting the
 *               frame first.
 *   projection  frame pixel (x, y) inside the box takes tile_mask[pad_top + nearest(y - y1, nh, y2 - y1)][pad_left +
 *               nearest(x - x1, nw, x2 - x1)] (a side with nh == y2 - y1 is copied); outside the box 0.
 *               area = number of box pixels whose value is > 0.
 * Parity against a real cv2 is unpinned, as for every other geometry entry (OpenCV is absent from the build image).
 *
 * ALIGNMENT, as in the main header: int32 buffers (boxes, box4, geom4, area) 4 bytes, the frame_ptrs array 8, u8 buffers
 * (frames, each frame_ptrs[i], tile, tile_mask, mask, the scratch buffers) any address.  A violation is OG_EINVAL before
 * anything is launched, copied or written.
 */
#ifndef OPENGLOTTAL_HIP_CROPS_H
#define OPENGLOTTAL_HIP_CROPS_H

#include "openglottal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, no handle, no device: the arithmetic above by the very inline functions the kernels call ------------------ */

/* letterbox_with_info's scalars (utils.py:114-122) for an h x w crop.  OG_EINVAL: h, w or size < 1, geom4 null.  A side that
 * rounds to 0 is REPORTED (geom4[2] or geom4[3] is 0, return 0): whether a box is usable is the caller's question. */
int og_crop_geometry_host(int h, int w, int size, int32_t* geom4);

/* boxed = letterbox_with_info(gray(frame)[y1:y2, x1:x2], size, value=0)[0] (infer.py:232-237): frame [H,W,channels] u8
 * (1 gray, 3 BGR), box4 = {x1, y1, x2, y2}, tile [size,size] u8.  An unusable box gives an all-zero tile (return 0). */
int og_crop_tile_host(const uint8_t* frame, int H, int W, int channels, const int32_t* box4, int size, uint8_t* tile);

/* infer.py:239-246: tile_mask [size,size] u8 -> *area = sum(mask_orig > 0) and, when mask_or_null is given, the full frame
 * [H,W] u8 (every byte written: the paste inside the box, 0 outside).  An unusable box gives *area = 0 and a zero frame. */
int og_crop_project_host(const uint8_t* tile_mask, int size, const int32_t* box4, int H, int W, uint8_t* mask_or_null,
                         int32_t* area);

/* The video pass -------------------------------------------------------------------------------------------------------- */

/* = the loop body of scripts/infer.py:222-248 over a video on the HOST, streamed through the ring of og_unet_stream_u8 and
 * COMPACTED: the boxes are host inputs, so only frames with a usable box are copied (frame by frame) into the pinned ring,
 * uploaded and segmented -- micro-batches are filled with usable frames only and results are scattered back to their frame
 * indices; every other frame gets area 0 and a zeroed mask from the host and costs nothing on the device.  A frame's result
 * does not depend on its micro-batch, so compaction changes no bit.
 * frames [B,H,W,channels] u8 (1 gray, 3 BGR: converted per tap on the device); boxes [B,4] int32 {x1,y1,x2,y2} in frame
 * pixels, already clamped as Python slicing does (x1 < 0: no detection); size: the tile side, a multiple of 2^n_levels;
 * mask [B,H,W] u8 {0,255} or NULL; area [B] int32 or NULL.  Synchronous.
 * Micro-batch = min(chunk, 64 MiB / (H*W*channels)) frames, at least 1; device memory = (lanes + 2) ring slots of one
 * micro-batch each (source frames, tiles, tile masks, areas, boxes, and full masks when asked for) + the arenas at
 * size x size: independent of B.  Errors: as og_unet_stream_u8 (everything in flight is waited for, the handle stays usable);
 * OG_ERANGE from "precision" 1 / 2 as there. */
int og_unet_stream_crops_u8(og_unet* h, const uint8_t* frames, int B, int H, int W, int channels, const int32_t* boxes,
                            int size, float threshold, uint8_t* mask, int32_t* area);

/* The same for a list of separately allocated frames (infer.py's `frames_bgr`), each of H*W*channels bytes. */
int og_unet_stream_frames_crops_u8(og_unet* h, const uint8_t* const* frame_ptrs, int B, int H, int W, int channels,
                                   const int32_t* boxes, int size, float threshold, uint8_t* mask, int32_t* area);

/* Resident frames: src_dev [B,H,W,channels] u8 and boxes_dev [B,4] int32 on the device, asynchronous on the handle's stream,
 * one lane, NO compaction (the boxes are not readable here: a frame without a usable box runs the network on a zero tile and
 * still gives area 0 and a zero mask).  tiles_scratch_dev and tile_masks_scratch_dev: [B,size,size] u8 each, fully written.
 * mask_dev [B,H,W] u8 or NULL; area_dev [B] int32 or NULL. */
int og_unet_segment_crops_area_u8_dev(og_unet* h, const uint8_t* src_dev, int B, int H, int W, int channels,
                                      const int32_t* boxes_dev, int size, float threshold, uint8_t* tiles_scratch_dev,
                                      uint8_t* tile_masks_scratch_dev, uint8_t* mask_dev, int32_t* area_dev);

/* Dry run of og_unet_stream_crops_u8 without a device, as og_unet_plan_resized: the boxes (host) decide the compaction.
 * One line per launch: kernel|gx|gy|gz|block|lds|workspace|counters|writes, where `writes` names the ring-slot buffers the
 * launch writes as "mask=END;area=END" (bytes from the slot buffer's start to the end of the launch's writes) or "-".
 * options: "name=value,..." of og_unet_set_option, and "chunk=N".  Returns the number of launches (0 when no box is usable),
 * *arena_bytes = the activation arena of one lane. */
int og_unet_plan_crops(const int* features, int n_levels, int B, int H, int W, int channels, const int32_t* boxes, int size,
                       int lanes, const char* options, char* out, size_t cap, long long* arena_bytes);

#ifdef __cplusplus
}
#endif
#endif
