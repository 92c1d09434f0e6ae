/*
 * openglottal_hip_sweep.h — detector ablation sweeps from one inference pass (seventh header; the conventions of openglottal_hip.h --
 * return codes, og_last_error, *_dev entry points asynchronous on the handle's stream, device restore, a failed call leaves the
 * handle usable -- all hold).  The paper's hold-duration ablation (eval_girafe.py --max-hold-frames h, once per value) and its
 * confidence sweep (scripts/sweep_bagls_conf.py) are one computation: the networks run once, afterwards only the detector's decision
 * parameters change and with them the box that gates the U-Net mask.  This family takes what the networks left on the device -- the
 * masks, the ground truth, the detector's `best` rows -- and gives the confusion counts of EVERY (threshold, hold) configuration,
 * reading the masks once.  No network is involved, so the family has a handle of its own.
 *
 * THE RULE.  Inputs, for N frames of one shape H x W:
 *   pred [N,H,W] u8, gt [N,H,W] u8     a pixel is set where its byte is > 0.
 *   best [N,5] f32                     rows x1, y1, x2, y2, conf as the detector leaves them; conf < 0: no detection.
 *   resets [N] u8 or NULL              as og_track_host: a nonzero byte clears EVERY configuration's state before that frame.
 *   conf_thres [n_conf] f64, max_hold [n_hold] int32, and the scalars max_shift_px, padding, inclusive.
 * Configuration c = it * n_hold + ih:
 *   gate       a frame has a detection iff conf >= 0 and, with inclusive = 0, (double)conf > conf_thres[it] -- the detector's own
 *              rule ("conf > conf_thres", openglottal_hip.h), so a column equals a re-run of the detector at that threshold; with
 *              inclusive = 1, (double)conf >= conf_thres[it], as sweep_bagls_conf.py:207 compares a Python float that holds an f32
 *              with a double.  The thresholds are f64 so that 0.02 stays the double 0.02; (float)0.02 is below it.
 *   tracker    the detection flag feeds og_track_advance UNCHANGED (openglottal_hip_gated.h, THE TRACKER RULE), with
 *              max_hold_frames = max_hold[ih]; hold-forever is 2147483647.  The measurement (centre, padded size) does not depend
 *              on the configuration.
 *   mask       the tracker's NORMALISED box gates the prediction: outside the box the prediction is zero, no box gives an empty
 *              prediction -- what k_mask_stats does with boxes.
 * Outputs:
 *   frame_counts [N,3] int32                {tp, n_pred, n_gt} of the ungated mask: the unet-only row, identical to
 *                                           og_mask_stats_dev without boxes.
 *   counts [n_conf*n_hold, N, 3] int32      {tp, n_pred, detected}: the yolo+unet row; detected = the tracker returned a box.
 *   boxes [n_conf*n_hold, N, 4] int32       optional; as og_track_boxes_dev would leave them.
 * Each rule is one inline function (og_sweep_gate, og_track_measure, og_track_advance) that the kernels and og_sweep_host both call.
 *
 * STATE: one og_track_state per configuration, held by the handle (og_sweep_host: by the caller).  It continues from call to call
 * and across micro-batches until og_sweep_reset.  A call whose grid (n_conf, n_hold, the values of conf_thres and max_hold) differs
 * from that of the call before resets it; max_shift_px, padding and inclusive may change without a reset.
 * LIMITS (og_sweep_limit): H * W <= 4194304, n_conf and n_hold 1..32 each, chunk 1..4096.
 * LAUNCHES per micro-batch of nb frames: k_sweep_sat_rows and k_sweep_sat_cols build, per frame, the exclusive summed-area tables
 * of P = pred > 0 and T = pred > 0 && gt > 0 as u32 pairs {P, T} over (H+1) x (W+1), row 0 and column 0 zero, and frame_counts;
 * k_sweep_track walks the micro-batch once per configuration (a lane per configuration); k_sweep_lookup takes four corners of the
 * table per (configuration, frame).  Every entry of the table is rewritten by every micro-batch, so a handle carries nothing but the
 * tracker states from call to call.
 * MEMORY: the handle's workspace is that of ONE micro-batch of nb = min(chunk, N) frames:
 *       workspace_bytes = nb * (8 * (H+1) * (W+1) + 16 * n_conf * n_hold)
 * (tables, boxes), plus 24 bytes of state, 8 of threshold and 4 of hold per configuration row.  The default chunk is
 * max(1, min(4096, 256 MiB / (8 * (H+1) * (W+1)))); og_sweep_set_chunk overrides it.  Results do not depend on the chunk.
 * og_sweep_counts_u8 additionally stages nb * (2 * H * W + 21 + 12 + 28 * n_conf * n_hold) bytes (pred, gt, best, resets,
 * frame_counts, counts, boxes).  og_sweep_plan reports workspace_bytes.
 *
 * ALIGNMENT: conf_thres 8 bytes; float / int32 buffers (best, max_hold, frame_counts, counts, boxes, og_track_state) 4; u8 buffers
 * (pred, gt, resets) any address.  A violation is OG_EINVAL before anything is launched, copied or written.
 */
#ifndef OPENGLOTTAL_HIP_SWEEP_H
#define OPENGLOTTAL_HIP_SWEEP_H

#include "openglottal_hip.h"
#include "openglottal_hip_gated.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct og_sweep og_sweep;

/* which: 0 max H * W, 1 max n_conf, 2 max n_hold, 3 max chunk; otherwise -1 */
long long og_sweep_limit(int which);

/* Host only, no handle, no device: the rule above by the very inline functions the kernels call -- og_track_step per configuration
 * and direct counting inside the box, no tables.  conf_thres and max_hold are host arrays.  states_inout_or_null [n_conf*n_hold]:
 * read and left as after the last frame; NULL starts every configuration without a centre.  boxes_or_null may be NULL. */
int og_sweep_host(const uint8_t* pred, const uint8_t* gt, const float* best, const uint8_t* resets_or_null, int N, int H, int W,
                  const double* conf_thres, int n_conf, const int32_t* max_hold, int n_hold, float max_shift_px, int padding, int inclusive,
                  og_track_state* states_inout_or_null, int32_t* frame_counts, int32_t* counts, int32_t* boxes_or_null);

/* The device is the one current at the first call that touches it; the handle owns its stream, workspace and states. */
og_sweep* og_sweep_create(void);
void og_sweep_destroy(og_sweep* h);
int og_sweep_sync(og_sweep* h);
int og_sweep_set_chunk(og_sweep* h, int chunk);   /* 1..og_sweep_limit(3); 0 restores the default */
int og_sweep_reset(og_sweep* h);                  /* every configuration: no centre; ordered after the work already enqueued */
/* the state of configuration c of the last call's grid, after everything enqueued (it waits) */
int og_sweep_get_state(og_sweep* h, int c, og_track_state* state);

/* Everything resident on the device except the grid: pred_dev, gt_dev [N,H,W] u8, best_dev [N,5] f32, resets_dev_or_null [N] u8;
 * conf_thres [n_conf] and max_hold [n_hold] are HOST arrays, copied before the call returns; frame_counts_dev [N,3],
 * counts_dev [n_conf*n_hold,N,3], boxes_dev_or_null [n_conf*n_hold,N,4] int32, every element written.  Asynchronous on the
 * handle's stream; N may exceed the chunk. */
int og_sweep_counts_u8_dev(og_sweep* h, const uint8_t* pred_dev, const uint8_t* gt_dev, const float* best_dev,
                           const uint8_t* resets_dev_or_null, int N, int H, int W, const double* conf_thres, int n_conf,
                           const int32_t* max_hold, int n_hold, float max_shift_px, int padding, int inclusive, int32_t* frame_counts_dev,
                           int32_t* counts_dev, int32_t* boxes_dev_or_null);

/* The same with every buffer on the host, staged micro-batch by micro-batch.  Synchronous.  On an error nothing is left in flight
 * and the handle stays usable; the states are those after the last micro-batch that ran. */
int og_sweep_counts_u8(og_sweep* h, const uint8_t* pred, const uint8_t* gt, const float* best, const uint8_t* resets_or_null, int N, int H,
                       int W, const double* conf_thres, int n_conf, const int32_t* max_hold, int n_hold, float max_shift_px, int padding,
                       int inclusive, int32_t* frame_counts, int32_t* counts, int32_t* boxes_or_null);

/* Dry run without a device: one line "b0|nb" per micro-batch into out (cap bytes); returns their number (0 for N = 0).  chunk:
 * 1..og_sweep_limit(3), or 0 for the default.  *workspace_bytes (may be NULL) = the formula under MEMORY. */
int og_sweep_plan(int N, int H, int W, int n_conf, int n_hold, int chunk, char* out, size_t cap, long long* workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
