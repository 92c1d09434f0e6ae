/*
 * openglottal_hip_mjps.h — split entropy decode: Motion-JPEG WITHOUT restart markers decoded in parallel (eleventh header; the
 * conventions of openglottal_hip.h and everything decode/openglottal_hip_mjpd.h states -- ACCEPTED, REFUSED, STATUS, ARITHMETIC, LIMITS,
 * ALIGNMENT -- hold unchanged).  An opt-in mode of the og_mjpd handle.  The tenth header's parallelism is the restart interval: a file
 * without DRI (OpenCV's MJPG writer, FFmpeg's mjpeg, most cameras, Pillow's default) is one interval, one lane of k_mjpd_entropy per
 * frame.  With the mode on, a call whose Ri is 0 runs k_mjps_entropy instead, which cuts the frame's scan into subsequences and lets
 * them synchronise themselves.  Coefficients, pixels and status[f] are og_jpegd_interval's for EVERY input, damaged files included;
 * a call with Ri > 0 launches exactly what it launches with the mode off.  Nothing takes this path by default.
 *
 * ALGORITHM, exact, not heuristic; inline functions of csrc/og_mjps.inc that og_jpegs_decode_host and the kernel both call.
 *   DATA END.  The scan is cut where og_jpegd_fill would stop: at the first 0xFF that is not followed by 0x00, or that is the scan's last
 *     byte.  It is found (a minimum over the lanes' hits) before anything is decoded; no lane starts at or past it and bytes[i] is read
 *     only for i < length.
 *   LANES.  The data is cut into subsequences of `sub` bytes; lane i owns subsequence i.  A symbol with its value bits belongs to the
 *     lane in whose subsequence its first bit lies, so a lane decodes from its entry state until the next symbol would start at or
 *     past its end (the frame's last lane: until the data ends), and a lane whose entry lies at or past its end passes it through.
 *   STATE between two symbols, 8 bytes: the raw byte index and bit of the next bit (never inside a stuffed 00), the block within the
 *     MCU (it selects component and tables), the zigzag index (0: a DC symbol is next); or "dead with status s".  The reader of
 *     og_mjpd.inc is restarted from such a position (og_jpegd_seek) and asked for it (og_jpegd_tell); og_jpegd_interval is unchanged.
 *   ENTRIES.  Lane 0 enters with the true start; every other lane first enters speculatively at its first data byte, block 0, DC next.
 *   ROUNDS.  In each round lane i takes lane i - 1's exit of the round before as its entry and decodes again only if that entry
 *     changed; the rounds end when no entry changed.  Lane 0 is always right, so after round r lanes 0..r are right: the fixed point is
 *     the sequential parse, reached after at most (lanes of the window) rounds -- the loop is bounded by that count -- and the worst
 *     case, one lane becoming right per round, costs one lane's walk per round: the sequential decode's time, no more.  Huffman codes
 *     resynchronise, so a speculative lane's EXIT is usually right although its entry was not, and two or three rounds are the rule
 *     (og_jpegs_decode_host counts them).
 *     In the rounds only missing bits (status 1: the data has ended) leave "dead", and every lane behind a dead entry is dead.  An
 *     invalid code, a run or ZRL that leaves the block and a category out of range (2, 3, 4) do NOT kill in the rounds: the block
 *     ends there (an invalid code also drops one bit) and the parse goes on.  The reason is measured in DESIGN section 24: a
 *     speculative parse in the wrong phase meets them all the time (nine 1-bits are no DC code of the Annex K table), and a dead exit
 *     that later rounds have to take back moves down the lanes one per round, exactly as fast as the right states that follow it,
 *     so one such lane costs a round per lane behind it.  Exactness does not depend on what a wrong parse does: the rounds' parse
 *     equals the sequential one up to the first error, the write pass below is strict and finds that error, and what lanes behind it
 *     wrote is taken back.
 *   RESULTS.  After the rounds each lane knows, for its right entry, how many blocks it starts and the sum of its DC differences per
 *     component.  Exclusive scans over the lanes give its first block in stream order and its three predictors.  The sums are kept
 *     modulo 2^32; for the blocks of the frame they cannot wrap: a difference is at most 2 047 in magnitude (category <= 11) and a
 *     component has at most H W / 64 + (H + W) / 4 + 4 < 2^19 blocks below og_mjpeg_limit(0) = 2^24 pixels (H, W <= 65 535), so a
 *     sum stays below 2^30.  (Bytes behind the last MCU may hold any number of "blocks"; their sums are never used.)
 *   WRITE PASS.  Each lane decodes once more, strictly, and writes where og_jpegd_interval writes ([component][block][64], natural
 *     order, the DC predicted), up to block M * blocks-per-MCU: bytes behind the last MCU are ignored and an error there does not
 *     exist.  A lane stops at its first error -- an entropy error or the DC range check (prediction outside [-2048, 2047]), whose
 *     block gets no DC and no AC -- and reports the key (4 * block + phase) * 8 + status, phase 0 a DC symbol, 1 the range check, 2 an
 *     AC symbol: the order in which og_jpegd_interval meets them.  The lowest key of the frame is its first error in stream order and
 *     gives status[f]; the lanes of that window behind the erring lane run the same walk once more storing 0 (each coefficient is
 *     addressed by one symbol of one lane, so this restores the zeros), and later windows are not decoded.
 *
 * KERNEL k_mjps_entropy, gfx950, wave64: one workgroup of 256 lanes per frame, grid = frames of the micro-batch; it honours
 * k_mjpd_markers' verdict (a frame it refused is skipped) and raises status[f] with atomicMax.  The frame's table set lies in LDS.  The scan
 * is walked in windows of min(256, 32 768 / sub) subsequences, in order: the window's bytes and og_mjps_limit(4)'s 16 bytes of slack
 * (a lane's last symbol runs at most 12 raw bytes past its end) are staged in LDS with aligned dword loads, the lanes read their
 * dependent byte chain from LDS; the states lie in LDS (two copies, one barrier per round: __syncthreads_or(changed)); the scans are
 * wave shuffles and one LDS step over the four waves.  The converged exit of a window's last lane, the block count and the
 * predictors are the next window's exact entry.  Static LDS og_mjps_limit(5) bytes <= 64 KiB; no workgroup waits for another; every
 * loop is bounded (windows by the scan's length, rounds by the lanes, a lane's walk by its bytes).  No new workspace.
 *
 * LIMITS (og_mjps_limit): sub a multiple of 4 in 4..1024, default og_mjps_limit(0); 256 lanes and 32 768 bytes per window.
 */
#ifndef OPENGLOTTAL_HIP_MJPS_H
#define OPENGLOTTAL_HIP_MJPS_H

#include "../decode/openglottal_hip_mjpd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* which: 0 the default sub, 1 its minimum, 2 its maximum, 3 lanes per window, 4 bytes of a window, 5 static LDS bytes of
 * k_mjps_entropy; otherwise -1 */
long long og_mjps_limit(int which);

/* mode 0 (the default): the handle launches exactly what it launches without this header.  mode 1: og_mjpd_decode_u8_dev and
 * og_mjpd_decode_stream send calls with Ri == 0 through k_mjps_entropy; calls with Ri > 0 are unchanged.  sub 0: the measured default;
 * otherwise a multiple of 4 in 4..1024.  OG_EINVAL otherwise, and the handle keeps what it had.  No device is touched. */
int og_mjps_set_split(og_mjpd* h, int mode, int sub);

/* og_mjpd_plan with the mode: with mode 1 and Ri == 0 the launches are k_mjpd_markers, k_mjps_entropy (grid = frames of the
 * micro-batch, block 256, its static LDS), k_mjpd_idct, k_mjpd_colour; otherwise og_mjpd_plan's text, byte for byte. */
int og_mjps_plan(int B, int H, int W, int sampling, int Ri, int chunk, int mode, int sub, char* out, size_t cap, long long* workspace_bytes);

/* The twin: og_jpegd_decode_host with the split pass, the lanes walked in a loop, round by round.  sub as above; lanes 1..256 per
 * window (the kernel's is min(256, 32 768 / sub), which also caps this), so that a small file can be made to take many windows.
 * stats, int32[4] or null: lanes in all, windows, the most rounds of a window (the round that finds nothing changed included), lane
 * decodes of the rounds in all.  A file with restart markers is decoded as og_jpegd_decode_host decodes it and leaves stats 0. */
int og_jpegs_decode_host(const uint8_t* jpeg, size_t size, int sub, int lanes, uint8_t* out_bgr, size_t cap, int* status, int32_t* stats);

#ifdef __cplusplus
}
#endif
#endif
