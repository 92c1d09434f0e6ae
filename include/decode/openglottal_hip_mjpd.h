/*
 * openglottal_hip_mjpd.h — baseline JPEG decoded on the device (tenth header; the conventions of openglottal_hip.h -- return codes,
 * og_last_error, *_dev entry points asynchronous on the handle's stream, device restore, a failed call leaves the handle usable -- all
 * hold).  The input side of openglottal_hip_mjpeg.h: the chunks of a Motion-JPEG AVI (what scripts/infer.py and
 * openglottal/utils.py:load_frames_bgr read through OpenCV, and what `cli infer --avi device` writes) go up COMPRESSED and become
 * [B,H,W,3] u8 BGR frames on the device.  The judge is Pillow's libjpeg(-turbo) decoder: inside the bound stated under ARITHMETIC the
 * host twin gives its bytes exactly, and the device gives the twin's bytes on every stream.  Parity with OpenCV's or FFmpeg's decoders
 * is UNPINNED, as every cv2 row of this project.
 *
 * ACCEPTED.  Sequential baseline DCT (SOF0), 8 bit, Huffman, ONE interleaved scan (Ss 0, Se 63, Ah Al 0) of
 *   sampling 0   one component (gray; its sampling factors do not matter, the scan is not interleaved: one block per MCU);
 *   sampling 1   three components, JFIF YCbCr, 4:4:4 (luma 1x1, chroma 1x1): an MCU is Y Cb Cr;
 *   sampling 2   4:2:2 (luma 2x1): Y Y Cb Cr, 16 x 8 pixels;
 *   sampling 3   4:2:0 (luma 2x2): Y Y Y Y Cb Cr, 16 x 16 pixels;
 * DQT (8 bit, ids 0..3) and DHT (classes 0 and 1, ids 0 and 1) anywhere before SOS, several per segment, later ones replacing earlier
 * ones; DRI present or absent (Ri = 0: the scan is one interval); APPn, COM and unknown segments with a length are skipped.  A file
 * with NO DHT at all is decoded with the four tables of ITU T.81 Annex K.3 (the AVI "MJPG" convention of many cameras; IJG libjpeg
 * refuses such files, libjpeg-turbo installs the same tables).  M = MCUs of the frame, nI = ceil(M / Ri) restart intervals (1 without DRI).
 * REFUSED by the parser, with the reason in og_last_error and status 6, never decoded approximately: no SOI; SOF1, SOF2 and every
 * other SOFn; 12-bit samples; DAC (arithmetic coding); other sampling factors (4:4:0, 4:1:1, chroma above 1x1); two or four
 * components; a scan that does not hold all components in SOF order, or spectral selection / successive approximation; a second scan;
 * 16-bit DQT; a table the scan names but no segment defined; a DHT whose counts do not form a prefix code; H or W of 0; H * W above
 * og_mjpd_limit(0) = og_mjpeg_limit(0); a file above og_mjpd_limit(5) = 2^30 bytes; a truncated header.
 *
 * STATUS per frame (int32): 0 ok, or
 *   1 truncated scan: an interval's bytes ended (or a marker other than RSTm stood) where a code or its value bits were due;
 *   2 invalid Huffman code: 16 bits that are no code of the table;
 *   3 coefficient index past 63 (a run or ZRL that leaves the block);
 *   4 value outside the baseline range: DC category above 11, AC category above 10, or a DC after prediction outside [-2048, 2047];
 *   5 marker count or order: the scan does not hold exactly nI - 1 RSTm, or the k-th is not RST(k mod 8);
 *   6 unsupported form (the list above; also a record whose extents leave its file or whose table set does not exist);
 *   7 the frame's H x W, sampling or Ri differ from the call's.
 * A frame with a non-zero status never stops its neighbours, and the call returns OG_OK.  Its pixels are defined: 6 and 7: every byte 0;
 * 5: no interval is decoded (every coefficient 0: mid-gray); 1..4: every interval is decoded on its own up to its first error, the
 * coefficients it did not reach stay 0, and the frame's status is the LARGEST code among its intervals.  og_jpegd_decode_host gives the
 * same pixels for the same bytes (for 6 it writes nothing: it does not know a size).
 *
 * ARITHMETIC, integer only; inline functions of csrc/og_mjpd.inc that og_jpegd_decode_host and the kernels both call.  `>>` is the
 * arithmetic shift.
 *   og_jpegd_interval  entropy decoding of ONE restart interval over (bytes, length, tables, first MCU, MCU count): DC predictors 0
 *                      at its start, 9-bit look-ahead then the canonical maxcode walk for codes of 10..16 bits, EOB, ZRL, EXTEND,
 *                      0xFF00 unstuffing; int16 coefficients in natural order.  SAFETY: it reads bytes[i] only for i < length (an
 *                      0xFF is data only if bytes[i + 1] exists and is 0x00; anything else ends the data); it writes only blocks of
 *                      MCUs [first, first + count), 64 int16 each, index = zigzag[k] with k checked <= 63 before every write; its
 *                      loops are MCUs < count, blocks of an MCU <= 6, k < 64, code lengths <= 16, and a refill that consumes at
 *                      least one byte per turn; on an error it returns the status at once.
 *   og_jpegd_idct8     libjpeg's jidctint "islow" pass: 13-bit constants 2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995
 *                      25172, PASS1_BITS 2; columns first, descale (x + 2^10) >> 11, then rows, descale (x + 2^17) >> 18, + 128, clamp
 *                      to 0..255.  Dequantisation is coefficient * table entry in 32 bits.  Everything runs in 32-bit wrap-around
 *                      (unsigned) arithmetic, so no stream has undefined behaviour.
 *                      BOUND.  Every intermediate of a pass -- each sum before a multiply, each product, each partial sum, each
 *                      result -- is a linear form w . in of the pass's 8 inputs; over all of them the largest Euclidean norm
 *                      |w|_2 is 31 871.2 (tests/test_mjpd_host.py recomputes it and holds its walk of the pass to
 *                      og_jpegd_idct_pass_host; the results themselves have 2^13 sqrt(8) = 23 170.5).  With E = the Euclidean norm of a block's 64 dequantised values: pass 1 stays
 *                      below 31 872 E + 2^10; its results are 4 sqrt(8) times an orthonormal transform, rounded, so their norm is at
 *                      most 11.32 E + 4; pass 2 stays below 31 872 (11.32 E + 4) + 2^17 < 2^31 for E <= 5 900.  Inside E <= 5 900
 *                      nothing wraps and parity with libjpeg is claimed.  A file encoded from pixels has E <= 1024 + |q|_2 / 2
 *                      (Parseval on samples of -128..127, and half a step per coefficient) <= 1024 + 1020 for any 8-bit table, so
 *                      every such file lies inside.  Outside the bound only device = twin is claimed.
 *                      RANGE.  libjpeg's C code limits through a table that wraps modulo 1024 (a sample of 128 + 638 comes out 0).
 *                      Pillow's answer decides, and a hand-made 8x8 file of one DC coefficient (tests/test_mjpd_host.py) gives it:
 *                      Pillow 12 on libjpeg-turbo saturates -- 255 for samples of 287 up to 1052, 0 down to -541 -- as this code's
 *                      clamp does, and leaves it only where its 16-bit first pass overflows (|4 * dequantised value| >= 2^15, a DC
 *                      of 8192: outside E <= 5 900).  So this code clamps, parity is claimed up to there, and beyond it only
 *                      device = twin.
 *   og_jpegd_chroma    libjpeg's fancy upsampling over the component's true extent cw x ch = ceil(W / 2) x (H or ceil(H / 2)):
 *                      h2v1 (3a + b + 1) >> 2 towards the left, (3a + c + 2) >> 2 towards the right, the first and last column copied;
 *                      h2v2 s = 3 near + far vertically (edge rows replicated), then (3s + s_left + 8) >> 4 and (3s + s_right + 7) >> 4,
 *                      (4s + 8) >> 4 and (4s + 7) >> 4 at the edge columns.  As libjpeg does, a component of cw <= 2 is replicated.
 *   og_jpegd_bgr       R = Y + ((91881 Cr' + 32768) >> 16), B = Y + ((116130 Cb' + 32768) >> 16), G = Y + ((-22554 Cb' - 46802 Cr' +
 *                      32768) >> 16), Cb' = Cb - 128, Cr' = Cr - 128, clamped, stored B G R.  Gray: B = G = R = Y.
 *
 * LAUNCHES per micro-batch, each a launch boundary where one workgroup needs another's result; no workgroup waits for another inside
 * a launch and every loop is bounded by a shape or a byte count.  Before them the micro-batch's coefficients are set to 0.
 *   k_mjpd_markers  a workgroup per frame walks the scan 256 bytes at a time; a prefix over the waves' ballots numbers the RSTm, and
 *                   the k-th closes interval k and opens k + 1 (start, end per interval in the workspace; nI comes from the host).
 *                   It holds the record to its file and writes the frame's status: the host's, 6, 7, 5 or 0.
 *   k_mjpd_entropy  one LANE per restart interval, 64 lanes per workgroup: lane i of the micro-batch is interval i mod nI of frame
 *                   i / nI, so the lanes of a wave take consecutive intervals of a frame and, with nI = 1, consecutive frames.  The
 *                   table set of the workgroup's first lane lies in LDS (6120 bytes); a lane whose frame uses another set reads that
 *                   set from global memory.  A frame without DRI is one lane's work.
 *   k_mjpd_idct     8 lanes per 8x8 block: a lane per column (dequantisation, pass 1), a transpose through a padded [8][9] LDS tile,
 *                   a lane per row (pass 2, range limit); u8 component planes at the padded extent (8 bw x 8 bh per component).
 *   k_mjpd_colour   a lane per output pixel: upsampling, colour, 3 bytes; exactly H x W pixels per frame.
 * LIMITS (og_mjpd_limit): H * W <= 2^24, chunk 1..1024, a file <= 2^30 bytes.
 * MEMORY: micro-batches of nb = min(chunk, 256 MiB / per-frame workspace), at least 1.  Per frame 192 bytes per block (int16
 * coefficients and the u8 planes), 8 per interval and 4 (the marker pass's verdict).  The streamed entry adds, per micro-batch, the compressed bytes with their offsets
 * and records, nb * H * W * 3 bytes of frames unless they stay on the device, nb statuses, and two pinned slots of the same.  The
 * table sets of a call (6120 bytes each, usually one) are uploaded once.
 *
 * ALIGNMENT: offsets 8 bytes, records and status 4, table sets 4, u8 buffers any address.  A violation is OG_EINVAL before anything is
 * launched, copied or written.
 */
#ifndef OPENGLOTTAL_HIP_MJPD_H
#define OPENGLOTTAL_HIP_MJPD_H

#include "../openglottal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct og_mjpd og_mjpd;

/* What the parser reads from one file's headers; no entropy decoding.  tables: bit i = DQT id i present, bit 4 + i = DHT DC id i,
 * bit 8 + i = DHT AC id i (no DHT bit at all: the Annex K.3 tables apply).  scan_offset, scan_length: the entropy-coded bytes, from
 * the byte after SOS's segment to the marker that ends them (EOI), or to the end of a file that has none. */
typedef struct og_jpegd_info {
    int32_t H, W, ncomp, sampling;
    int32_t Ri, M, nI, tables;
    int64_t scan_offset, scan_length;
    int32_t status, reserved;
} og_jpegd_info;

/* The per-frame record of the resident entry: 8 int32.  scan_offset is counted from the frame's first byte; status is the parser's
 * (0, 6 or 7); tabset indexes the table sets given to og_mjpd_set_tables. */
typedef struct og_mjpd_rec {
    int32_t scan_offset, scan_length, status, tabset, Ri, nI, reserved0, reserved1;
} og_mjpd_rec;

/* which: 0 max H * W, 1 max chunk, 2 bytes of a record, 3 bytes of a table set, 4 the highest status code, 5 max bytes of one file,
 * 6 the default chunk; otherwise -1 */
long long og_mjpd_limit(int which);

/* Host only, no handle, no device. */

/* Always fills *info (status 0 or 6); returns OG_OK unless an argument is bad.  The reason of a refusal is in og_last_error. */
int og_jpegd_parse_host(const uint8_t* jpeg, size_t size, og_jpegd_info* info);

/* The twin: one file -> out [H,W,3] u8 BGR, cap >= H * W * 3 or OG_EINVAL and nothing is written; *status as above. */
int og_jpegd_decode_host(const uint8_t* jpeg, size_t size, uint8_t* out_bgr, size_t cap, int* status);

/* One pass of og_jpegd_idct8 over 8 values, as the twin and k_mjpd_idct run it: shift 11 (columns) or 18 (rows), no + 128, no clamp.
 * For tests that hold the BOUND paragraph to the code. */
int og_jpegd_idct_pass_host(const int32_t* in8, int shift, int32_t* out8);

/* Parses B files (file i = blob[offsets[i], offsets[i + 1])) for the resident entry: recs [B]; the distinct table sets, og_mjpd_limit(3)
 * bytes each, into tabs (room for tabs_cap sets; OG_EINVAL if there are more; B always suffices); *nsets their count.  *H, *W,
 * *sampling, *Ri: the form of the first file the parser accepts (0, 0, -1, 0 if none); files of another form get status 7. */
int og_jpegd_records_host(const uint8_t* blob, const int64_t* offsets, int B, og_mjpd_rec* recs, uint8_t* tabs, int tabs_cap, int* nsets,
                          int* H, int* W, int* sampling, int* Ri);

/* The device is the one current at the first call that touches it; the handle owns its stream and workspace.  chunk 128. */
og_mjpd* og_mjpd_create(void);
void og_mjpd_destroy(og_mjpd* h);
int og_mjpd_sync(og_mjpd* h);
int og_mjpd_set_chunk(og_mjpd* h, int chunk);

/* The table sets (from og_jpegd_records_host) and the form of the og_mjpd_decode_u8_dev calls that follow; copied to the device before
 * the call returns.  og_mjpd_decode_stream replaces them. */
int og_mjpd_set_tables(og_mjpd* h, const uint8_t* tabs, int nsets, int sampling, int Ri);

/* Everything resident: blob_dev the files, offsets_dev [B + 1] int64 into it, recs_dev [B] og_mjpd_rec, frames_dev [B,H,W,3] u8 BGR
 * with cap >= B * H * W * 3 or OG_EINVAL before anything runs, status_dev [B] int32.  Reads nothing outside
 * blob_dev[offsets[0], offsets[B]); writes exactly B * H * W * 3 bytes of frames and B statuses.  Asynchronous on the handle's stream. */
int og_mjpd_decode_u8_dev(og_mjpd* h, const uint8_t* blob_dev, const int64_t* offsets_dev, const og_mjpd_rec* recs_dev, int B, int H, int W,
                          uint8_t* frames_dev, size_t cap, int32_t* status_dev);

/* Host bytes in: parses them, uploads the COMPRESSED bytes micro-batch by micro-batch through the two pinned slots, and delivers the
 * frames to frames_out_host, to frames_out_dev (they never visit the host), or both; cap counts either.  status [B] on the host; *H, *W
 * the size found (the form is the first accepted file's).  cap < B * H * W * 3 is OG_EINVAL before anything runs.  Synchronous.  On an
 * error everything in flight is waited for and the handle stays usable. */
int og_mjpd_decode_stream(og_mjpd* h, const uint8_t* blob, const int64_t* offsets, int B, uint8_t* frames_out_host_or_null,
                          uint8_t* frames_out_dev_or_null, size_t cap, int32_t* status, int* H, int* W);

/* Dry run of og_mjpd_decode_stream of B frames of one form with cap = B * H * W * 3, without a device: one line per launch in the
 * columns of og_mjpeg_plan, kernel|gx|gy|gz|block|lds|workspace|counters|writes ("frames=END;status=END" or "-").  Returns the number
 * of launches; *workspace_bytes = the device workspace of the call apart from the compressed bytes, whose size no shape tells. */
int og_mjpd_plan(int B, int H, int W, int sampling, int Ri, int chunk, char* out, size_t cap, long long* workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
