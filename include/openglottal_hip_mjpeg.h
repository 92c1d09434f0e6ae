/*
 * openglottal_hip_mjpeg.h — baseline JPEG on the device (ninth header; the conventions of openglottal_hip.h -- return codes,
 * og_last_error, *_dev entry points asynchronous on the handle's stream, device restore, a failed call leaves the handle usable -- all
 * hold): the frames k_overlay leaves on the device (openglottal_hip_overlay.h) become complete JPEG files there, so that an annotated
 * video leaves the device compressed, as the chunks of a Motion-JPEG AVI (scripts/infer.py:274-275 writes cv2's "MJPG").  No network
 * is involved, so the family has a handle of its own.  Parity with OpenCV's own MJPG writer is UNPINNED, as every cv2 row of this
 * project; the judges are Pillow's libjpeg decoder and encoder and a bit-exact scan decoder in the tests.
 *
 * FORMAT.  Sequential baseline DCT (SOF0), 8 bit, three components, JFIF YCbCr full range, 4:4:4 (every sampling factor 1): one MCU
 * is three 8x8 blocks in the order Y, Cb, Cr; MCUs run left to right, top to bottom.
 *   source     [B,H,W,3] u8 BGR.  A frame whose sides are no multiples of 8 is padded by repeating its last column and row; SOF0
 *              carries the true H and W.
 *   file       SOI, APP0 (JFIF 1.01, no density, no thumbnail), DQT luminance (id 0), DQT chrominance (id 1), SOF0, DHT DC 0, DHT AC 0,
 *              DHT DC 1, DHT AC 1, DRI, SOS, the scan, EOI.  SOI through SOS is og_mjpeg_limit(6) = 629 bytes for every (H, W, quality).
 *   DQT        the two base tables of ITU T.81 Annex K.1 scaled by the IJG quality rule: s = 5000 / q below 50, else 200 - 2q; entry =
 *              clamp((base * s + 50) / 100, 1, 255), integer division; quality 1..100, default 75.
 *   DHT        the four tables of Annex K.3.
 *   DRI        Ri = og_mjpeg_limit(1) = 16 MCUs.  Every Ri MCUs the scan is padded with 1-bits to a byte, RSTm follows (m counts the
 *              intervals of the frame modulo 8) and the three DC predictors return to 0; the last interval is followed by EOI instead.
 *              An interval depends on nothing outside it, which is what lets one workgroup code it.  A block is at most 63 * 26 + 22
 *              = 1660 bits, 208 bytes, before byte stuffing (0xFF -> 0xFF 0x00) and 416 after: an interval of 48 blocks with its
 *              marker fits a slot of og_mjpeg_limit(5) = 19972 bytes, and the kernel's 38 KB of LDS.
 *
 * ARITHMETIC, integer only; three inline functions of csrc/og_mjpeg.inc that og_jpeg_*_host and the kernels both call.  `>>` is the
 * arithmetic shift (floor), so (x + half) >> n rounds half up.
 *   og_jpeg_ycc      16-bit constants (Y 19595 38470 7471; Cb -11059 -21709 32768; Cr 32768 -27439 -5329, on R G B), result kept
 *                    with 4 fraction bits and level shifted: (sum + 2^11) >> 12, minus 2048 for Y (Cb, Cr: the +128 and the -128
 *                    cancel).  |result| <= 2048.
 *   og_jpeg_fdct8x8  out(v,u) = sum b(v,y) b(u,x) in(y,x), b(u,x) = C(u)/2 cos((2x+1) u pi / 16), by two passes of og_jpeg_dct8 with
 *                    b rounded to 14 fraction bits (|b| 2^14 <= 8035, row sums of |.| <= 2.83 * 2^14).  Pass 1 (rows): |acc| <=
 *                    2.83 * 2^14 * 2048 < 2^27, kept as (acc + 2^11) >> 12: 6 fraction bits, |.| <= 362.04 * 64 < 23171 + 2.  Pass 2
 *                    (columns): |acc| <= 2.83 * 2^14 * 23173 < 2^31, kept as (acc + 2^15) >> 16: the coefficient with 4 fraction
 *                    bits, |.| <= 1024 * 16 + 8.
 *   og_jpeg_quant    sign(c) * ((|c| + 8q) / (16q)): round half away from zero, sign-symmetric.  AC results are clamped to +-1023
 *                    (the column pattern sign(cos((2x+1) 4 pi / 16)) at the u8 extremes reaches 1024; category 11 does not exist
 *                    for AC in baseline); DC lies in [-1024, 1016] and its difference in +-2040, category 11 at most.
 *   ERROR BOUND against the exact transform of the exact JFIF matrix, in coefficient units: samples are off by at most e_s = 1/32 +
 *   255 * (sum of the three constants' rounding errors) / 65536 <= 0.0369, which the transform amplifies by at most A^2 = 8 (A = the
 *   largest row sum of |b|, 2.83); pass 1 is off by (8 * 0.5 * 2048 / 2^12 + 0.5) / 64 = 0.0391, amplified by A; pass 2 adds
 *   8 * 0.5 * 23173 / 2^20 = 0.0884 and the last rounding 1/32.  Sum: E = 8 e_s + 2.83 * 0.0391 + 0.0884 + 0.0313 <= 0.53.  A quantised
 *   value equals the exact one wherever the exact quotient is farther than E / q from a half-integer, and is never more than 1 away.
 *
 * LAUNCHES per micro-batch, each a launch boundary where one workgroup needs another's result; no workgroup waits for another inside
 * a launch and every loop is bounded by a shape:
 *   k_mjpeg_transform  8 lanes per 8x8 pixel block (a lane per row, then per column; the transpose goes through a padded LDS tile):
 *                      BGR -> YCbCr, DCT, quantisation, zigzag; int16 coefficients [frame][MCU][Y,Cb,Cr][64] in the workspace.
 *   k_mjpeg_entropy    one wave per restart interval: a lane per block counts its bits, a prefix sum places it, the codes are OR-ed
 *                      into the interval's bit string in LDS, a second prefix sum over the 0xFF bytes places the stuffed bytes, then
 *                      padding and RSTm; the interval's bytes go to its slot and its length to the workspace.
 *   k_mjpeg_offsets    one workgroup: the prefix sum over the micro-batch's intervals and frames; sizes and the running total.
 *   k_mjpeg_place      a workgroup per interval copies it to its place in the caller's buffer; the first of a frame adds the header,
 *                      the last EOI.  Frames are dense: frame i starts where frame i - 1 ends.
 * LIMITS (og_mjpeg_limit): H * W <= 2^24 pixels, H and W <= 65535 each (SOF0's fields); chunk 1..1024; quality 1..100.
 * MEMORY: frames are processed in micro-batches of nb = min(chunk, 256 MiB / per-frame workspace), at least 1, frames.  The handle's
 * device workspace is that of ONE micro-batch, independent of B: per frame M * 384 bytes of coefficients (M MCUs) and nI * (19972 + 12)
 * bytes of slots, lengths and offsets (nI = ceil(M / 16) intervals); for the streamed entry nb * (H * W * 3 + og_jpeg_bound + 4) + 8
 * bytes more (frames, files, sizes, total) and two pinned slots that hold the frames and the bytes actually produced.
 * The host learns ONE number per micro-batch, its total bytes, through one event wait (streamed entry); the resident entry learns none.
 *
 * ALIGNMENT: sizes 4 bytes, total 8, int16 coefficients 2, u8 buffers (frames, out, tables, header) any address.  A violation is
 * OG_EINVAL before anything is launched, copied or written.
 */
#ifndef OPENGLOTTAL_HIP_MJPEG_H
#define OPENGLOTTAL_HIP_MJPEG_H

#include "openglottal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct og_mjpeg og_mjpeg;

/* which: 0 max H * W, 1 Ri (MCUs per restart interval), 2 max chunk, 3 lowest quality, 4 highest quality, 5 bytes of an interval's
 * slot, 6 bytes of a file's headers (SOI through SOS), 7 the default quality; otherwise -1 */
long long og_mjpeg_limit(int which);

/* Worst-case bytes of one frame's file: headers + 1248 per MCU + 2 per interval + EOI.  -1 (and og_last_error) on a bad H or W. */
long long og_jpeg_bound(int H, int W);

/* Host only, no handle, no device: the same inline functions the kernels call. */

/* qlum64, qchroma64: the two quantisation tables in natural (row-major) order, 64 bytes each.  header_or_null: SOI through SOS of a
 * frame of H x W, header_cap >= og_mjpeg_limit(6) bytes; *header_len_or_null = their count. */
int og_jpeg_tables_host(int quality, int H, int W, uint8_t* qlum64, uint8_t* qchroma64, uint8_t* header_or_null, size_t header_cap,
                        int* header_len_or_null);

/* frame [H,W,3] u8 BGR -> out int16 [M][3][64]: the quantised coefficients of every block in scan order, each block in zigzag order. */
int og_jpeg_coefficients_host(const uint8_t* frame, int H, int W, int quality, int16_t* out);

/* One complete file into out; cap >= og_jpeg_bound(H, W), else OG_EINVAL and nothing is written; *size = its bytes. */
int og_jpeg_encode_host(const uint8_t* frame, int H, int W, int quality, uint8_t* out, size_t cap, int* size);

/* The device is the one current at the first call that touches it; the handle owns its stream and workspace.  chunk 128, quality 75. */
og_mjpeg* og_mjpeg_create(void);
void og_mjpeg_destroy(og_mjpeg* h);
int og_mjpeg_sync(og_mjpeg* h);
int og_mjpeg_set_chunk(og_mjpeg* h, int chunk);
int og_mjpeg_set_quality(og_mjpeg* h, int quality);

/* Everything resident on the device: frames_dev [B,H,W,3] u8 BGR; out_dev cap bytes, cap >= B * og_jpeg_bound(H, W) or OG_EINVAL
 * before anything runs; sizes_dev [B] int32; total_dev one int64.  The B files lie back to back from out_dev[0]; file i has
 * sizes_dev[i] bytes; *total_dev is their sum, and nothing at or past out_dev[*total_dev] is written.  Asynchronous on the handle's
 * stream. */
int og_mjpeg_encode_u8_dev(og_mjpeg* h, const uint8_t* frames_dev, int B, int H, int W, uint8_t* out_dev, size_t cap, int32_t* sizes_dev,
                           long long* total_dev);

/* Host in, host out, micro-batch by micro-batch through the two pinned slots; only the bytes used come back from the device.  The same
 * layout and the same cap rule.  Synchronous.  On an error everything in flight is waited for and the handle stays usable. */
int og_mjpeg_encode_stream_u8(og_mjpeg* h, const uint8_t* frames, int B, int H, int W, uint8_t* out, size_t cap, int32_t* sizes,
                              long long* total);

/* Dry run of og_mjpeg_encode_stream_u8 with cap = B * og_jpeg_bound(H, W), without a device: one line per launch in the columns of
 * og_overlay_plan, kernel|gx|gy|gz|block|lds|workspace|counters|writes ("out=END;sizes=END;total=END": bytes from the start of the
 * caller's buffer to the end of what the launch may write, or "-").  Returns the number of launches; *workspace_bytes = the device
 * workspace of the call. */
int og_mjpeg_plan(int B, int H, int W, int chunk, char* out, size_t cap, long long* workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
