/*
 * openglottal_hip_pnge.h — PNG files ENCODED on the device (thirteenth header; the conventions of openglottal_hip.h -- return codes,
 * og_last_error, *_dev entry points asynchronous on the handle's stream, device restore, a failed call leaves the handle usable -- all
 * hold, and the entries mirror the ninth header, include/openglottal_hip_mjpeg.h).  include/ and include_ext/ are closed by directory
 * listings in older tests, so this header opens include_enc/; no test pins this directory's listing, the next header may join it.
 * What `cli infer --frames png` writes through Pillow and what the reference's crop trainer writes through cv2.imwrite: the frames
 * k_overlay or k_crop_tiles leave on the device become complete PNG files there.  PNG is lossless, so the judges are exact: Pillow and
 * this project's own decoder for the pixels, zlib for the stream.  Parity of the BYTES with cv2.imwrite's is UNPINNED, as every cv2 row
 * of this project; the pixels are the same by construction.
 *
 * ACCEPTED.  One shape per call: frames [B,H,W,C] u8.  C = 1: colour type 0 (gray), depth 8.  C = 3: stored B G R, written as colour
 * type 2 (R G B), depth 8.  H * W <= og_pnge_limit(0) = og_png_limit(0).
 * OUT OF SCOPE: palette output, alpha, 16-bit samples, Adam7 interlace, mixed shapes in one call, LZ77 matches beyond distance 1.
 *
 * THE ARITHMETIC is integer only; inline functions of csrc/og_pnge.inc that og_pnge_*_host and the kernels both call.
 *   FILTER (og_pnge_filt, og_pnge_cost).  rb = W * C bytes per scanline, bpp = C.  Per row the type among 0 None, 1 Sub, 2 Up,
 *     3 Average, 4 Paeth (the predictors of og_png_recon) with the least sum over the row of |filtered byte read as int8|; ties go to
 *     the lower type.  A row depends only on the unfiltered row above it, so rows are independent.  The raw stream is H rows of
 *     1 + rb bytes, N = H * (1 + rb).
 *   SEGMENTS.  The raw stream is cut into segments of S bytes, the last one short: nseg = ceil(N / S).  S is a power of two,
 *     64 <= S <= 32768 (default 32768), settable per handle and per twin call.  A segment is compressed with no knowledge of its
 *     neighbours.
 *   TOKENS (og_pnge_run; zlib's Z_RLE parse in closed form).  Inside a segment a run is a maximal stretch of equal bytes.  Its first
 *     byte is a literal.  Of the remaining R bytes: R / 258 matches of length 258 at distance 1, then, with r = R mod 258, one match of
 *     length r if r >= 3, else r literals.  Runs are independent of each other.
 *   CODE (og_pnge_rank, og_pnge_build).  One dynamic block per segment.  The lit/len histogram counts the tokens and one end-of-block
 *     (256).  The used symbols are ordered by (count, symbol) ascending.  A Huffman tree is built by the two-queue method: leaves in
 *     that order, internal nodes in the order they are made; of two nodes of equal weight the LEAF is taken first, and of two leaves or
 *     two internal nodes the earlier.  Only the NUMBER of leaves per depth is kept.  LIMITER: depths above 15 count as 15; while the
 *     Kraft sum (in units of 2^-15) exceeds 2^15, one code of length 15 is removed, and the longest length l < 15 that has a code gives
 *     one up: that code and the removed one become two codes of length l + 1 -- the sum falls by exactly one unit per turn, at most
 *     286 turns, and ends at exactly 2^15: the set is always Kraft-complete (a non-empty segment has at least two symbols, a literal and
 *     256).  The lengths are then dealt out longest first to the symbols in ascending (count, symbol) order, and the codes are the
 *     canonical ones of RFC 1951 3.2.2.  The distance set is one code: symbol 0, length 1.
 *   BLOCK HEADER (og_pnge_code, og_pnge_hdr_put).  BFINAL, BTYPE = 2, HLIT = max(257, highest used symbol + 1) - 257, HDIST = 0.  The
 *     HLIT + 257 lit/len lengths and the one distance length form one sequence, cut into maximal stretches of one value v, r long.
 *     v = 0: while r >= 11 a code 18 for min(r, 138); then, if r >= 3, one code 17 for r; what is left (r < 3) as zeros.  v > 0: v
 *     once; then while r >= 3 a code 16 for min(r, 6); what is left (r < 3) as v.  The code-length code is the same construction over
 *     the symbols 0..18 of that sequence with the limit 7 (if the sequence used one symbol only, symbol 0 -- or 1 -- joins with count
 *     1), HCLEN trimmed to the last used entry of RFC 1951's order.  The form costs more code than 4 bits a length, and was taken
 *     because the flat form made a 256 x 256 mask 2.5 times zlib's size: three segments of 153 header bytes around 90 bytes of runs.
 *   STORED.  If the dynamic block with its closing alignment is not smaller than the stored block of 5 + n bytes, the segment is
 *     stored: noise does not grow.
 *   JOINING.  Every segment starts on a byte.  A non-final dynamic segment that ends off the byte grid is closed by an empty stored
 *     block (three zero bits, zero padding to the byte, 00 00 FF FF: a sync flush); the final segment carries BFINAL and zero padding.
 *     Around the segments: the zlib header 78 01 and the Adler-32 of the raw stream (og_png_adler_part / og_png_adler_join).
 *   FILE.  Signature, IHDR, ONE IDAT, IEND; 57 fixed bytes around the zlib stream.  The CRC-32 of every chunk is computed on the
 *     device: a piece's CRC (og_pnge_crc) from the CRCs of its parts by crc(A B) = og_pnge_crc_shift(crc(A), |B|) ^ crc(B), the shift
 *     being the multiplication by x^(8 |B|) modulo the CRC polynomial.
 *   BOUND.  og_pnge_bound(H, W, C, S) = 57 + 2 + 4 + N + 5 * nseg: every segment stored (5 bytes of header each), the zlib header and
 *     trailer, the fixed bytes.  A dynamic segment is only chosen when it is smaller, so no file exceeds it.
 *
 * LAUNCHES per micro-batch, each a launch boundary where one group needs another's result; no workgroup waits for another inside a
 * launch and every loop is bounded by a shape or a byte count.
 *   k_pnge_filter   a wave per row: the five costs, the choice, the row's 1 + rb raw bytes into the workspace, its Adler-32 partial sums.
 *   k_pnge_segment  a workgroup of 1024 per (file, segment): the segment, the run starts (a suffix-minimum scan over the threads'
 *                   stretches), the histogram, the code and the emitted bits all in LDS (og_pnge_limit(7) bytes: two workgroups per CU);
 *                   the segment's bytes, their count and their CRC-32 go to its slot.
 *   k_pnge_offsets  one workgroup, a thread per file: the segments' places in the file, the IDAT CRC and the Adler-32 joined, the
 *                   sizes; then the prefix sum over the files and the running total.
 *   k_pnge_place    a workgroup per (file, segment) copies the slot to its place in the caller's buffer; the first of a file adds the
 *                   signature, IHDR and the IDAT header, the last the Adler-32, the IDAT CRC and IEND.  Files are dense.
 *   k_label_bbox    (og_pnge_label_bbox_u8_dev only) a workgroup per label: min and max of x and y over label > 0.
 * LIMITS (og_pnge_limit): H * W <= 2^24, chunk 1..1024, S 64..32768.
 * MEMORY: micro-batches of nb = min(chunk, 256 MiB / per-frame workspace), at least 1, frames.  Workspace per frame: N raw bytes
 * (rounded to 16), nseg slots of S + 16 bytes, 12 bytes per segment, 8 per row, 24 per frame.  The streamed entry adds nb * (H * W * C +
 * bound + 4) + 8 bytes and two pinned slots that hold the frames and the bytes actually produced.
 *
 * ALIGNMENT: sizes 4 bytes, total 8, u8 buffers any address.  A violation is OG_EINVAL before anything is launched, copied or written.
 */
#ifndef OPENGLOTTAL_HIP_PNGE_H
#define OPENGLOTTAL_HIP_PNGE_H

#include "../include_ext/openglottal_hip_png.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct og_pnge og_pnge;

/* which: 0 max H * W, 1 max chunk, 2 smallest S, 3 largest S, 4 the default S, 5 the default chunk, 6 the fixed bytes of a file around
 * its zlib stream (57), 7 bytes of LDS of k_pnge_segment; otherwise -1 */
long long og_pnge_limit(int which);

/* Worst-case bytes of one file (see BOUND).  -1 (and og_last_error) on a bad H, W, C or S. */
long long og_pnge_bound(int H, int W, int C, int S);

/* Host only, no handle, no device: the same inline functions the kernels call. */

/* frame [H,W,C] u8 -> the raw stream, H * (1 + W * C) bytes; cap at least that or OG_EINVAL and nothing is written. */
int og_pnge_filter_host(const uint8_t* frame, int H, int W, int C, uint8_t* out, size_t cap);

/* n >= 1 raw bytes -> one zlib stream cut at S; cap >= 6 + n + 5 * ceil(n / S) or OG_EINVAL and nothing is written; *size its bytes. */
int og_pnge_deflate_host(const uint8_t* raw, size_t n, int S, uint8_t* out, size_t cap, size_t* size);

/* The twin: one complete file into out; cap >= og_pnge_bound(H, W, C, S), else OG_EINVAL and nothing is written; *size = its bytes. */
int og_pnge_encode_host(const uint8_t* frame, int H, int W, int C, int S, uint8_t* out, size_t cap, int* size);

/* The device is the one current at the first call that touches it; the handle owns its stream and workspace.  chunk 128, S 32768. */
og_pnge* og_pnge_create(void);
void og_pnge_destroy(og_pnge* h);
int og_pnge_sync(og_pnge* h);
int og_pnge_set_chunk(og_pnge* h, int chunk);
int og_pnge_set_segment(og_pnge* h, int S);

/* Everything resident on the device: frames_dev [B,H,W,C] u8; out_dev cap bytes, cap >= B * og_pnge_bound(H, W, C, S) or OG_EINVAL
 * before anything runs; sizes_dev [B] int32; total_dev one int64.  The B files lie back to back from out_dev[0]; file i has
 * sizes_dev[i] bytes; *total_dev is their sum, and nothing at or past out_dev[*total_dev] is written.  Asynchronous on the handle's
 * stream. */
int og_pnge_encode_u8_dev(og_pnge* h, const uint8_t* frames_dev, int B, int H, int W, int C, uint8_t* out_dev, size_t cap,
                          int32_t* sizes_dev, long long* total_dev);

/* Host in, host out, micro-batch by micro-batch through the two pinned slots; only the bytes used come back from the device.  The same
 * layout and the same cap rule.  Synchronous.  On an error everything in flight is waited for and the handle stays usable. */
int og_pnge_encode_stream_u8(og_pnge* h, const uint8_t* frames, int B, int H, int W, int C, uint8_t* out, size_t cap, int32_t* sizes,
                             long long* total);

/* THE CROP-TRAINING CACHE (openglottal_amd/cropcache.py) needs two more things on the handle's stream, both asynchronous.
 * og_pnge_label_bbox_*: the tight box of label > 0 of B labels [H,W] u8 as x0 y0 x1 + 1 y1 + 1 (int32 [B][4]); 0 0 0 0 for a label
 * without such a pixel.  k_label_bbox, a workgroup per label; the host twin is the same rule in two loops.
 * og_pnge_crop_tiles_u8_dev: the tiles alone -- k_crop_tiles of openglottal_hip_crops.h (og_crop_tile_host is its twin) without the
 * network behind it: frames_dev [B,H,W,channels] u8, boxes_dev [B][4] int32 x1 y1 x2 y2, tiles_dev [B,size,size] u8; an unusable box
 * gives an all-zero tile.  The tiles can go straight into og_pnge_encode_u8_dev of the same handle. */
int og_pnge_label_bbox_host(const uint8_t* label, int H, int W, int32_t* box4);
int og_pnge_label_bbox_u8_dev(og_pnge* h, const uint8_t* labels_dev, int B, int H, int W, int32_t* boxes_dev);
int og_pnge_crop_tiles_u8_dev(og_pnge* h, const uint8_t* frames_dev, int B, int H, int W, int channels, const int32_t* boxes_dev, int size,
                              uint8_t* tiles_dev);

/* Dry run of og_pnge_encode_stream_u8 with cap = B * og_pnge_bound(H, W, C, S), without a device: one line per launch in the columns
 * of og_mjpeg_plan, kernel|gx|gy|gz|block|lds|workspace|counters|writes ("out=END;sizes=END;total=END": bytes from the start of the
 * caller's buffer to the end of what the launch may write, or "-").  Returns the number of launches; *workspace_bytes = the device
 * workspace of the call. */
int og_pnge_plan(int B, int H, int W, int C, int S, int chunk, char* out, size_t cap, long long* workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
