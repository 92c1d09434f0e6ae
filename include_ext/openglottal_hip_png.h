/*
 * openglottal_hip_png.h — PNG files decoded on the device (twelfth header; the conventions of openglottal_hip.h -- return codes,
 * og_last_error, *_dev entry points asynchronous on the handle's stream, device restore, a failed call leaves the handle usable -- all
 * hold, and the layout follows the tenth header, include/decode/openglottal_hip_mjpd.h).  The listing of include/ is pinned by older
 * tests, so this header and every later one live in include_ext/.  What scripts/eval_bagls.py, eval_girafe.py, sweep_bagls_conf.py
 * and `infer.py --mode images` read through OpenCV: the files go up COMPRESSED and become [H,W,C] u8 pixels on the device, C = 3
 * (B G R) or 1 (gray).  PNG is lossless, so the judges are exact: zlib for the inflated bytes, Pillow's convert("RGB") / ("L") for the
 * pixels.  Parity with cv2.imread's IMREAD_GRAYSCALE of a colour file is UNPINNED, as every cv2 row of this project.
 *
 * ACCEPTED (og_pngd_parse_host).  The 8-byte signature; IHDR first, length 13; compression 0, filter method 0, interlace 0; colour
 * type and depth one of gray (0) at 1, 2, 4, 8; palette (3) at 1, 2, 4, 8; RGB (2) at 8; gray+alpha (4) at 8; RGBA (6) at 8.  PLTE
 * before the first IDAT for palette files, length 3 n, 1 <= n <= 256.  At least one IDAT; the payloads of the consecutive IDAT chunks
 * form one zlib stream.  The CRC-32 of every chunk up to the last IDAT is verified.  tRNS, gAMA, sRGB, iCCP, text and every other
 * ancillary chunk are skipped (Pillow's convert("RGB") ignores them too); nothing after the last IDAT is required.
 * REFUSED with status 6 and the reason in og_last_error, never decoded approximately: a bad signature; 16-bit samples; Adam7
 * interlace; any other (type, depth); a bad CRC; a chunk that leaves the file before the IDAT run has ended; an unknown critical
 * chunk before it; a missing, second or malformed PLTE; no IDAT; H or W of 0; H * W above og_png_limit(0) = og_mjpd_limit(0); a
 * file above og_png_limit(5) = 2^30 bytes.
 *
 * FILES OF ONE CALL MAY DIFFER IN SIZE AND FORM: there is no "form of the call".  A record (og_png_rec) carries H, W, type, depth, a
 * palette index and two int64 offsets; file i's pixels are written densely at out + out_offset as [H,W,C] u8, C the call's.
 * The device sees one zlib stream per file (the host joins the IDAT payloads) and never a chunk header.  The distinct palettes of a
 * call, 768 bytes each (R G B per entry, zero beyond PLTE's n), go up once as table sets.
 *
 * PIXELS.  rb = ceil(W * samples * depth / 8) bytes per scanline, bpp = max(1, samples * depth / 8).  The raw data is H rows of
 * 1 + rb bytes.  Filter types 0..4: None, Sub, Up, Average ((a + b) >> 1), Paeth (p = a + b - c; the nearest of a, b, c, ties in
 * that order); the row above row 0 and the bytes left of a row are 0.  Depths 1, 2, 4 unpack MSB first; gray samples scale by 255,
 * 85, 17.  A palette index beyond PLTE gives (0, 0, 0), as Pillow does.  Alpha is dropped.  C = 3 stores B G R.  C = 1 stores the
 * sample of a gray or gray+alpha file and og_gray_at's (3735 B + 19235 G + 9798 R + 2^14) >> 15 of a colour or palette file:
 * bgr_to_gray of the C = 3 result.
 *
 * INFLATE: RFC 1950 and RFC 1951 in full -- stored, fixed and dynamic blocks; HLIT 257..286, HDIST 1..30, HCLEN 4..19; code lengths
 * up to 15 with the repeat codes 16, 17, 18; length codes 257..285, distance codes 0..29; distances up to 32 768; matches that
 * overlap their own output.  zlib's rule for code sets: an over-subscribed set is invalid; an incomplete one is invalid except a
 * single distance code of length 1, and except an all-zero distance set (then any distance code is "no code").  All of it is inline
 * functions of csrc/og_png.inc that og_pngd_inflate_host, og_pngd_decode_host and the kernels call: og_inf_fill / og_inf_take (a
 * 64-bit LSB-first bit buffer), og_inf_build (canonical counts and symbols), og_inf_sym (the canonical walk, 1..15 bits),
 * og_png_zlib<LANES> (the stream), og_png_adler_part / og_png_adler_join, og_png_recon (one byte of a filter), og_png_pixel.
 * SAFETY.  og_png_zlib reads in[i] only for i < length (the fill loop's condition) and writes out[j] only for j < cap = H * (1 + rb):
 * a literal is stored behind `pos < cap`, a match and a stored block behind `pos + len <= cap`.  The window is a 32 KiB ring indexed
 * `& 32767`; a distance is checked against pos before the ring is read.  Every turn of every loop consumes at least one input bit
 * or produces at least one output byte (the table builders loop over at most 320 symbols and 15 lengths), so the decoder runs at most
 * 8 * length + H * (1 + rb) turns.  On an error it returns the status at once.
 *
 * STATUS per file (int32): 0 ok, or
 *   1 truncated: the bytes ended before the final block's end-of-block or before the 4-byte trailer, or the stream ended with fewer
 *     than H * (1 + rb) bytes;
 *   2 invalid deflate data: block type 3, LEN != ~NLEN, HLIT above 286 or HDIST above 30, a bad code-length set, bits that are no
 *     code, litlen symbol 286 / 287, distance symbol 30 / 31, a repeat with nothing to repeat or past HLIT + HDIST, no end-of-block code;
 *   3 a distance that reaches before the first output byte;
 *   4 output past H * (1 + rb) bytes;
 *   5 zlib wrapper: CM != 8, CINFO > 7, header no multiple of 31, FDICT set, or Adler-32 mismatch;
 *   6 the parser's refusal (also a record whose extents leave the buffers of the call or whose palette does not exist);
 *   7 a filter-type byte above 4.
 * Order when several apply: 6; 5 for the header; the first of 1..4 in stream order (for one match 3 before 4; a stored block that
 * both runs out of input and leaves the output is 1 when the input ends first or at the same byte); 5 for Adler; 7.  Adler-32 is
 * computed on the device over the raw bytes.  A file with a non-zero status has every output byte 0 and never stops its
 * neighbours; the call returns OG_OK.  A refused file (6 from the parser) has no size: it takes no output bytes.  The twin is
 * stricter than Pillow on purpose (Pillow pads a short stream with zero rows and ignores surplus bytes), so against Pillow only
 * "status 0 => the same bytes" is claimed.
 *
 * LAUNCHES per micro-batch, each a launch boundary where one group needs another's result; no workgroup waits for another inside a
 * launch and every loop is bounded by a shape or a byte count.
 *   k_png_inflate   one WAVE (a workgroup of 64) per file.  Bit buffer, position and code tables are wave-uniform; the tables and the
 *                   32 KiB window lie in LDS (33 824 bytes per wave: four files per CU); a literal is stored by lane 0, a match
 *                   and a stored block are copied by all 64 lanes, src = pos - dist + (i mod dist) for i < len: at most five turns.
 *                   It writes the file's raw bytes into the workspace and never reads them back.
 *   k_png_unfilter  one wave per file, in place.  First Adler-32 over the raw bytes (64 strided partial sums), then the filter-type
 *                   bytes, then bands of 64 rows: lane r on row r of the band, one byte-step behind lane r - 1; "up" comes by a wave
 *                   shuffle, "left" and "up-left" from two register queues of bpp values; no LDS, no barrier inside a band.  The
 *                   bands of a file go in sequence, the last row carried through memory behind a workgroup fence.
 *                   ceil(H / 64) * (rb + 63) steps per file.
 *   k_png_expand    a lane per output pixel: unpack, palette, alpha dropped, B G R or gray; exactly H * W * C bytes per file whose
 *                   record is sound, zeros for a file with a non-zero status.
 * LIMITS (og_png_limit): H * W <= 2^24, chunk 1..1024, a file <= 2^30 bytes, at most 65 535 palettes per call.
 * MEMORY: a micro-batch is at most `chunk` files and, when it holds more than one file, at most 256 MiB of raw bytes.  Workspace:
 * the raw bytes, 4 per file (the stored Adler-32).  The streamed entry adds the zlib bytes with their offsets and records, the
 * pixels unless they stay in the caller's device buffer, the statuses, and two pinned slots of the same.
 *
 * ALIGNMENT: offsets and records 8 bytes, status and sizes 4, u8 buffers any address.  A violation is OG_EINVAL before anything is
 * launched, copied or written.
 */
#ifndef OPENGLOTTAL_HIP_PNG_H
#define OPENGLOTTAL_HIP_PNG_H

#include "../include/openglottal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct og_png og_png;

/* What the parser reads from one file; nothing is inflated.  samples: per pixel (1 2 3 4); zlib_bytes: the joined IDAT payloads. */
typedef struct og_png_info {
    int32_t H, W, ctype, depth, samples, rb, bpp, npal, nidat, status;
    int64_t raw_bytes, zlib_bytes;
} og_png_info;

/* The per-file record of the resident entry: 40 bytes.  status is the parser's (0 or 6); palette indexes the sets given to
 * og_png_set_palettes (ignored unless ctype is 3); out_offset: first byte of the file's pixels in the output; raw_offset: first
 * byte of its H * (1 + rb) raw bytes in the workspace. */
typedef struct og_png_rec {
    int32_t H, W, ctype, depth, palette, status;
    int64_t out_offset, raw_offset;
} og_png_rec;

/* which: 0 max H * W, 1 max chunk, 2 bytes of a record, 3 bytes of a palette, 4 the highest status code, 5 max bytes of one file,
 * 6 the default chunk, 7 bytes of the inflate window; otherwise -1 */
long long og_png_limit(int which);

/* Host only, no handle, no device. */

/* Always fills *info (status 0 or 6); returns OG_OK unless an argument is bad.  The reason of a refusal is in og_last_error. */
int og_pngd_parse_host(const uint8_t* png, size_t size, og_png_info* info);

/* One zlib stream (no PNG around it) -> out; *produced bytes were written (never more than cap); *status 0, 1, 2, 3, 4 or 5. */
int og_pngd_inflate_host(const uint8_t* zlib_stream, size_t size, uint8_t* out, size_t cap, size_t* produced, int* status);

/* The twin: one file -> out [H,W,channels] u8, channels 3 or 1, cap >= H * W * channels or OG_EINVAL and nothing is written. */
int og_pngd_decode_host(const uint8_t* png, size_t size, int channels, uint8_t* out, size_t cap, int* status);

/* Parses B files (file i = blob[offsets[i], offsets[i + 1])) for the resident entry: recs [B] with dense offsets in file order;
 * the joined zlib streams into zblob (zcap bytes; OG_EINVAL if they do not fit; the files' total size always suffices) with
 * zoffsets [B + 1]; the distinct palettes, 768 bytes each, into pals (room for pals_cap; B always suffices); *npals their count;
 * totals[0] the bytes of all pixels, totals[1] of all raw bytes, totals[2] the largest H * W. */
int og_pngd_records_host(const uint8_t* blob, const int64_t* offsets, int B, int channels, og_png_rec* recs, uint8_t* zblob, size_t zcap,
                         int64_t* zoffsets, uint8_t* pals, int pals_cap, int* npals, int64_t* totals);

/* The device is the one current at the first call that touches it; the handle owns its stream and workspace.  chunk 128. */
og_png* og_png_create(void);
void og_png_destroy(og_png* h);
int og_png_sync(og_png* h);
int og_png_set_chunk(og_png* h, int chunk);

/* The palettes of the og_png_decode_u8_dev calls that follow (npals may be 0); copied to the device before the call returns.
 * og_png_decode_stream replaces them. */
int og_png_set_palettes(og_png* h, const uint8_t* pals, int npals);

/* Everything resident, one micro-batch: zblob_dev the zlib streams, zoffsets_dev [B + 1] int64 into it, recs_dev [B], out_dev of cap
 * bytes, status_dev [B] int32.  raw_bytes: the workspace the records' raw_offsets lie in (totals[1]); max_pixels: the largest H * W
 * (it sizes a grid; a larger file is still decoded).  A record whose pixels leave cap gets status 6 and nothing of it is written; one whose raw
 * bytes leave raw_bytes gets status 6 and zeros.  Reads nothing outside zblob_dev[zoffsets[0], zoffsets[B]); writes only the records' pixel ranges and B statuses.
 * Asynchronous on the handle's stream. */
int og_png_decode_u8_dev(og_png* h, const uint8_t* zblob_dev, const int64_t* zoffsets_dev, const og_png_rec* recs_dev, int B, int channels,
                         long long raw_bytes, int max_pixels, uint8_t* out_dev, size_t cap, int32_t* status_dev);

/* Host bytes in: parses them, joins the IDAT payloads into the pinned slots, uploads the COMPRESSED bytes micro-batch by micro-batch
 * and delivers the pixels to out_host, to out_dev (they never visit the host), or both; cap counts either and must hold the sum of
 * H * W * channels over the accepted files, or OG_EINVAL before anything runs.  out_offsets [B + 1] int64, hw [B][2] int32 (0 0 for a
 * refused file) and status [B] on the host.  Synchronous.  On an error everything in flight is waited for and the handle stays usable. */
int og_png_decode_stream(og_png* h, const uint8_t* blob, const int64_t* offsets, int B, int channels, uint8_t* out_host_or_null,
                         uint8_t* out_dev_or_null, size_t cap, int64_t* out_offsets, int32_t* hw, int32_t* status);

/* Dry run of og_png_decode_stream over B files of forms [B][4] int32 (H, W, ctype, depth), without a device: one line per launch in
 * the columns of og_mjpd_plan, kernel|gx|gy|gz|block|lds|workspace|counters|writes ("out=END;status=END" or "-").  Returns the number
 * of launches; *workspace_bytes = the device workspace of the call apart from the compressed bytes, whose size no shape tells. */
int og_png_plan(const int32_t* forms, int B, int channels, int chunk, char* out, size_t cap, long long* workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
