// Baseline JPEG decoded on the device (include/decode/openglottal_hip_mjpd.h): the chunks of a Motion-JPEG AVI become [B,H,W,3] u8 BGR
// frames.  Included by og_api.hip after og_mjpeg.inc, whose Annex K tables and limits it shares; the kernels live here too.  A handle of
// its own: one stream, the workspace of ONE micro-batch, two pinned host slots.  Per micro-batch: k_mjpd_markers (the restart
// intervals of every frame), k_mjpd_entropy (a lane per interval: coefficients), k_mjpd_idct (component planes), k_mjpd_colour (BGR).
// All arithmetic is integer: the host twin and the kernels call the same inline functions and agree byte for byte.
// og_mjps.inc (included after this file) replaces k_mjpd_entropy for calls without restart markers when the handle asks for it; it
// restarts the bit reader below through og_jpegd_seek / og_jpegd_tell.
// With OG_MJPD_HOST_ONLY defined the file is a translation unit of its own for a host compiler: the parser and the twin, no HIP
// (tools/mjpd_host_fuzz.cpp builds it under sanitizers).
#include "../../include/decode/openglottal_hip_mjpd.h"

#ifdef OG_MJPD_HOST_ONLY
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#define OG_JPEG_HD inline
namespace {
thread_local std::string g_err;
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
bool og_misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
#define OG_ALIGN(ptr)                                                                                                              \
    do {                                                                                                                           \
        if (og_misaligned((ptr), alignof(decltype(*(ptr)))))                                                                       \
            return fail(OG_EINVAL, std::string(#ptr) + " must be aligned to " + std::to_string(alignof(decltype(*(ptr)))) + " bytes"); \
    } while (0)
constexpr long long kMjpegMaxPixels = 1ll << 24;
constexpr long long kMjpegBatchBytes = 256ll << 20;
#include "og_jpeg_annexk.inc"
}  // namespace
extern "C" const char* og_last_error(void) { return g_err.c_str(); }
#endif

constexpr long long kMjpdMaxFile = 1ll << 30;
constexpr int kMjpdMaxChunk = 1024;   // as the encoder's
constexpr int kMjpdStatusMax = 7;

// what the kernels read beside the bytes: one per distinct (DQT, DHT, component selectors) of a call, built on the host
struct MjpdTab {
    uint16_t q[3][64];        // per component, natural order
    uint16_t look[4][512];    // [0] DC table 0, [1] DC 1, [2] AC 0, [3] AC 1: (length << 8) | symbol for codes of up to 9 bits, else 0
    int32_t maxcode[4][17];   // [len]: the largest code of that length, -1 if there is none
    int32_t valoff[4][17];    // [len]: vals index of code c of that length = valoff + c
    uint8_t vals[4][256];
    uint8_t zz[64];           // zigzag position -> natural index
    uint8_t dcsel[4], acsel[4];   // per component: which of the four tables
};
static_assert(sizeof(MjpdTab) == 6120 && sizeof(og_mjpd_rec) == 32, "layouts stated in the header");

// the geometry of a form: by value into the kernels
struct MjpdForm {
    int sampling, ncomp, H, W;
    int hs[3], vs[3];         // blocks of a component in an MCU
    int mx, my, M;            // MCUs across, down, per frame
    int bw[3], bh[3];         // blocks across and down per component: the padded extent
    int boff[3], blocks;      // first block of a component in a frame, blocks per frame
    int cw, ch;               // the chroma components' true extent
};

// ---- the arithmetic: host twin and kernels ---------------------------------------------------------------------------------------
struct OgJpegdBits {
    const uint8_t* p;
    long long n, pos;   // bytes of the interval, the next one to read
    uint32_t acc;       // the low nb bits are the bits not yet consumed, oldest highest
    int nb;
};

// tops the bit buffer up to more than 24 bits; past the last data byte nothing is added.  Reads p[i] only for i < n.
OG_JPEG_HD void og_jpegd_fill(OgJpegdBits& s) {
    for (; s.nb <= 24 && s.pos < s.n;) {
        const uint32_t b = s.p[s.pos];
        if (b == 0xFF) {
            if (s.pos + 1 >= s.n || s.p[s.pos + 1] != 0) {   // a marker, or 0xFF as the last byte: the data ends here
                s.n = s.pos;
                break;
            }
            s.pos += 2;
        } else {
            s.pos += 1;
        }
        s.acc = (s.acc << 8) | b;
        s.nb += 8;
    }
}

// the next k bits (1..16) without consuming them; what lies past the data reads as 0
OG_JPEG_HD uint32_t og_jpegd_peek(const OgJpegdBits& s, int k) {
    return (s.nb >= k ? s.acc >> (s.nb - k) : s.acc << (k - s.nb)) & ((1u << k) - 1);
}

// one Huffman symbol of table `tab`; a negative result is minus the status
OG_JPEG_HD int og_jpegd_symbol(OgJpegdBits& s, const MjpdTab* t, int tab) {
    og_jpegd_fill(s);
    const uint32_t e = t->look[tab][og_jpegd_peek(s, 9)];
    int len = (int)(e >> 8), sym = (int)(e & 255);
    if (!e) {
        const int code = (int)og_jpegd_peek(s, 16);
        for (int l = 10; l <= 16; ++l) {
            const int c = code >> (16 - l);
            if (c <= t->maxcode[tab][l]) {
                len = l;
                sym = t->vals[tab][(t->valoff[tab][l] + c) & 255];
                break;
            }
        }
        if (!len) return s.nb < 16 ? -1 : -2;   // fewer than 16 bits left: the scan ended inside a code
    }
    if (len > s.nb) return -1;
    s.nb -= len;
    return sym;
}

// the n (1..11) value bits after a symbol, EXTENDed; *st = 1 if they are not there
OG_JPEG_HD int og_jpegd_receive(OgJpegdBits& s, int n, int* st) {
    og_jpegd_fill(s);
    if (s.nb < n) {
        *st = 1;
        return 0;
    }
    const int v = (int)og_jpegd_peek(s, n);
    s.nb -= n;
    return v < (1 << (n - 1)) ? v - (1 << n) + 1 : v;
}

// The reader restarted at a position: the next bit is bit `bit` (0 the highest) of data byte p[pos], which is no stuffed 00.
OG_JPEG_HD void og_jpegd_seek(OgJpegdBits& s, const uint8_t* p, long long n, long long pos, int bit) {
    s.p = p;
    s.n = n;
    s.pos = pos;
    s.acc = 0;
    s.nb = 0;
    if (bit) {
        og_jpegd_fill(s);
        s.nb = s.nb > bit ? s.nb - bit : 0;
    }
}

// Where the reader stands, in og_jpegd_seek's terms.  The nb bits not yet consumed end the last ceil(nb / 8) data bytes before
// s.pos; a data byte is never a 00 behind an FF (that 00 was skipped as stuffing), so the walk back steps over such pairs.  It reads
// only bytes the reader has read.
OG_JPEG_HD void og_jpegd_tell(const OgJpegdBits& s, long long* pos, int* bit) {
    long long q = s.pos;
    for (int left = (s.nb + 7) >> 3; left > 0; --left) {
        q -= 1;
        if (q >= 1 && s.p[q] == 0 && s.p[q - 1] == 0xFF) q -= 1;
    }
    *pos = q;
    *bit = (8 - (s.nb & 7)) & 7;
}

// One restart interval: MCUs [m0, m0 + count) of a frame whose coefficients ([component][block][64] int16, natural order, zero before
// the call) start at `coefs`.  Returns the status.  See SAFETY in the header.
OG_JPEG_HD int og_jpegd_interval(const uint8_t* bytes, long long length, const MjpdTab* t, const MjpdForm& g, int m0, int count, int16_t* coefs) {
    OgJpegdBits s{bytes, length, 0, 0, 0};
    int pred[3] = {0, 0, 0};
    for (int m = m0; m < m0 + count; ++m) {
        const int myi = m / g.mx, mxi = m - myi * g.mx;
        for (int c = 0; c < g.ncomp; ++c)
            for (int by = 0; by < g.vs[c]; ++by)
                for (int bx = 0; bx < g.hs[c]; ++bx) {
                    int16_t* blk = coefs + ((long long)g.boff[c] + (long long)(myi * g.vs[c] + by) * g.bw[c] + mxi * g.hs[c] + bx) * 64;
                    int st = 0;
                    int sym = og_jpegd_symbol(s, t, t->dcsel[c] & 3);
                    if (sym < 0) return -sym;
                    if (sym > 11) return 4;
                    if (sym) pred[c] += og_jpegd_receive(s, sym, &st);
                    if (st) return st;
                    if (pred[c] < -2048 || pred[c] > 2047) return 4;
                    blk[0] = (int16_t)pred[c];
                    for (int k = 1; k < 64; ++k) {
                        sym = og_jpegd_symbol(s, t, t->acsel[c] & 3);
                        if (sym < 0) return -sym;
                        const int run = sym >> 4, size = sym & 15;
                        if (size == 0) {
                            if (run != 15) break;   // EOB
                            k += 15;                // ZRL: sixteen zeros
                            if (k > 63) return 3;
                            continue;
                        }
                        k += run;
                        if (k > 63) return 3;
                        if (size > 10) return 4;
                        const int v = og_jpegd_receive(s, size, &st);
                        if (st) return st;
                        blk[t->zz[k] & 63] = (int16_t)v;
                    }
                }
    }
    return 0;
}

// one pass of libjpeg's jidctint over 8 values, in wrap-around arithmetic; shift 11 for the columns, 18 for the rows
OG_JPEG_HD int og_jpegd_descale(uint32_t x, int shift) { return (int)(int32_t)(x + (1u << (shift - 1))) >> shift; }
OG_JPEG_HD void og_jpegd_idct8(const int* in, int* out, int shift) {
    typedef uint32_t U;
    U z2 = (U)in[2], z3 = (U)in[6];
    U z1 = (z2 + z3) * 4433u;
    U tmp2 = z1 + z3 * (U)-15137;
    U tmp3 = z1 + z2 * 6270u;
    z2 = (U)in[0];
    z3 = (U)in[4];
    U tmp0 = (z2 + z3) << 13, tmp1 = (z2 - z3) << 13;
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = (U)in[7];
    tmp1 = (U)in[5];
    tmp2 = (U)in[3];
    tmp3 = (U)in[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    U z4 = tmp1 + tmp3;
    const U z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u;
    tmp1 *= 16819u;
    tmp2 *= 25172u;
    tmp3 *= 12299u;
    z1 *= (U)-7373;
    z2 *= (U)-20995;
    z3 *= (U)-16069;
    z4 *= (U)-3196;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    out[0] = og_jpegd_descale(tmp10 + tmp3, shift);
    out[7] = og_jpegd_descale(tmp10 - tmp3, shift);
    out[1] = og_jpegd_descale(tmp11 + tmp2, shift);
    out[6] = og_jpegd_descale(tmp11 - tmp2, shift);
    out[2] = og_jpegd_descale(tmp12 + tmp1, shift);
    out[5] = og_jpegd_descale(tmp12 - tmp1, shift);
    out[3] = og_jpegd_descale(tmp13 + tmp0, shift);
    out[4] = og_jpegd_descale(tmp13 - tmp0, shift);
}
OG_JPEG_HD int og_jpegd_clamp(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// the chroma sample of pixel (y, x) from a component plane of true extent cw x ch (row stride `stride`)
OG_JPEG_HD int og_jpegd_chroma(const uint8_t* plane, int stride, int cw, int ch, int sampling, int y, int x) {
    if (sampling <= 1) return plane[(long long)y * stride + x];
    const int i = x >> 1, odd = x & 1;
    const int j = odd ? (i + 1 < cw ? i + 1 : cw - 1) : (i > 0 ? i - 1 : 0);
    if (sampling == 2) {
        const uint8_t* r = plane + (long long)y * stride;
        if (cw <= 2) return r[i];
        return (3 * r[i] + r[j] + (odd ? 2 : 1)) >> 2;
    }
    const int rn = y >> 1;
    const uint8_t* near = plane + (long long)rn * stride;
    if (cw <= 2) return near[i];
    const int rf = (y & 1) ? (rn + 1 < ch ? rn + 1 : ch - 1) : (rn > 0 ? rn - 1 : 0);
    const uint8_t* far = plane + (long long)rf * stride;
    const int a = 3 * near[i] + far[i], b = 3 * near[j] + far[j];
    return (3 * a + b + (odd ? 7 : 8)) >> 4;
}

OG_JPEG_HD void og_jpegd_bgr(int y, int cb, int cr, uint8_t* out) {
    cb -= 128;
    cr -= 128;
    out[0] = (uint8_t)og_jpegd_clamp(y + ((116130 * cb + 32768) >> 16));
    out[1] = (uint8_t)og_jpegd_clamp(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    out[2] = (uint8_t)og_jpegd_clamp(y + ((91881 * cr + 32768) >> 16));
}

// pixel (y, x) of a frame from its planes ([component] at 64 * boff[c], stride 8 * bw[c])
OG_JPEG_HD void og_jpegd_pixel(const uint8_t* planes, const MjpdForm& g, int y, int x, uint8_t* out) {
    const int Y = planes[(long long)y * (8 * g.bw[0]) + x];
    if (g.ncomp == 1) {
        out[0] = out[1] = out[2] = (uint8_t)Y;
        return;
    }
    const int cb = og_jpegd_chroma(planes + 64ll * g.boff[1], 8 * g.bw[1], g.cw, g.ch, g.sampling, y, x);
    const int cr = og_jpegd_chroma(planes + 64ll * g.boff[2], 8 * g.bw[2], g.cw, g.ch, g.sampling, y, x);
    og_jpegd_bgr(Y, cb, cr, out);
}

// the frame's status from the record the host made and the extents of its file; 0: the scan may be walked
OG_JPEG_HD int og_jpegd_rec_status(const og_mjpd_rec& r, long long size, int nsets, int nI, int Ri) {
    if (r.status) return r.status > 0 && r.status <= kMjpdStatusMax ? r.status : 6;
    if (size < 0 || size > kMjpdMaxFile || r.scan_offset < 0 || r.scan_length < 0 || (long long)r.scan_offset + r.scan_length > size) return 6;
    if (r.tabset < 0 || r.tabset >= nsets) return 6;
    if (r.nI != nI || r.Ri != Ri) return 7;
    return 0;
}

#ifndef OG_MJPD_HOST_ONLY
// ---- kernels ---------------------------------------------------------------------------------------------------------------------
// A workgroup per frame.  ivl [frame][nI][2]: start and end of every interval inside the scan; mstat [frame]: the status it found.
__global__ __launch_bounds__(256) void k_mjpd_markers(const uint8_t* __restrict__ blob, const long long* __restrict__ offsets,
                                                      const og_mjpd_rec* __restrict__ recs, int nsets, int nI, int Ri, int* __restrict__ ivl,
                                                      int* __restrict__ mstat, int32_t* __restrict__ status) {
    __shared__ int s_wave[4];
    __shared__ int s_bad;
    const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const og_mjpd_rec rec = recs[f];
    const int st = og_jpegd_rec_status(rec, offsets[f + 1] - offsets[f], nsets, nI, Ri);
    if (st) {   // (the same for every lane)
        if (t == 0) status[f] = mstat[f] = st;
        return;
    }
    const uint8_t* p = blob + offsets[f] + rec.scan_offset;
    const int n = rec.scan_length;
    int* mine = ivl + (long long)f * nI * 2;
    if (t == 0) s_bad = 0;
    int base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + t;
        const bool hit = i + 1 < n && p[i] == 0xFF && (p[i + 1] & 0xF8) == 0xD0;
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) s_wave[w] = __popcll(bal);
        __syncthreads();
        int before = base;
        for (int j = 0; j < 4; ++j) {
            if (j < w) before += s_wave[j];
            base += s_wave[j];
        }
        if (hit) {
            const int k = before + __popcll(bal & ((1ull << lane) - 1));
            if ((p[i + 1] & 7) != (k & 7)) s_bad = 1;
            if (k + 1 < nI) {
                mine[2 * k + 1] = i;
                mine[2 * k + 2] = i + 2;
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        mine[0] = 0;
        mine[2 * nI - 1] = n;
        status[f] = mstat[f] = (base != nI - 1 || s_bad) ? 5 : 0;
    }
}

// A lane per restart interval: lane i of the micro-batch is interval i % nI of frame i / nI.
__global__ __launch_bounds__(64) void k_mjpd_entropy(const uint8_t* __restrict__ blob, const long long* __restrict__ offsets,
                                                     const og_mjpd_rec* __restrict__ recs, const MjpdTab* __restrict__ tabs, MjpdForm g, int nI,
                                                     int Ri, long long items, const int* __restrict__ ivl, const int* __restrict__ mstat,
                                                     int16_t* __restrict__ coefs, int32_t* __restrict__ status) {
    __shared__ MjpdTab s_tab;
    const int t = threadIdx.x;
    const long long i0 = (long long)blockIdx.x * 64, i = i0 + t;
    // the first lane's frame: its set goes to LDS unless the frame is refused (then its record may hold anything)
    const int f0 = (int)(i0 / nI);
    const int set0 = mstat[f0] == 0 ? recs[f0].tabset : -1;
    if (set0 >= 0) {
        const uint32_t* src = (const uint32_t*)(tabs + set0);
        uint32_t* dst = (uint32_t*)&s_tab;
        for (int j = t; j < (int)(sizeof(MjpdTab) / 4); j += 64) dst[j] = src[j];
    }
    __syncthreads();
    if (i >= items) return;
    const int f = (int)(i / nI), k = (int)(i - (long long)f * nI);
    if (mstat[f] != 0) return;   // (k_mjpd_markers' verdict; status[f] itself is raised by the lanes of this launch)
    const og_mjpd_rec rec = recs[f];
    const MjpdTab* tab = rec.tabset == set0 ? &s_tab : tabs + rec.tabset;
    const int* mine = ivl + ((long long)f * nI + k) * 2;
    const int m0 = Ri ? k * Ri : 0, count = Ri ? min(Ri, g.M - m0) : g.M;
    const int st = og_jpegd_interval(blob + offsets[f] + rec.scan_offset + mine[0], (long long)mine[1] - mine[0], tab, g, m0, count,
                                     coefs + (long long)f * g.blocks * 64);
    if (st) atomicMax(&status[f], st);
}

constexpr int kMjpdIdctLds = 32 * 8 * 9 * 4;

// 8 lanes per block: column r, then row r.
__global__ __launch_bounds__(256) void k_mjpd_idct(const int16_t* __restrict__ coefs, long long nblocks, MjpdForm g,
                                                   const og_mjpd_rec* __restrict__ recs, const MjpdTab* __restrict__ tabs, int nsets,
                                                   uint8_t* __restrict__ planes) {
    extern __shared__ uint32_t lds_i[];
    const int gi = threadIdx.x >> 3, r = threadIdx.x & 7;
    int* tile = (int*)lds_i + gi * 72;   // [8][9]
    const long long blk = (long long)blockIdx.x * 32 + gi;
    const bool valid = blk < nblocks;
    int f = 0, c = 0, lb = 0;
    if (valid) {
        f = (int)(blk / g.blocks);
        const int b = (int)(blk - (long long)f * g.blocks);
        c = g.ncomp == 3 ? (b >= g.boff[1]) + (b >= g.boff[2]) : 0;
        lb = b - g.boff[c];
        int set = recs[f].tabset;   // (a refused frame's coefficients are all 0: any set serves)
        set = set < 0 || set >= nsets ? 0 : set;
        const uint16_t* q = tabs[set].q[c];
        const int16_t* src = coefs + blk * 64;
        int in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = (int)src[8 * k + r] * (int)q[8 * k + r];
        og_jpegd_idct8(in, out, 11);
#pragma unroll
        for (int k = 0; k < 8; ++k) tile[9 * k + r] = out[k];
    }
    __syncthreads();
    if (valid) {
        int in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = tile[9 * r + k];
        og_jpegd_idct8(in, out, 18);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= (uint32_t)og_jpegd_clamp(out[k] + 128) << (8 * k);
            hi |= (uint32_t)og_jpegd_clamp(out[k + 4] + 128) << (8 * k);
        }
        const int by = lb / g.bw[c], bx = lb - by * g.bw[c];
        uint32_t* dst = (uint32_t*)(planes + ((long long)f * g.blocks + g.boff[c]) * 64 + (long long)(by * 8 + r) * (8 * g.bw[c]) + 8 * bx);
        dst[0] = lo;
        dst[1] = hi;
    }
}

// A lane per pixel: grid (ceil(H * W / 256), frames).
__global__ __launch_bounds__(256) void k_mjpd_colour(const uint8_t* __restrict__ planes, MjpdForm g, const int32_t* __restrict__ status,
                                                     uint8_t* __restrict__ frames) {
    const int f = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= g.H * g.W) return;
    uint8_t px[3] = {0, 0, 0};
    if (status[f] < 6) {
        const int y = idx / g.W, x = idx - y * g.W;
        og_jpegd_pixel(planes + (long long)f * g.blocks * 64, g, y, x, px);
    }
    uint8_t* dst = frames + ((long long)f * g.H * g.W + idx) * 3;
    dst[0] = px[0];
    dst[1] = px[1];
    dst[2] = px[2];
}
// og_mjps.inc: a workgroup per frame decodes a scan without restart markers in parallel
__global__ void k_mjps_entropy(const uint8_t* __restrict__ blob, const long long* __restrict__ offsets, const og_mjpd_rec* __restrict__ recs,
                               const MjpdTab* __restrict__ tabs, MjpdForm g, int sub, const int* __restrict__ mstat, int16_t* __restrict__ coefs,
                               int32_t* __restrict__ status);
#endif   // OG_MJPD_HOST_ONLY

// ---- host side -------------------------------------------------------------------------------------------------------------------
#ifndef OG_MJPD_HOST_ONLY
struct og_mjpd : OgStreamHandle {
    int split = 0, sub = 0;   // og_mjps_set_split (og_mjps.inc): 1 sends calls with Ri == 0 through k_mjps_entropy; sub 0 is the default
    OgBuf<MjpdTab> d_tabs;
    int nsets = 0, sampling = -1, Ri = 0;   // what d_tabs holds, and the form of the resident calls
    // each buffer holds the bytes of the largest micro-batch run so far
    OgBuf<uint8_t> d_ws;    // coefficients, planes, intervals
    OgBuf<uint8_t> d_in;    // streamed entry: offsets, records, bytes
    OgBuf<uint8_t> d_out;   // streamed entry: frames, unless the caller's device buffer takes them
    OgBuf<int32_t> d_status;
    struct Slot {
        OgBuf<uint8_t> h_in{true}, h_out{true};
        OgBuf<int32_t> h_status{true};
        hipEvent_t ev = nullptr;
        int b0 = -1, nb = 0;
    } slots[2];
};
#endif

namespace {

// what distinguishes one table set from another, as the segments gave it (zeroed before it is filled, so memcmp compares it)
struct MjpdSpec {
    uint8_t q[4][64];          // natural order
    uint8_t bits[4][16];       // [0] DC 0, [1] DC 1, [2] AC 0, [3] AC 1
    uint8_t vals[4][256];
    uint8_t qhave[4], hhave[4];
    uint8_t tq[4], td[4], ta[4];
    int32_t ncomp;
};

struct MjpdParsed {
    og_jpegd_info info;
    MjpdSpec spec;
};

int mjpd_refuse(og_jpegd_info* info, const std::string& why) {
    info->status = 6;
    g_err = "unsupported JPEG: " + why;
    return 6;
}

bool mjpd_form(int H, int W, int sampling, MjpdForm* g) {
    if (sampling < 0 || sampling > 3 || H <= 0 || W <= 0) return false;
    memset(g, 0, sizeof *g);
    g->sampling = sampling;
    g->ncomp = sampling ? 3 : 1;
    g->H = H;
    g->W = W;
    const int hl = sampling >= 2 ? 2 : 1, vl = sampling == 3 ? 2 : 1;
    for (int c = 0; c < 3; ++c) g->hs[c] = g->vs[c] = 1;
    g->hs[0] = hl;
    g->vs[0] = vl;
    g->mx = (W + 8 * hl - 1) / (8 * hl);
    g->my = (H + 8 * vl - 1) / (8 * vl);
    g->M = g->mx * g->my;
    int at = 0;
    for (int c = 0; c < g->ncomp; ++c) {
        g->bw[c] = g->mx * g->hs[c];
        g->bh[c] = g->my * g->vs[c];
        g->boff[c] = at;
        at += g->bw[c] * g->bh[c];
    }
    g->blocks = at;
    g->cw = (W + hl - 1) / hl;
    g->ch = (H + vl - 1) / vl;
    return true;
}
int mjpd_intervals(const MjpdForm& g, int Ri) { return Ri > 0 ? (g.M + Ri - 1) / Ri : 1; }

// The headers of one file.  Returns 0 or 6; the reason of a refusal goes to g_err.  Reads jpeg[i] only for i < size.
int mjpd_parse(const uint8_t* jpeg, size_t size, MjpdParsed* out) {
    memset(out, 0, sizeof *out);
    og_jpegd_info* info = &out->info;
    MjpdSpec& sp = out->spec;
    info->sampling = -1;
    if (size > (size_t)kMjpdMaxFile) return mjpd_refuse(info, "the file is above 2^30 bytes");
    if (size < 4 || jpeg[0] != 0xFF || jpeg[1] != 0xD8) return mjpd_refuse(info, "no SOI");
    size_t pos = 2;
    bool sof = false, sos = false;
    int cid[3] = {0, 0, 0}, ch[3] = {0, 0, 0}, cv[3] = {0, 0, 0};
    for (; pos < size && !sos;) {
        if (jpeg[pos] != 0xFF) return mjpd_refuse(info, "a byte that is no marker at offset " + std::to_string(pos) + " of the headers");
        if (pos + 1 >= size) break;
        const int m = jpeg[pos + 1];
        if (m == 0xFF) {   // a fill byte
            pos += 1;
            continue;
        }
        pos += 2;
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // no length
        if (m == 0xD9) return mjpd_refuse(info, "EOI before SOS");
        if (m == 0xD8) return mjpd_refuse(info, "a second SOI");
        if (pos + 2 > size) break;
        const size_t L = ((size_t)jpeg[pos] << 8) | jpeg[pos + 1];
        if (L < 2 || pos + L > size) return mjpd_refuse(info, "a truncated header segment");
        const uint8_t* s = jpeg + pos + 2;
        const size_t n = L - 2;
        if (m == 0xC0) {
            if (sof) return mjpd_refuse(info, "two SOF0 segments");
            if (n < 6) return mjpd_refuse(info, "a truncated header segment");
            if (s[0] != 8) return mjpd_refuse(info, std::to_string((int)s[0]) + "-bit samples");
            info->H = (s[1] << 8) | s[2];
            info->W = (s[3] << 8) | s[4];
            info->ncomp = s[5];
            if (info->ncomp != 1 && info->ncomp != 3) return mjpd_refuse(info, std::to_string(info->ncomp) + " components");
            if (n < 6 + 3 * (size_t)info->ncomp) return mjpd_refuse(info, "a truncated header segment");
            if (info->H == 0 || info->W == 0) return mjpd_refuse(info, "H or W of 0");
            if ((long long)info->H * info->W > kMjpegMaxPixels) return mjpd_refuse(info, "H * W above " + std::to_string(kMjpegMaxPixels) + " pixels");
            for (int c = 0; c < info->ncomp; ++c) {
                cid[c] = s[6 + 3 * c];
                ch[c] = s[7 + 3 * c] >> 4;
                cv[c] = s[7 + 3 * c] & 15;
                if (s[8 + 3 * c] > 3) return mjpd_refuse(info, "a quantisation table id above 3");
                sp.tq[c] = s[8 + 3 * c];
            }
            if (info->ncomp == 1) {
                info->sampling = 0;
            } else {
                const std::string form = std::to_string(ch[0]) + "x" + std::to_string(cv[0]) + "," + std::to_string(ch[1]) + "x" + std::to_string(cv[1]) +
                                         "," + std::to_string(ch[2]) + "x" + std::to_string(cv[2]);
                if (ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1) return mjpd_refuse(info, "sampling factors " + form);
                if (ch[0] == 1 && cv[0] == 1) info->sampling = 1;
                else if (ch[0] == 2 && cv[0] == 1) info->sampling = 2;
                else if (ch[0] == 2 && cv[0] == 2) info->sampling = 3;
                else return mjpd_refuse(info, "sampling factors " + form);
            }
            sp.ncomp = info->ncomp;
            sof = true;
        } else if (m == 0xCC) {
            return mjpd_refuse(info, "arithmetic coding (DAC)");
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8) {
            return mjpd_refuse(info, m == 0xC2 ? "progressive DCT (SOF2)" : m == 0xC1 ? "extended sequential DCT (SOF1)"
                                                                                       : "frame type SOF" + std::to_string(m - 0xC0));
        } else if (m == 0xC4) {
            for (size_t at = 0; at < n;) {
                if (at + 17 > n) return mjpd_refuse(info, "a truncated DHT");
                const int tc = s[at] >> 4, th = s[at] & 15;
                if (tc > 1 || th > 1) return mjpd_refuse(info, "a Huffman table of class " + std::to_string(tc) + " id " + std::to_string(th));
                const int ti = 2 * tc + th;
                int total = 0, code = 0;
                for (int l = 1; l <= 16; ++l) {
                    const int cnt = s[at + l];
                    code += cnt;
                    if (code > (1 << l)) return mjpd_refuse(info, "a DHT whose counts are no prefix code");
                    code <<= 1;
                    total += cnt;
                }
                if (total > 256 || at + 17 + total > n) return mjpd_refuse(info, "a truncated DHT");
                memset(sp.vals[ti], 0, 256);
                memcpy(sp.bits[ti], s + at + 1, 16);
                memcpy(sp.vals[ti], s + at + 17, total);
                sp.hhave[ti] = 1;
                at += 17 + total;
            }
        } else if (m == 0xDB) {
            for (size_t at = 0; at < n;) {
                const int pq = s[at] >> 4, tq = s[at] & 15;
                if (pq != 0) return mjpd_refuse(info, "a 16-bit quantisation table");
                if (tq > 3) return mjpd_refuse(info, "a quantisation table id above 3");
                if (at + 65 > n) return mjpd_refuse(info, "a truncated DQT");
                for (int k = 0; k < 64; ++k) sp.q[tq][kJpegZigzag[k]] = s[at + 1 + k];
                sp.qhave[tq] = 1;
                at += 65;
            }
        } else if (m == 0xDD) {
            if (n < 2) return mjpd_refuse(info, "a truncated DRI");
            info->Ri = (s[0] << 8) | s[1];
        } else if (m == 0xDA) {
            if (!sof) return mjpd_refuse(info, "SOS before SOF0");
            if (n < 1 || n < 1 + 2 * (size_t)s[0] + 3) return mjpd_refuse(info, "a truncated SOS");
            if (s[0] != info->ncomp) return mjpd_refuse(info, "a scan of " + std::to_string((int)s[0]) + " of the " + std::to_string(info->ncomp) +
                                                                  " components (several scans)");
            for (int c = 0; c < info->ncomp; ++c) {
                if (s[1 + 2 * c] != cid[c]) return mjpd_refuse(info, "a scan whose components are not in SOF order");
                sp.td[c] = s[2 + 2 * c] >> 4;
                sp.ta[c] = s[2 + 2 * c] & 15;
                if (sp.td[c] > 1 || sp.ta[c] > 1) return mjpd_refuse(info, "a scan that names a Huffman table id above 1");
            }
            const uint8_t* e = s + 1 + 2 * info->ncomp;
            if (e[0] != 0 || e[1] != 63 || e[2] != 0) return mjpd_refuse(info, "spectral selection or successive approximation");
            sos = true;
        }
        pos += L;
    }
    if (!sos) return mjpd_refuse(info, "a truncated header (no SOS)");
    // the scan: to the first marker that is neither RSTm nor a stuffed or fill 0xFF
    size_t end = size;
    for (size_t at = pos; at < size;) {
        const uint8_t* hit = (const uint8_t*)memchr(jpeg + at, 0xFF, size - at);
        if (!hit) break;
        const size_t i = (size_t)(hit - jpeg);
        if (i + 1 >= size) break;
        const int m = jpeg[i + 1];
        if (m == 0 || (m >= 0xD0 && m <= 0xD7)) {
            at = i + 2;
        } else if (m == 0xFF) {
            at = i + 1;
        } else {
            if (m != 0xD9) return mjpd_refuse(info, "a marker after the scan that is not EOI (several scans)");
            end = i;
            break;
        }
    }
    info->scan_offset = (int64_t)pos;
    info->scan_length = (int64_t)(end - pos);
    int nh = 0;
    for (int i = 0; i < 4; ++i) {
        if (sp.qhave[i]) info->tables |= 1 << i;
        if (sp.hhave[i]) info->tables |= 1 << ((i < 2 ? 4 : 8) + (i & 1));
        nh += sp.hhave[i];
    }
    for (int c = 0; c < info->ncomp; ++c) {
        if (!sp.qhave[sp.tq[c]]) return mjpd_refuse(info, "quantisation table " + std::to_string((int)sp.tq[c]) + " is not defined");
        if (nh && (!sp.hhave[sp.td[c]] || !sp.hhave[2 + sp.ta[c]])) return mjpd_refuse(info, "a Huffman table the scan names is not defined");
    }
    if (!nh) {   // no DHT at all: Annex K.3
        for (int i = 0; i < 2; ++i) {
            memcpy(sp.bits[i], kJpegDcBits[i], 16);
            memcpy(sp.vals[i], kJpegDcVals, 12);
            memcpy(sp.bits[2 + i], kJpegAcBits[i], 16);
            memcpy(sp.vals[2 + i], kJpegAcVals[i], 162);
        }
    }
    // only what the scan uses tells one set from another
    for (int i = 0; i < 4; ++i) {
        bool qused = false, hused = false;
        for (int c = 0; c < info->ncomp; ++c) {
            qused |= sp.tq[c] == i;
            hused |= (i < 2 ? sp.td[c] == i : sp.ta[c] == i - 2);
        }
        if (!qused) memset(sp.q[i], 0, 64);
        if (!hused) {
            memset(sp.bits[i], 0, 16);
            memset(sp.vals[i], 0, 256);
        }
        sp.qhave[i] = sp.hhave[i] = 0;
    }
    MjpdForm g;
    mjpd_form(info->H, info->W, info->sampling, &g);
    info->M = g.M;
    info->nI = mjpd_intervals(g, info->Ri);
    return 0;
}

void mjpd_build_tab(const MjpdSpec& sp, MjpdTab* t) {
    memset(t, 0, sizeof *t);
    for (int c = 0; c < sp.ncomp && c < 3; ++c) {
        for (int i = 0; i < 64; ++i) t->q[c][i] = sp.q[sp.tq[c]][i];
        t->dcsel[c] = sp.td[c];
        t->acsel[c] = (uint8_t)(2 + sp.ta[c]);
    }
    for (int k = 0; k < 64; ++k) t->zz[k] = kJpegZigzag[k];
    for (int i = 0; i < 4; ++i) {
        memcpy(t->vals[i], sp.vals[i], 256);
        int code = 0, at = 0;
        for (int l = 1; l <= 16; ++l) {
            const int cnt = sp.bits[i][l - 1];
            t->valoff[i][l] = at - code;
            t->maxcode[i][l] = cnt ? code + cnt - 1 : -1;
            if (l <= 9)
                for (int j = 0; j < cnt; ++j)
                    for (int r = 0; r < (1 << (9 - l)); ++r) t->look[i][((code + j) << (9 - l)) | r] = (uint16_t)((l << 8) | sp.vals[i][(at + j) & 255]);
            code = (code + cnt) << 1;
            at += cnt;
        }
        t->maxcode[i][0] = -1;
    }
}

// the RSTm of a scan as k_mjpd_markers finds them: ivl [nI][2]; returns 0 or 5
int mjpd_markers_host(const uint8_t* p, int n, int nI, int* ivl) {
    int k = 0;
    bool bad = false;
    ivl[0] = 0;
    for (int i = 0; i + 1 < n; ++i) {
        if (p[i] != 0xFF || (p[i + 1] & 0xF8) != 0xD0) continue;
        if ((p[i + 1] & 7) != (k & 7)) bad = true;
        if (k + 1 < nI) {
            ivl[2 * k + 1] = i;
            ivl[2 * k + 2] = i + 2;
        }
        ++k;
    }
    ivl[2 * nI - 1] = n;
    return (k != nI - 1 || bad) ? 5 : 0;
}

// what k_mjpd_idct and k_mjpd_colour do to one frame's coefficients: H * W * 3 bytes
void mjpd_pixels_host(const int16_t* coefs, const MjpdTab& tab, const MjpdForm& g, uint8_t* out) {
    std::vector<uint8_t> planes((size_t)g.blocks * 64);
    for (int c = 0; c < g.ncomp; ++c)
        for (int lb = 0; lb < g.bw[c] * g.bh[c]; ++lb) {
            const int16_t* src = coefs + ((size_t)g.boff[c] + lb) * 64;
            int ws[64], in[8], o[8];
            for (int r = 0; r < 8; ++r) {
                for (int k = 0; k < 8; ++k) in[k] = (int)src[8 * k + r] * (int)tab.q[c][8 * k + r];
                og_jpegd_idct8(in, o, 11);
                for (int k = 0; k < 8; ++k) ws[8 * k + r] = o[k];
            }
            const int by = lb / g.bw[c], bx = lb - by * g.bw[c];
            for (int r = 0; r < 8; ++r) {
                og_jpegd_idct8(ws + 8 * r, o, 18);
                uint8_t* dst = planes.data() + (size_t)g.boff[c] * 64 + (size_t)(by * 8 + r) * (8 * g.bw[c]) + 8 * bx;
                for (int k = 0; k < 8; ++k) dst[k] = (uint8_t)og_jpegd_clamp(o[k] + 128);
            }
        }
    for (int y = 0; y < g.H; ++y)
        for (int x = 0; x < g.W; ++x) og_jpegd_pixel(planes.data(), g, y, x, out + ((size_t)y * g.W + x) * 3);
}

// the twin of one micro-batch's work on one accepted frame: status and H * W * 3 bytes
int mjpd_frame_host(const uint8_t* jpeg, const og_jpegd_info& info, const MjpdTab& tab, uint8_t* out) {
    MjpdForm g;
    mjpd_form(info.H, info.W, info.sampling, &g);
    std::vector<int16_t> coefs((size_t)g.blocks * 64, 0);
    std::vector<int> ivl((size_t)info.nI * 2, 0);
    const uint8_t* scan = jpeg + info.scan_offset;
    int st = mjpd_markers_host(scan, (int)info.scan_length, info.nI, ivl.data());
    if (!st)
        for (int k = 0; k < info.nI; ++k) {
            const int m0 = info.Ri ? k * info.Ri : 0, count = info.Ri ? std::min(info.Ri, g.M - m0) : g.M;
            st = std::max(st, og_jpegd_interval(scan + ivl[2 * k], (long long)ivl[2 * k + 1] - ivl[2 * k], &tab, g, m0, count, coefs.data()));
        }
    mjpd_pixels_host(coefs.data(), tab, g, out);
    return st;
}

// B files: records, distinct table sets, the form of the first accepted one
struct MjpdCall {
    std::vector<og_mjpd_rec> recs;
    std::vector<MjpdSpec> specs;
    int H = 0, W = 0, sampling = -1, Ri = 0;
    std::string first_refusal;
};
int mjpd_records(const uint8_t* blob, const int64_t* offsets, int B, MjpdCall* call) {
    call->recs.assign((size_t)B, og_mjpd_rec{0, 0, 0, 0, 0, 0, 0, 0});
    MjpdParsed p;
    for (int i = 0; i < B; ++i) {
        if (offsets[i] < 0 || offsets[i + 1] < offsets[i]) return fail(OG_EINVAL, "offsets must not be negative or decrease");
        og_mjpd_rec& r = call->recs[i];
        if (mjpd_parse(blob + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), &p)) {
            r.status = 6;
            if (call->first_refusal.empty()) call->first_refusal = g_err;
            continue;
        }
        if (call->sampling < 0) {
            call->H = p.info.H;
            call->W = p.info.W;
            call->sampling = p.info.sampling;
            call->Ri = p.info.Ri;
        }
        if (p.info.H != call->H || p.info.W != call->W || p.info.sampling != call->sampling || p.info.Ri != call->Ri) {
            r.status = 7;
            continue;
        }
        r.scan_offset = (int32_t)p.info.scan_offset;
        r.scan_length = (int32_t)p.info.scan_length;
        r.Ri = p.info.Ri;
        r.nI = p.info.nI;
        int set = -1;
        for (int j = (int)call->specs.size() - 1; j >= 0 && set < 0; --j)
            if (!memcmp(&call->specs[j], &p.spec, sizeof(MjpdSpec))) set = j;
        if (set < 0) {
            set = (int)call->specs.size();
            call->specs.push_back(p.spec);
        }
        r.tabset = set;
    }
    return OG_OK;
}

long long mjpd_frame_ws(const MjpdForm& g, int nI) { return (long long)g.blocks * 192 + (long long)nI * 8 + 4; }
int mjpd_chunk(int chunk, const MjpdForm& g, int nI) {
    const long long fit = kMjpegBatchBytes / mjpd_frame_ws(g, nI);
    return (int)(fit < 1 ? 1 : (fit < chunk ? fit : chunk));
}
int check_mjpd_shape(int H, int W) {
    if (H <= 0 || W <= 0) return fail(OG_EINVAL, "bad H/W");
    if (H > 65535 || W > 65535) return fail(OG_EINVAL, "H and W must fit SOF0's 16 bits");
    if ((long long)H * W > kMjpegMaxPixels) return fail(OG_EINVAL, "H*W above " + std::to_string(kMjpegMaxPixels) + " pixels");
    return OG_OK;
}

#ifndef OG_MJPD_HOST_ONLY
// og_mjps.inc: the split entropy pass, its static LDS, and the subsequence length a handle's mode asks for (0: the lane per interval)
int mjps_lds_bytes();
int mjps_sub_of(int mode, int sub, int Ri);

void mjpd_free(og_mjpd* h) {
    og_release(h->d_tabs, h->d_ws, h->d_in, h->d_out, h->d_status);
    for (auto& s : h->slots) {
        og_release(s.h_in, s.h_out, s.h_status);
        if (s.ev) (void)hipEventDestroy(s.ev);
    }
}

int mjpd_upload_tabs(og_mjpd* h, const MjpdTab* tabs, int nsets, int sampling, int Ri) {
    h->nsets = 0;
    h->sampling = -1;
    int rc = h->d_tabs.grow(h, (size_t)(nsets ? nsets : 1) * sizeof(MjpdTab), "mjpd");
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));   // (launches in flight read the old sets; the pageable source must outlive the copy)
    if (nsets) HIPCHK(hipMemcpy(h->d_tabs, tabs, (size_t)nsets * sizeof(MjpdTab), hipMemcpyHostToDevice));
    h->nsets = nsets;
    h->sampling = sampling;
    h->Ri = Ri;
    return OG_OK;
}

// One micro-batch of nb resident files.  ws: the handle's workspace (a placeholder in a dry run).  frames, status: of these nb frames.
// sub > 0 (only with Ri == 0): the entropy pass is k_mjps_entropy at that subsequence length (og_mjps.inc).
int mjpd_batch(hipStream_t st, uint8_t* ws, const MjpdTab* tabs, int nsets, const uint8_t* blob, const long long* offsets,
               const og_mjpd_rec* recs, int nb, const MjpdForm& g, int Ri, int sub, uint8_t* frames, int32_t* status) {
    const int nI = mjpd_intervals(g, Ri);
    const long long nblocks = (long long)nb * g.blocks, items = (long long)nb * nI;
    int16_t* coefs = (int16_t*)ws;
    uint8_t* planes = ws + nblocks * 128;
    int* ivl = (int*)(planes + nblocks * 64);
    int* mstat = ivl + items * 2;
    if (!g_plan) HIPCHK(hipMemsetAsync(coefs, 0, (size_t)nblocks * 128, st));
    plan_need((long long)nb * mjpd_frame_ws(g, nI), 0);
    OG_LAUNCH(k_mjpd_markers, dim3((unsigned)nb), dim3(256), 0, st, blob, offsets, recs, nsets, nI, Ri, ivl, mstat, status);
    if (g_plan) plan_write("status", status, (long long)nb * 4);
    if (sub > 0 && Ri == 0) {
        OG_LAUNCH(k_mjps_entropy, dim3((unsigned)nb), dim3(256), 0, st, blob, offsets, recs, tabs, g, sub, (const int*)mstat, coefs, status);
    } else {
        OG_LAUNCH(k_mjpd_entropy, dim3((unsigned)((items + 63) / 64)), dim3(64), 0, st, blob, offsets, recs, tabs, g, nI, Ri, items, (const int*)ivl,
                  (const int*)mstat, coefs, status);
    }
    if (g_plan) {
        g_plan->recs.back().lds = sub > 0 && Ri == 0 ? (unsigned)mjps_lds_bytes() : (unsigned)sizeof(MjpdTab);   // static LDS: stated, so that the plan tells the truth
        plan_write("status", status, (long long)nb * 4);
    }
    OG_LAUNCH(k_mjpd_idct, dim3((unsigned)((nblocks + 31) / 32)), dim3(256), kMjpdIdctLds, st, (const int16_t*)coefs, nblocks, g, recs, tabs, nsets,
              planes);
    OG_LAUNCH(k_mjpd_colour, dim3((unsigned)(((long long)g.H * g.W + 255) / 256), (unsigned)nb), dim3(256), 0, st, (const uint8_t*)planes, g,
              (const int32_t*)status, frames);
    if (g_plan) plan_write("frames", frames, (long long)nb * g.H * g.W * 3);
    return OG_OK;
}
#endif   // OG_MJPD_HOST_ONLY

}  // namespace

extern "C" {

long long og_mjpd_limit(int which) {
    switch (which) {
        case 0: return kMjpegMaxPixels;
        case 1: return kMjpdMaxChunk;
        case 2: return (long long)sizeof(og_mjpd_rec);
        case 3: return (long long)sizeof(MjpdTab);
        case 4: return kMjpdStatusMax;
        case 5: return kMjpdMaxFile;
        case 6: return 128;
        default: return -1;
    }
}

int og_jpegd_parse_host(const uint8_t* jpeg, size_t size, og_jpegd_info* info) {
    if (!jpeg || !info) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(info);
    MjpdParsed p;
    mjpd_parse(jpeg, size, &p);
    *info = p.info;
    return OG_OK;
}

int og_jpegd_decode_host(const uint8_t* jpeg, size_t size, uint8_t* out_bgr, size_t cap, int* status) {
    if (!jpeg || !out_bgr || !status) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(status);
    MjpdParsed p;
    if (mjpd_parse(jpeg, size, &p)) {
        *status = 6;
        return OG_OK;
    }
    const unsigned long long need = (unsigned long long)p.info.H * p.info.W * 3;
    if ((unsigned long long)cap < need) return fail(OG_EINVAL, "cap is below H * W * 3 = " + std::to_string(need) + " bytes");
    MjpdTab tab;
    mjpd_build_tab(p.spec, &tab);
    *status = mjpd_frame_host(jpeg, p.info, tab, out_bgr);
    return OG_OK;
}

int og_jpegd_idct_pass_host(const int32_t* in8, int shift, int32_t* out8) {
    if (!in8 || !out8) return fail(OG_EINVAL, "null buffer");
    if (shift != 11 && shift != 18) return fail(OG_EINVAL, "shift must be 11 (the column pass) or 18 (the row pass)");
    OG_ALIGN(in8);
    OG_ALIGN(out8);
    int in[8], out[8];
    for (int k = 0; k < 8; ++k) in[k] = in8[k];
    og_jpegd_idct8(in, out, shift);
    for (int k = 0; k < 8; ++k) out8[k] = out[k];
    return OG_OK;
}

int og_jpegd_records_host(const uint8_t* blob, const int64_t* offsets, int B, og_mjpd_rec* recs, uint8_t* tabs, int tabs_cap, int* nsets,
                          int* H, int* W, int* sampling, int* Ri) {
    if (B < 0 || tabs_cap < 0) return fail(OG_EINVAL, "bad B");
    if (!nsets || !H || !W || !sampling || !Ri) return fail(OG_EINVAL, "null result");
    OG_ALIGN(offsets);
    OG_ALIGN(recs);
    OG_ALIGN((const uint32_t*)tabs);
    OG_ALIGN(nsets);
    OG_ALIGN(H);
    OG_ALIGN(W);
    OG_ALIGN(sampling);
    OG_ALIGN(Ri);
    if (B > 0 && (!blob || !offsets || !recs || !tabs)) return fail(OG_EINVAL, "null buffer");
    MjpdCall call;
    const int rc = B ? mjpd_records(blob, offsets, B, &call) : OG_OK;
    if (rc) return rc;
    if ((int)call.specs.size() > tabs_cap) return fail(OG_EINVAL, "tabs_cap is below the " + std::to_string(call.specs.size()) + " table sets of these files");
    for (size_t i = 0; i < call.specs.size(); ++i) {
        MjpdTab t;
        mjpd_build_tab(call.specs[i], &t);
        memcpy(tabs + i * sizeof(MjpdTab), &t, sizeof t);
    }
    if (B) memcpy(recs, call.recs.data(), (size_t)B * sizeof(og_mjpd_rec));
    *nsets = (int)call.specs.size();
    *H = call.H;
    *W = call.W;
    *sampling = call.sampling;
    *Ri = call.Ri;
    if (!call.first_refusal.empty()) g_err = call.first_refusal;
    return OG_OK;
}

#ifndef OG_MJPD_HOST_ONLY
og_mjpd* og_mjpd_create(void) { return new og_mjpd(); }

void og_mjpd_destroy(og_mjpd* h) {
    og_stream_destroy(h, [h] { mjpd_free(h); });
}

int og_mjpd_sync(og_mjpd* h) { return og_stream_sync(h); }

int og_mjpd_set_chunk(og_mjpd* h, int chunk) { return og_stream_set_chunk(h, chunk, kMjpdMaxChunk); }

int og_mjpd_set_tables(og_mjpd* h, const uint8_t* tabs, int nsets, int sampling, int Ri) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (nsets < 1 || !tabs) return fail(OG_EINVAL, "at least one table set is needed");
    if (sampling < 0 || sampling > 3) return fail(OG_EINVAL, "sampling must be 0..3");
    if (Ri < 0 || Ri > 65535) return fail(OG_EINVAL, "Ri must be 0..65535");
    OG_ALIGN((const uint32_t*)tabs);
    int rc = og_stream_ready(h);
    if (rc) return rc;
    OG_SCOPE(h);
    return mjpd_upload_tabs(h, (const MjpdTab*)tabs, nsets, sampling, Ri);
}

int og_mjpd_decode_u8_dev(og_mjpd* h, const uint8_t* blob_dev, const int64_t* offsets_dev, const og_mjpd_rec* recs_dev, int B, int H, int W,
                          uint8_t* frames_dev, size_t cap, int32_t* status_dev) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (B < 0) return fail(OG_EINVAL, "bad B");
    int rc = check_mjpd_shape(H, W);
    if (rc) return rc;
    if ((unsigned long long)cap < (unsigned long long)B * H * W * 3)
        return fail(OG_EINVAL, "cap is below B * H * W * 3 = " + std::to_string((unsigned long long)B * H * W * 3) + " bytes");
    OG_ALIGN(offsets_dev);
    OG_ALIGN(recs_dev);
    OG_ALIGN(status_dev);
    if (B == 0) return OG_OK;
    if (!blob_dev || !offsets_dev || !recs_dev || !frames_dev || !status_dev) return fail(OG_EINVAL, "null buffer");
    if (h->sampling < 0 || h->nsets < 1) return fail(OG_ESTATE, "og_mjpd_set_tables has not been called");
    if ((rc = og_stream_ready(h))) return rc;
    OG_SCOPE(h);
    MjpdForm g;
    mjpd_form(H, W, h->sampling, &g);
    const int nI = mjpd_intervals(g, h->Ri), chunk = mjpd_chunk(h->chunk, g, nI), cb = chunk < B ? chunk : B;
    if ((rc = h->d_ws.grow(h, (size_t)cb * mjpd_frame_ws(g, nI), "mjpd"))) return rc;
    const size_t fb = (size_t)H * W * 3;
    for (int b0 = 0; b0 < B && !rc; b0 += chunk) {
        const int nb = (B - b0 < chunk) ? B - b0 : chunk;
        rc = mjpd_batch(h->stream, h->d_ws, h->d_tabs, h->nsets, blob_dev, (const long long*)offsets_dev + b0, recs_dev + b0, nb, g, h->Ri,
                        mjps_sub_of(h->split, h->sub, h->Ri), frames_dev + b0 * fb, status_dev + b0);
    }
    if (rc) og_stream_drain(h);
    return rc;
}

int og_mjpd_decode_stream(og_mjpd* h, const uint8_t* blob, const int64_t* offsets, int B, uint8_t* frames_out_host_or_null,
                          uint8_t* frames_out_dev_or_null, size_t cap, int32_t* status, int* H, int* W) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (B < 0) return fail(OG_EINVAL, "bad B");
    OG_ALIGN(offsets);
    OG_ALIGN(status);
    OG_ALIGN(H);
    OG_ALIGN(W);
    if (!H || !W) return fail(OG_EINVAL, "H and W are null");
    if (B == 0) {
        *H = *W = 0;
        return OG_OK;
    }
    if (!blob || !offsets || !status) return fail(OG_EINVAL, "null buffer");
    if (!frames_out_host_or_null && !frames_out_dev_or_null) return fail(OG_EINVAL, "no place for the frames");
    MjpdCall call;
    int rc = mjpd_records(blob, offsets, B, &call);
    if (rc) return rc;
    if (call.sampling < 0) {   // every file refused: nothing to run
        for (int i = 0; i < B; ++i) status[i] = call.recs[i].status;
        *H = *W = 0;
        g_err = call.first_refusal;
        return OG_OK;
    }
    const int Hh = call.H, Ww = call.W;
    if ((unsigned long long)cap < (unsigned long long)B * Hh * Ww * 3)
        return fail(OG_EINVAL, "cap is below B * H * W * 3 = " + std::to_string((unsigned long long)B * Hh * Ww * 3) + " bytes");
    if ((rc = og_stream_ready(h))) return rc;
    OG_SCOPE(h);
    std::vector<MjpdTab> tabs(call.specs.size());
    for (size_t i = 0; i < tabs.size(); ++i) mjpd_build_tab(call.specs[i], &tabs[i]);
    if ((rc = mjpd_upload_tabs(h, tabs.data(), (int)tabs.size(), call.sampling, call.Ri))) return rc;
    MjpdForm g;
    mjpd_form(Hh, Ww, call.sampling, &g);
    const int nI = mjpd_intervals(g, call.Ri), chunk = mjpd_chunk(h->chunk, g, nI), cb = chunk < B ? chunk : B;
    const size_t fb = (size_t)Hh * Ww * 3;
    size_t in_max = 0;   // offsets, records and bytes of the largest micro-batch, the bytes kept 8-aligned by what precedes them
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = (B - b0 < chunk) ? B - b0 : chunk;
        in_max = std::max(in_max, (size_t)(nb + 1) * 8 + (size_t)nb * sizeof(og_mjpd_rec) + (size_t)(offsets[b0 + nb] - offsets[b0]));
    }
    const bool to_host = frames_out_host_or_null != nullptr, own_out = !frames_out_dev_or_null;
    if ((rc = h->d_ws.grow(h, (size_t)cb * mjpd_frame_ws(g, nI), "mjpd"))) return rc;
    if ((rc = h->d_in.grow(h, in_max, "mjpd"))) return rc;
    if (own_out && (rc = h->d_out.grow(h, cb * fb, "mjpd"))) return rc;
    if ((rc = h->d_status.grow(h, (size_t)cb * 4, "mjpd"))) return rc;
    for (auto& s : h->slots) {
        if ((rc = s.h_in.grow(h, in_max, "mjpd"))) return rc;
        if (to_host && (rc = s.h_out.grow(h, cb * fb, "mjpd"))) return rc;
        if ((rc = s.h_status.grow(h, (size_t)cb * 4, "mjpd"))) return rc;
        if (!s.ev) HIPCHK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    }
    const hipStream_t st = h->stream;

    auto retire = [&](og_mjpd::Slot& s) -> int {
        if (s.b0 < 0) return OG_OK;
        const int b0 = s.b0;
        s.b0 = -1;
        HIPCHK(hipEventSynchronize(s.ev));
        if (to_host) memcpy(frames_out_host_or_null + (size_t)b0 * fb, s.h_out, (size_t)s.nb * fb);
        memcpy(status + b0, s.h_status, (size_t)s.nb * 4);
        return OG_OK;
    };
    auto fill = [&](og_mjpd::Slot& s, int b0, int nb) -> int {
        long long* off = (long long*)s.h_in.p;
        og_mjpd_rec* recs = (og_mjpd_rec*)(s.h_in + (size_t)(nb + 1) * 8);
        uint8_t* bytes = (uint8_t*)(recs + nb);
        const size_t nbytes = (size_t)(offsets[b0 + nb] - offsets[b0]), head = (size_t)(bytes - s.h_in);
        for (int i = 0; i <= nb; ++i) off[i] = offsets[b0 + i] - offsets[b0];
        memcpy(recs, call.recs.data() + b0, (size_t)nb * sizeof(og_mjpd_rec));
        memcpy(bytes, blob + offsets[b0], nbytes);
        HIPCHK(hipMemcpyAsync(h->d_in, s.h_in, head + nbytes, hipMemcpyHostToDevice, st));
        uint8_t* dst = own_out ? h->d_out : frames_out_dev_or_null + (size_t)b0 * fb;
        const int rc2 = mjpd_batch(st, h->d_ws, h->d_tabs, h->nsets, h->d_in + head, (const long long*)h->d_in.p,
                                   (const og_mjpd_rec*)(h->d_in + (size_t)(nb + 1) * 8), nb, g, call.Ri, mjps_sub_of(h->split, h->sub, call.Ri), dst,
                                   h->d_status);
        if (rc2) return rc2;
        if (to_host) HIPCHK(hipMemcpyAsync(s.h_out, dst, (size_t)nb * fb, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(s.h_status, h->d_status, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(s.ev, st));
        s.b0 = b0;
        s.nb = nb;
        return OG_OK;
    };

    if ((rc = og_two_slot(B, chunk, h->slots, retire, fill, [h] { og_stream_drain(h); }))) return rc;
    *H = Hh;
    *W = Ww;
    if (!call.first_refusal.empty()) g_err = call.first_refusal;
    return OG_OK;
}

}  // extern "C"

namespace {
// og_mjpd_plan, and og_mjps_plan (og_mjps.inc) with a subsequence length
int mjpd_plan_text(int B, int H, int W, int sampling, int Ri, int chunk, int sub, char* out, size_t cap, long long* workspace_bytes) {
    if (!out || cap == 0 || B < 1) return fail(OG_EINVAL, "bad argument");
    int rc = check_mjpd_shape(H, W);
    if (rc) return rc;
    if (sampling < 0 || sampling > 3) return fail(OG_EINVAL, "sampling must be 0..3");
    if (Ri < 0 || Ri > 65535) return fail(OG_EINVAL, "Ri must be 0..65535");
    if ((rc = og_check_chunk(chunk, kMjpdMaxChunk))) return rc;
    MjpdForm g;
    mjpd_form(H, W, sampling, &g);
    const int nI = mjpd_intervals(g, Ri), mb = mjpd_chunk(chunk, g, nI), cb = mb < B ? mb : B;
    const long long fb = (long long)H * W * 3;
    if (workspace_bytes)
        *workspace_bytes = (long long)cb * mjpd_frame_ws(g, nI) + (long long)cb * (fb + 4 + 8 + (long long)sizeof(og_mjpd_rec)) + 8 +
                           (long long)sizeof(MjpdTab);
    const uintptr_t gap = (uintptr_t)1 << 40;   // placeholder bases: nothing dereferences them in a dry run
    uint8_t* frames = (uint8_t*)(1 * gap);
    int32_t* status = (int32_t*)(2 * gap);
    Plan plan;
    plan.bases = {{"frames", frames}, {"status", status}};
    g_plan = &plan;
    for (int b0 = 0; b0 < B && !rc; b0 += mb) {
        const int nb = (B - b0 < mb) ? B - b0 : mb;
        rc = mjpd_batch(nullptr, (uint8_t*)(3 * gap), (const MjpdTab*)(4 * gap), 1, (const uint8_t*)(5 * gap), (const long long*)(6 * gap),
                        (const og_mjpd_rec*)(7 * gap), nb, g, Ri, sub, frames + b0 * fb, status + b0);
    }
    g_plan = nullptr;
    if (rc) return rc;
    return og_plan_text(plan, kPlanWrites, out, cap);
}
}  // namespace

extern "C" {

int og_mjpd_plan(int B, int H, int W, int sampling, int Ri, int chunk, char* out, size_t cap, long long* workspace_bytes) {
    return mjpd_plan_text(B, H, W, sampling, Ri, chunk, 0, out, cap, workspace_bytes);
}
#endif   // OG_MJPD_HOST_ONLY

}  // extern "C"
