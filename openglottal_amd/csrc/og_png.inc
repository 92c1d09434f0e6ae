// PNG files decoded on the device (include_ext/openglottal_hip_png.h): the zlib stream of every file is inflated, unfiltered and
// expanded to [H,W,C] u8 pixels.  Included by og_api.hip after og_mjps.inc; the kernels live here too.  A handle of its own: one
// stream, the workspace of ONE micro-batch, two pinned host slots.  Per micro-batch: k_png_inflate (a wave per file: raw bytes),
// k_png_unfilter (a wave per file: Adler-32, filter types, rows in place), k_png_expand (a lane per pixel).  The host twin and the
// kernels call the same inline functions and agree byte for byte and status for status.
// With OG_PNG_HOST_ONLY defined the file is a translation unit of its own for a host compiler: the parser and the twin, no HIP
// (tools/png_host_fuzz.cpp builds it under sanitizers).
#include "../../include_ext/openglottal_hip_png.h"

#ifdef OG_PNG_HOST_ONLY
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#define OG_PNG_HD inline
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
}  // namespace
extern "C" const char* og_last_error(void) { return g_err.c_str(); }
#else
#define OG_PNG_HD __host__ __device__ __forceinline__
#endif

constexpr long long kPngMaxFile = 1ll << 30;
constexpr int kPngMaxChunk = 1024;
constexpr int kPngStatusMax = 7;
constexpr int kPngWindow = 32768;
constexpr int kPngMaxPalettes = 65535;
constexpr uint32_t kAdlerMod = 65521;
static_assert(sizeof(og_png_rec) == 40 && sizeof(og_png_info) == 56, "layouts stated in the header");

// the code tables of one block and the scratch of their construction: per wave in LDS, on the stack in the twin
struct OgInfTab {
    uint16_t lcnt[16], lsym[288];   // literal / length code: codes per length, symbols in canonical order
    uint16_t dcnt[16], dsym[32];    // distance code (and, while a dynamic header is read, the code-length code)
    uint16_t offs[16];
    uint8_t lens[320];
};

// ---- the arithmetic: host twin and kernels ---------------------------------------------------------------------------------------
struct OgInfBits {
    const uint8_t* p;
    long long n, i;   // bytes of the stream, the next one to read
    uint64_t acc;     // the low nb bits are the bits not yet consumed, the next one lowest; the bits above them are 0
    int nb;
};

// tops the bit buffer up to more than 56 bits; reads p[i] only for i < n
OG_PNG_HD void og_inf_fill(OgInfBits& s) {
    for (; s.nb <= 56 && s.i < s.n;) {
        s.acc |= (uint64_t)s.p[s.i++] << s.nb;
        s.nb += 8;
    }
}

// the next k bits (0..16); *st = 1 if they are not there
OG_PNG_HD uint32_t og_inf_take(OgInfBits& s, int k, int* st) {
    og_inf_fill(s);
    if (s.nb < k) {
        *st = 1;
        return 0;
    }
    const uint32_t v = (uint32_t)(s.acc & ((1ull << k) - 1));
    s.acc >>= k;
    s.nb -= k;
    return v;
}

// Canonical tables of n code lengths (0: unused): cnt[len] codes of each length, sym in code order.  Returns what is left of the
// code space: 0 complete, > 0 incomplete, < 0 over-subscribed (then sym is not filled).  *ncodes: lengths that are not 0.
OG_PNG_HD int og_inf_build(const uint8_t* lens, int n, uint16_t* cnt, uint16_t* sym, uint16_t* offs, int* ncodes) {
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    for (int s = 0; s < n; ++s) cnt[lens[s] & 15] = (uint16_t)(cnt[lens[s] & 15] + 1);
    *ncodes = n - cnt[0];
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        left = 2 * left - cnt[l];
        if (left < 0) return left;
    }
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
    for (int s = 0; s < n; ++s)
        if (lens[s] & 15) {
            const int l = lens[s] & 15;
            sym[offs[l]] = (uint16_t)s;
            offs[l] = (uint16_t)(offs[l] + 1);
        }
    return left;
}

// one symbol of a canonical code; -1: the bits ended inside it, -2: 15 bits that are no code
OG_PNG_HD int og_inf_sym(OgInfBits& s, const uint16_t* cnt, const uint16_t* sym) {
    og_inf_fill(s);
    uint32_t bits = (uint32_t)s.acc;
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {
        code |= (int)(bits & 1);
        bits >>= 1;
        const int count = cnt[len];
        if (code - count < first) {
            if (len > s.nb) return -1;
            s.acc >>= len;
            s.nb -= len;
            return sym[index + (code - first)];
        }
        index += count;
        first = (first + count) << 1;
        code <<= 1;
    }
    return s.nb < 15 ? -1 : -2;
}

// len bytes at pos by LANES lanes: byte i is src(i), stored to the window and to out
#define OG_INF_COPY(len, src)                                   \
    for (int i_ = lane; i_ < (len); i_ += LANES) {              \
        const uint8_t b_ = (src);                               \
        ring[(pos + i_) & (kPngWindow - 1)] = b_;               \
        out[pos + i_] = b_;                                     \
    }

// One zlib stream: in[0, n) -> out[0, cap).  Every lane of a wave calls it with the same arguments and its own `lane` (the twin:
// LANES 1, lane 0); all state is the same in every lane, only the stores are divided.  Returns the status 0..5 without the Adler
// comparison: *produced bytes were written, *adler is the trailer's value.  See SAFETY in the header.
template <int LANES>
OG_PNG_HD int og_png_zlib(const uint8_t* in, long long n, uint8_t* out, long long cap, OgInfTab* t, uint8_t* ring, int lane,
                          long long* produced, uint32_t* adler) {
    *produced = 0;
    *adler = 0;
    if (n < 2) return 1;
    const int cmf = in[0], flg = in[1];
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 32)) return 5;
    OgInfBits s{in, n, 2, 0, 0};
    long long pos = 0;
    int st = 0;
    for (int last = 0; !last;) {
        last = (int)og_inf_take(s, 1, &st);
        const int type = (int)og_inf_take(s, 2, &st);
        if (st) return st;
        if (type == 3) return 2;
        if (type == 0) {
            og_inf_take(s, s.nb & 7, &st);   // to the byte boundary (after a fill nb & 7 is what the last byte has left)
            const uint32_t len = og_inf_take(s, 16, &st), nlen = og_inf_take(s, 16, &st);
            if (st) return st;
            if ((len ^ nlen) != 0xFFFF) return 2;
            s.i -= s.nb >> 3;   // hand the whole bytes of the buffer back: the block is copied from the stream itself
            s.acc = 0;
            s.nb = 0;
            const long long avail = s.n - s.i, room = cap - pos;
            if (avail < (long long)len && avail <= room) return 1;
            if (room < (long long)len) return 4;
            OG_INF_COPY((int)len, in[s.i + i_])
            s.i += len;
            pos += len;
            *produced = pos;
            continue;
        }
        int ncodes = 0, dist_codes = 0;
        if (type == 1) {
            for (int i = 0; i < 288; ++i) t->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
            og_inf_build(t->lens, 288, t->lcnt, t->lsym, t->offs, &ncodes);
            for (int i = 0; i < 32; ++i) t->lens[i] = 5;
            og_inf_build(t->lens, 32, t->dcnt, t->dsym, t->offs, &dist_codes);
        } else {
            const int hlit = (int)og_inf_take(s, 5, &st) + 257, hdist = (int)og_inf_take(s, 5, &st) + 1, hclen = (int)og_inf_take(s, 4, &st) + 4;
            if (st) return st;
            if (hlit > 286 || hdist > 30) return 2;
            // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
            const uint64_t order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                                      5ull << 45 | 11ull << 50 | 4ull << 55;
            const uint64_t order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
            for (int i = 0; i < 19; ++i) t->lens[i] = 0;
            for (int i = 0; i < hclen; ++i) {
                const int k = (int)((i < 12 ? order_lo >> (5 * i) : order_hi >> (5 * (i - 12))) & 31);
                t->lens[k] = (uint8_t)og_inf_take(s, 3, &st);
            }
            if (st) return st;
            if (og_inf_build(t->lens, 19, t->dcnt, t->dsym, t->offs, &ncodes) != 0) return 2;
            const int total = hlit + hdist;
            for (int idx = 0; idx < total;) {
                const int sym = og_inf_sym(s, t->dcnt, t->dsym);
                if (sym < 0) return -sym;
                if (sym < 16) {
                    t->lens[idx++] = (uint8_t)sym;
                    continue;
                }
                int prev = 0, rep;
                if (sym == 16) {
                    if (idx == 0) return 2;
                    prev = t->lens[idx - 1];
                    rep = 3 + (int)og_inf_take(s, 2, &st);
                } else if (sym == 17) {
                    rep = 3 + (int)og_inf_take(s, 3, &st);
                } else {
                    rep = 11 + (int)og_inf_take(s, 7, &st);
                }
                if (st) return st;
                if (idx + rep > total) return 2;
                for (; rep > 0; --rep) t->lens[idx++] = (uint8_t)prev;
            }
            if (t->lens[256] == 0) return 2;
            if (og_inf_build(t->lens, hlit, t->lcnt, t->lsym, t->offs, &ncodes) != 0) return 2;
            const int left = og_inf_build(t->lens + hlit, hdist, t->dcnt, t->dsym, t->offs, &dist_codes);
            if (left < 0 || (left > 0 && dist_codes != 0 && !(dist_codes == 1 && t->dcnt[1] == 1))) return 2;
        }
        for (;;) {
            int sym = og_inf_sym(s, t->lcnt, t->lsym);
            if (sym < 0) return -sym;
            if (sym < 256) {
                if (pos >= cap) return 4;
                if (lane == 0) {
                    ring[pos & (kPngWindow - 1)] = (uint8_t)sym;
                    out[pos] = (uint8_t)sym;
                }
                pos += 1;
                continue;
            }
            if (sym == 256) break;
            if (sym >= 286) return 2;
            sym -= 257;
            const int lext = sym < 8 || sym == 28 ? 0 : (sym - 4) >> 2;
            const int len = (sym < 8 ? 3 + sym : sym == 28 ? 258 : 3 + ((4 + (sym & 3)) << lext)) + (int)og_inf_take(s, lext, &st);
            if (st) return st;
            const int ds = og_inf_sym(s, t->dcnt, t->dsym);
            if (ds < 0) return -ds;
            if (ds >= 30) return 2;
            const int dext = ds < 4 ? 0 : (ds - 2) >> 1;
            const int dist = (ds < 4 ? 1 + ds : 1 + ((2 + (ds & 1)) << dext)) + (int)og_inf_take(s, dext, &st);
            if (st) return st;
            if (dist > pos) return 3;
            if (pos + len > cap) return 4;
            OG_INF_COPY(len, ring[(pos - dist + (i_ % dist)) & (kPngWindow - 1)])
            pos += len;
        }
        *produced = pos;
    }
    og_inf_take(s, s.nb & 7, &st);
    uint32_t a = 0;
    for (int k = 0; k < 4; ++k) a = (a << 8) | og_inf_take(s, 8, &st);
    if (st) return st;
    *adler = a;
    return 0;
}

// Adler-32 in parts: lane's share of s1 = sum d[i] and s2 = sum (N - i) d[i], both below 65521
template <int LANES>
OG_PNG_HD void og_png_adler_part(const uint8_t* p, long long N, int lane, uint32_t* s1, uint32_t* s2) {
    uint64_t a = 0, b = 0;
    for (long long i = lane; i < N; i += LANES) {
        const uint32_t d = p[i];
        a += d;
        b += (uint64_t)(uint32_t)((N - i) % kAdlerMod) * d;
    }
    *s1 = (uint32_t)(a % kAdlerMod);
    *s2 = (uint32_t)(b % kAdlerMod);
}
// from the sums of all parts (each sum below 2^32)
OG_PNG_HD uint32_t og_png_adler_join(uint32_t s1, uint32_t s2, long long N) {
    const uint32_t a = (1 + s1 % kAdlerMod) % kAdlerMod, b = (uint32_t)((N % kAdlerMod + s2 % kAdlerMod) % kAdlerMod);
    return (b << 16) | a;
}

// one byte of a scanline: x the filtered byte, a left, b up, c up-left
OG_PNG_HD int og_png_recon(int ft, int x, int a, int b, int c) {
    int pred = 0;
    if (ft == 1) pred = a;
    else if (ft == 2) pred = b;
    else if (ft == 3) pred = (a + b) >> 1;
    else if (ft == 4) {
        const int p = a + b - c;
        const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
        pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    }
    return (x + pred) & 255;
}

OG_PNG_HD int og_png_samples(int ctype) { return ctype == 0 || ctype == 3 ? 1 : ctype == 2 ? 3 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0; }
OG_PNG_HD bool og_png_form_ok(int ctype, int depth) {
    if (ctype == 0 || ctype == 3) return depth == 1 || depth == 2 || depth == 4 || depth == 8;
    return (ctype == 2 || ctype == 4 || ctype == 6) && depth == 8;
}
// bytes of a scanline (for a form og_png_form_ok accepts and W <= 2^24: below 2^26)
OG_PNG_HD long long og_png_rb(int W, int ctype, int depth) { return ((long long)W * og_png_samples(ctype) * depth + 7) >> 3; }
OG_PNG_HD int og_png_bpp(int ctype, int depth) {
    const int v = og_png_samples(ctype) * depth / 8;
    return v < 1 ? 1 : v;
}
OG_PNG_HD int og_png_gray3(const uint8_t* bgr) {
#ifdef OG_PNG_HOST_ONLY
    return (bgr[0] * 3735 + bgr[1] * 19235 + bgr[2] * 9798 + (1 << 14)) >> 15;
#else
    return og_gray_at<3>(bgr, 0);
#endif
}

// pixel x of an unfiltered row (the byte after its filter type first) -> C bytes.  pal: 768 bytes, or anything for other types.
OG_PNG_HD void og_png_pixel(const uint8_t* row, int x, int ctype, int depth, const uint8_t* pal, int C, uint8_t* px) {
    uint8_t bgr[3];
    if (ctype == 0 || ctype == 3) {
        int s;
        if (depth == 8) {
            s = row[x];
        } else {
            const long long bit = (long long)x * depth;
            s = (row[bit >> 3] >> (8 - depth - (int)(bit & 7))) & ((1 << depth) - 1);
        }
        if (ctype == 0) {
            bgr[0] = bgr[1] = bgr[2] = (uint8_t)(s * (255 / ((1 << depth) - 1)));
        } else {
            bgr[0] = pal[3 * s + 2];
            bgr[1] = pal[3 * s + 1];
            bgr[2] = pal[3 * s];
        }
    } else if (ctype == 4) {
        bgr[0] = bgr[1] = bgr[2] = row[2ll * x];
    } else {
        const uint8_t* p = row + (long long)x * (ctype == 6 ? 4 : 3);
        bgr[0] = p[2];
        bgr[1] = p[1];
        bgr[2] = p[0];
    }
    if (C == 3) {
        px[0] = bgr[0];
        px[1] = bgr[1];
        px[2] = bgr[2];
    } else {
        px[0] = (ctype == 0 || ctype == 4) ? bgr[0] : (uint8_t)og_png_gray3(bgr);
    }
}

// the pixels of a record lie inside the output
OG_PNG_HD bool og_png_out_ok(const og_png_rec& r, int C, long long cap) {
    if (r.H <= 0 || r.W <= 0 || (long long)r.H * r.W > kMjpegMaxPixels) return false;
    return r.out_offset >= 0 && r.out_offset <= cap && (long long)r.H * r.W * C <= cap - r.out_offset;
}
// the file's status from the record the host made and the extents of the call; 0: the stream may be inflated
OG_PNG_HD int og_png_rec_status(const og_png_rec& r, long long zsize, int npals, int C, long long raw_bytes, long long cap) {
    if (r.status) return r.status > 0 && r.status <= kPngStatusMax ? r.status : 6;
    if (!og_png_out_ok(r, C, cap) || !og_png_form_ok(r.ctype, r.depth)) return 6;
    const long long raw = (long long)r.H * (1 + og_png_rb(r.W, r.ctype, r.depth));
    if (r.raw_offset < 0 || r.raw_offset > raw_bytes || raw > raw_bytes - r.raw_offset) return 6;
    if (r.ctype == 3 && (r.palette < 0 || r.palette >= npals)) return 6;
    if (zsize < 0 || zsize > kPngMaxFile) return 6;
    return 0;
}

#ifndef OG_PNG_HOST_ONLY
// ---- kernels ---------------------------------------------------------------------------------------------------------------------
// A wave per file.  raw: the micro-batch's raw bytes; adler [file]: the trailer's value.
__global__ __launch_bounds__(64) void k_png_inflate(const uint8_t* __restrict__ zblob, const long long* __restrict__ zoffsets,
                                                    const og_png_rec* __restrict__ recs, int npals, int C, long long raw_bytes, long long cap,
                                                    uint8_t* __restrict__ raw, uint32_t* __restrict__ adler, int32_t* __restrict__ status) {
    __shared__ OgInfTab s_tab;
    __shared__ uint8_t s_ring[kPngWindow];
    const int f = blockIdx.x, lane = threadIdx.x;
    const og_png_rec rec = recs[f];
    const long long z0 = zoffsets[f], zsize = zoffsets[f + 1] - z0;
    int st = og_png_rec_status(rec, zsize, npals, C, raw_bytes, cap);
    uint32_t want = 0;
    if (!st) {
        const long long need = (long long)rec.H * (1 + og_png_rb(rec.W, rec.ctype, rec.depth));
        long long produced = 0;
        st = og_png_zlib<64>(zblob + z0, zsize, raw + rec.raw_offset, need, &s_tab, s_ring, lane, &produced, &want);
        if (!st && produced < need) st = 1;
    }
    if (lane == 0) {
        status[f] = st;
        adler[f] = want;
    }
}

// A wave per file, in place: Adler-32, the filter types, then bands of 64 rows.
__global__ __launch_bounds__(64) void k_png_unfilter(const og_png_rec* __restrict__ recs, uint8_t* __restrict__ raw,
                                                     const uint32_t* __restrict__ adler, int32_t* __restrict__ status) {
    const int f = blockIdx.x, lane = threadIdx.x;
    if (status[f] != 0) return;   // (k_png_inflate held the record to the workspace)
    const og_png_rec rec = recs[f];
    const int H = rec.H, rb = (int)og_png_rb(rec.W, rec.ctype, rec.depth), bpp = og_png_bpp(rec.ctype, rec.depth);
    const long long stride = 1 + (long long)rb, N = (long long)H * stride;
    uint8_t* base = raw + rec.raw_offset;
    uint32_t s1, s2;
    og_png_adler_part<64>(base, N, lane, &s1, &s2);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    if (og_png_adler_join(s1, s2, N) != adler[f]) {
        if (lane == 0) status[f] = 5;
        return;
    }
    bool bad = false;
    for (int r = lane; r < H; r += 64) bad |= base[r * stride] > 4;
    if (__any(bad)) {
        if (lane == 0) status[f] = 7;
        return;
    }
    for (int band = 0; band < H; band += 64) {
        const int r = band + lane;
        const bool active = r < H;
        uint8_t* cur = base + (active ? r : band) * stride + 1;
        const uint8_t* above = cur - stride;   // read by lane 0 only, and only when band > 0
        const int ft = active ? cur[-1] : 0;
        int qa0 = 0, qa1 = 0, qa2 = 0, qa3 = 0, qb0 = 0, qb1 = 0, qb2 = 0, qb3 = 0, mine = 0;
        for (int t = 0; t < rb + 63; ++t) {
            const int x = t - lane;
            const int up = __shfl_up(mine, 1);
            if (active && x >= 0 && x < rb) {
                const int b = lane == 0 ? (band ? above[x] : 0) : up;
                const int a = bpp == 1 ? qa0 : bpp == 2 ? qa1 : bpp == 3 ? qa2 : qa3;
                const int c = bpp == 1 ? qb0 : bpp == 2 ? qb1 : bpp == 3 ? qb2 : qb3;
                mine = og_png_recon(ft, cur[x], a, b, c);
                cur[x] = (uint8_t)mine;
                qa3 = qa2; qa2 = qa1; qa1 = qa0; qa0 = mine;
                qb3 = qb2; qb2 = qb1; qb1 = qb0; qb0 = b;
            }
        }
        __threadfence_block();   // the band's last row is the next band's row above: lane 63's stores before lane 0's loads
    }
}

// A lane per pixel: grid (x, files); a file larger than the grid's x extent is walked in strides.
__global__ __launch_bounds__(256) void k_png_expand(const og_png_rec* __restrict__ recs, const uint8_t* __restrict__ pals, int C, long long cap,
                                                    const uint8_t* __restrict__ raw, const int32_t* __restrict__ status, uint8_t* __restrict__ out) {
    const int f = blockIdx.y;
    const og_png_rec rec = recs[f];
    const int st = status[f];
    if (!og_png_out_ok(rec, C, cap)) return;   // (a refused file has no size; status 0: k_png_inflate held the record to the workspace too)
    const long long HW = (long long)rec.H * rec.W, stride = 1 + og_png_rb(rec.W, rec.ctype, rec.depth);
    const uint8_t* pal = pals + 768ll * (rec.ctype == 3 && st == 0 ? rec.palette : 0);
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < HW; idx += (long long)gridDim.x * 256) {
        uint8_t px[3] = {0, 0, 0};
        if (st == 0) {
            const int y = (int)(idx / rec.W), x = (int)(idx - (long long)y * rec.W);
            og_png_pixel(raw + rec.raw_offset + y * stride + 1, x, rec.ctype, rec.depth, pal, C, px);
        }
        uint8_t* dst = out + rec.out_offset + idx * C;
        dst[0] = px[0];
        if (C == 3) {
            dst[1] = px[1];
            dst[2] = px[2];
        }
    }
}
#endif   // OG_PNG_HOST_ONLY

// ---- host side -------------------------------------------------------------------------------------------------------------------
#ifndef OG_PNG_HOST_ONLY
struct og_png : OgStreamHandle {
    OgBuf<uint8_t> d_pals;
    int npals = -1;           // what d_pals holds; -1: og_png_set_palettes has not been called
    // each buffer holds the bytes of the largest micro-batch run so far
    OgBuf<uint8_t> d_ws;      // raw bytes, then the stored Adler-32 of every file
    OgBuf<uint8_t> d_in;      // streamed entry: offsets, records, zlib bytes
    OgBuf<uint8_t> d_out;     // streamed entry: pixels, unless the caller's device buffer takes them
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

struct PngParsed {
    og_png_info info;
    std::vector<std::pair<size_t, size_t>> idat;   // payload offset and length of every IDAT
    uint8_t pal[768];
};

int png_refuse(og_png_info* info, const std::string& why) {
    info->status = 6;
    g_err = "unsupported PNG: " + why;
    return 6;
}

uint32_t png_crc32(const uint8_t* p, size_t n) {
    static const std::vector<uint32_t> table = [] {
        std::vector<uint32_t> t(256);
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[i] = c;
        }
        return t;
    }();
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 255] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

uint32_t png_be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// The chunks of one file.  Returns 0 or 6; the reason of a refusal goes to g_err.  Reads png[i] only for i < size.
int png_parse(const uint8_t* png, size_t size, PngParsed* out) {
    out->info = og_png_info{};
    out->idat.clear();
    memset(out->pal, 0, sizeof out->pal);
    og_png_info* info = &out->info;
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    if (size > (size_t)kPngMaxFile) return png_refuse(info, "the file is above 2^30 bytes");
    if (size < 8 || memcmp(png, sig, 8) != 0) return png_refuse(info, "no PNG signature");
    bool ihdr = false, plte = false;
    for (size_t pos = 8;;) {
        const bool header = size - pos >= 8;
        const size_t len = header ? png_be32(png + pos) : 0;
        const bool whole = header && len <= size - pos - 8 && size - pos - 8 - len >= 4;
        const bool is_idat = header && memcmp(png + pos + 4, "IDAT", 4) == 0;
        if (!out->idat.empty() && !is_idat) break;   // the IDAT run has ended: nothing after it is required
        if (!whole) {
            if (pos == size && ihdr) return png_refuse(info, "no IDAT chunk");
            return png_refuse(info, "a chunk that leaves the file at byte " + std::to_string(pos));
        }
        const uint8_t* type = png + pos + 4;
        const uint8_t* data = type + 4;
        if (png_crc32(type, 4 + len) != png_be32(data + len)) return png_refuse(info, "a bad CRC in the chunk at byte " + std::to_string(pos));
        if (!ihdr) {
            if (memcmp(type, "IHDR", 4) != 0 || len != 13) return png_refuse(info, "the first chunk is not an IHDR of 13 bytes");
            ihdr = true;
            const uint32_t W = png_be32(data), H = png_be32(data + 4);
            const int depth = data[8], ctype = data[9];
            if (H == 0 || W == 0) return png_refuse(info, "H or W of 0");
            if (H > (uint32_t)kMjpegMaxPixels || W > (uint32_t)kMjpegMaxPixels || (long long)H * W > kMjpegMaxPixels)
                return png_refuse(info, "H * W above " + std::to_string(kMjpegMaxPixels) + " pixels");
            info->H = (int32_t)H;
            info->W = (int32_t)W;
            info->ctype = ctype;
            info->depth = depth;
            if (depth == 16) return png_refuse(info, "16-bit samples");
            if (!og_png_form_ok(ctype, depth)) return png_refuse(info, "colour type " + std::to_string(ctype) + " at depth " + std::to_string(depth));
            if (data[10] != 0) return png_refuse(info, "compression method " + std::to_string((int)data[10]));
            if (data[11] != 0) return png_refuse(info, "filter method " + std::to_string((int)data[11]));
            if (data[12] == 1) return png_refuse(info, "Adam7 interlace");
            if (data[12] != 0) return png_refuse(info, "interlace method " + std::to_string((int)data[12]));
            info->samples = og_png_samples(ctype);
            info->rb = (int32_t)og_png_rb(info->W, ctype, depth);
            info->bpp = og_png_bpp(ctype, depth);
            info->raw_bytes = (int64_t)info->H * (1 + (int64_t)info->rb);
        } else if (memcmp(type, "IHDR", 4) == 0) {
            return png_refuse(info, "a second IHDR");
        } else if (memcmp(type, "PLTE", 4) == 0) {
            if (plte) return png_refuse(info, "a second PLTE");
            if (len == 0 || len % 3 != 0 || len > 768) return png_refuse(info, "a PLTE of " + std::to_string(len) + " bytes");
            plte = true;
            if (info->ctype == 3) {
                memcpy(out->pal, data, len);
                info->npal = (int32_t)(len / 3);
            }
        } else if (is_idat) {
            if (info->ctype == 3 && !plte) return png_refuse(info, "a palette file without PLTE before IDAT");
            out->idat.push_back({(size_t)(data - png), len});
            info->zlib_bytes += (int64_t)len;
            info->nidat += 1;
        } else if (memcmp(type, "IEND", 4) == 0) {
            return png_refuse(info, "no IDAT chunk");
        } else if (!(type[0] & 32)) {
            return png_refuse(info, "an unknown critical chunk at byte " + std::to_string(pos));
        }
        pos += 12 + len;
    }
    return 0;
}

std::vector<uint8_t> png_join(const uint8_t* png, const PngParsed& p) {
    std::vector<uint8_t> z;
    z.reserve((size_t)p.info.zlib_bytes + 1);
    for (const auto& c : p.idat) z.insert(z.end(), png + c.first, png + c.first + c.second);
    return z;
}

// the twin of the three launches on one accepted file: status and H * W * C bytes
int png_file_host(const og_png_info& info, const uint8_t* z, size_t zn, const uint8_t* pal, int C, uint8_t* out) {
    const long long stride = 1 + (long long)info.rb, N = info.raw_bytes;
    const size_t px = (size_t)info.H * info.W * C;
    std::vector<uint8_t> raw((size_t)N), ring(kPngWindow);
    OgInfTab tab;
    long long produced = 0;
    uint32_t want = 0;
    int st = og_png_zlib<1>(z, (long long)zn, raw.data(), N, &tab, ring.data(), 0, &produced, &want);
    if (!st && produced < N) st = 1;
    if (!st) {
        uint32_t s1, s2;
        og_png_adler_part<1>(raw.data(), N, 0, &s1, &s2);
        if (og_png_adler_join(s1, s2, N) != want) st = 5;
    }
    for (int r = 0; r < info.H && !st; ++r)
        if (raw[(size_t)(r * stride)] > 4) st = 7;
    if (st) {
        memset(out, 0, px);
        return st;
    }
    for (int r = 0; r < info.H; ++r) {
        uint8_t* cur = raw.data() + r * stride + 1;
        const uint8_t* above = cur - stride;
        const int ft = cur[-1];
        for (int x = 0; x < info.rb; ++x)
            cur[x] = (uint8_t)og_png_recon(ft, cur[x], x >= info.bpp ? cur[x - info.bpp] : 0, r ? above[x] : 0, (r && x >= info.bpp) ? above[x - info.bpp] : 0);
    }
    for (int y = 0; y < info.H; ++y)
        for (int x = 0; x < info.W; ++x)
            og_png_pixel(raw.data() + y * stride + 1, x, info.ctype, info.depth, pal, C, out + ((size_t)y * info.W + x) * C);
    return 0;
}

// B files: what the parser found, the records with dense offsets, the distinct palettes
struct PngCall {
    std::vector<PngParsed> files;
    std::vector<og_png_rec> recs;
    std::vector<uint8_t> pals;   // 768 bytes each
    long long out_total = 0, raw_total = 0, max_pixels = 0;
    std::string first_refusal;
};
int png_records(const uint8_t* blob, const int64_t* offsets, int B, int C, PngCall* call) {
    call->files.resize((size_t)B);
    call->recs.assign((size_t)B, og_png_rec{0, 0, 0, 0, 0, 0, 0, 0});
    for (int i = 0; i < B; ++i) {
        if (offsets[i] < 0 || offsets[i + 1] < offsets[i]) return fail(OG_EINVAL, "offsets must not be negative or decrease");
        og_png_rec& r = call->recs[i];
        PngParsed& p = call->files[i];
        r.out_offset = call->out_total;
        r.raw_offset = call->raw_total;
        if (png_parse(blob + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), &p)) {
            r.status = 6;
            if (call->first_refusal.empty()) call->first_refusal = g_err;
            continue;
        }
        r.H = p.info.H;
        r.W = p.info.W;
        r.ctype = p.info.ctype;
        r.depth = p.info.depth;
        if (r.ctype == 3) {
            int set = -1;
            const int have = (int)(call->pals.size() / 768);
            for (int j = have - 1; j >= 0 && set < 0; --j)
                if (!memcmp(call->pals.data() + 768 * (size_t)j, p.pal, 768)) set = j;
            if (set < 0) {
                if (have >= kPngMaxPalettes) return fail(OG_EINVAL, "more than " + std::to_string(kPngMaxPalettes) + " distinct palettes in one call");
                set = have;
                call->pals.insert(call->pals.end(), p.pal, p.pal + 768);
            }
            r.palette = set;
        }
        call->out_total += (long long)r.H * r.W * C;
        call->raw_total += p.info.raw_bytes;
        call->max_pixels = std::max(call->max_pixels, (long long)r.H * r.W);
    }
    return OG_OK;
}

int check_png_channels(int C) { return C == 3 || C == 1 ? OG_OK : fail(OG_EINVAL, "channels must be 3 (B G R) or 1 (gray)"); }

// where the micro-batch that starts at b0 ends: at most `chunk` files, and at most 256 MiB of raw bytes once it holds a file
int png_batch_end(const long long* raw_sizes, int b0, int B, int chunk) {
    long long sum = 0;
    int e = b0;
    for (; e < B && e - b0 < chunk; ++e) {
        if (e > b0 && sum + raw_sizes[e] > kMjpegBatchBytes) break;
        sum += raw_sizes[e];
    }
    return e;
}

#ifndef OG_PNG_HOST_ONLY
void png_free(og_png* h) {
    og_release(h->d_pals, h->d_ws, h->d_in, h->d_out, h->d_status);
    for (auto& s : h->slots) {
        og_release(s.h_in, s.h_out, s.h_status);
        if (s.ev) (void)hipEventDestroy(s.ev);
    }
}

int png_upload_pals(og_png* h, const uint8_t* pals, int npals) {
    h->npals = -1;
    int rc = h->d_pals.grow(h, (size_t)(npals ? npals : 1) * 768, "png");
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));   // (launches in flight read the old palettes; the pageable source must outlive the copy)
    if (npals) HIPCHK(hipMemcpy(h->d_pals, pals, (size_t)npals * 768, hipMemcpyHostToDevice));
    h->npals = npals;
    return OG_OK;
}

long long png_ws_bytes(long long raw_bytes, int nb) { return ((raw_bytes + 3) & ~3ll) + 4ll * nb; }

// One micro-batch of nb resident files whose raw bytes take raw_bytes.  ws: the handle's workspace (a placeholder in a dry run).
int png_batch(hipStream_t st, uint8_t* ws, const uint8_t* pals, int npals, const uint8_t* zblob, const long long* zoffsets, const og_png_rec* recs,
              int nb, int C, long long raw_bytes, long long max_pixels, uint8_t* out, long long cap, long long out_bytes, int32_t* status) {
    uint32_t* adler = (uint32_t*)(ws + ((raw_bytes + 3) & ~3ll));
    plan_need(png_ws_bytes(raw_bytes, nb), 0);
    OG_LAUNCH(k_png_inflate, dim3((unsigned)nb), dim3(64), 0, st, zblob, zoffsets, recs, npals, C, raw_bytes, cap, ws, adler, status);
    if (g_plan) {
        g_plan->recs.back().lds = (unsigned)(sizeof(OgInfTab) + kPngWindow);   // static LDS: stated, so that the plan tells the truth
        plan_write("status", status, (long long)nb * 4);
    }
    OG_LAUNCH(k_png_unfilter, dim3((unsigned)nb), dim3(64), 0, st, recs, ws, (const uint32_t*)adler, status);
    if (g_plan) plan_write("status", status, (long long)nb * 4);
    const long long gx = (std::max(max_pixels, 1ll) + 255) / 256;
    OG_LAUNCH(k_png_expand, dim3((unsigned)gx, (unsigned)nb), dim3(256), 0, st, recs, pals, C, cap, (const uint8_t*)ws, (const int32_t*)status, out);
    if (g_plan) plan_write("out", out, out_bytes);
    return OG_OK;
}
#endif   // OG_PNG_HOST_ONLY

}  // namespace

extern "C" {

long long og_png_limit(int which) {
    switch (which) {
        case 0: return kMjpegMaxPixels;
        case 1: return kPngMaxChunk;
        case 2: return (long long)sizeof(og_png_rec);
        case 3: return 768;
        case 4: return kPngStatusMax;
        case 5: return kPngMaxFile;
        case 6: return 128;
        case 7: return kPngWindow;
        default: return -1;
    }
}

int og_pngd_parse_host(const uint8_t* png, size_t size, og_png_info* info) {
    if (!png || !info) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(info);
    PngParsed p;
    png_parse(png, size, &p);
    *info = p.info;
    return OG_OK;
}

int og_pngd_inflate_host(const uint8_t* zlib_stream, size_t size, uint8_t* out, size_t cap, size_t* produced, int* status) {
    if (!zlib_stream || !out || !produced || !status) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(produced);
    OG_ALIGN(status);
    if (size > (size_t)kPngMaxFile) return fail(OG_EINVAL, "the stream is above 2^30 bytes");
    if (cap > (size_t)1 << 40) return fail(OG_EINVAL, "cap is above 2^40 bytes");
    OgInfTab tab;
    std::vector<uint8_t> ring(kPngWindow);
    long long n = 0;
    uint32_t want = 0;
    int st = og_png_zlib<1>(zlib_stream, (long long)size, out, (long long)cap, &tab, ring.data(), 0, &n, &want);
    if (!st) {
        uint32_t s1, s2;
        og_png_adler_part<1>(out, n, 0, &s1, &s2);
        if (og_png_adler_join(s1, s2, n) != want) st = 5;
    }
    *produced = (size_t)n;
    *status = st;
    return OG_OK;
}

int og_pngd_decode_host(const uint8_t* png, size_t size, int channels, uint8_t* out, size_t cap, int* status) {
    if (!png || !out || !status) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(status);
    int rc = check_png_channels(channels);
    if (rc) return rc;
    PngParsed p;
    if (png_parse(png, size, &p)) {
        *status = 6;
        return OG_OK;
    }
    const unsigned long long need = (unsigned long long)p.info.H * p.info.W * channels;
    if ((unsigned long long)cap < need) return fail(OG_EINVAL, "cap is below H * W * channels = " + std::to_string(need) + " bytes");
    const std::vector<uint8_t> z = png_join(png, p);
    *status = png_file_host(p.info, z.data(), z.size(), p.pal, channels, out);
    return OG_OK;
}

int og_pngd_records_host(const uint8_t* blob, const int64_t* offsets, int B, int channels, og_png_rec* recs, uint8_t* zblob, size_t zcap,
                         int64_t* zoffsets, uint8_t* pals, int pals_cap, int* npals, int64_t* totals) {
    if (B < 0 || pals_cap < 0) return fail(OG_EINVAL, "bad B");
    int rc = check_png_channels(channels);
    if (rc) return rc;
    if (!npals || !totals || !zoffsets) return fail(OG_EINVAL, "null result");
    OG_ALIGN(offsets);
    OG_ALIGN(recs);
    OG_ALIGN(zoffsets);
    OG_ALIGN(npals);
    OG_ALIGN(totals);
    if (B > 0 && (!blob || !offsets || !recs || !zblob || !pals)) return fail(OG_EINVAL, "null buffer");
    PngCall call;
    if (B && (rc = png_records(blob, offsets, B, channels, &call))) return rc;
    if ((int)(call.pals.size() / 768) > pals_cap)
        return fail(OG_EINVAL, "pals_cap is below the " + std::to_string(call.pals.size() / 768) + " palettes of these files");
    unsigned long long zneed = 0;
    for (const PngParsed& p : call.files) zneed += p.info.status ? 0 : (unsigned long long)p.info.zlib_bytes;
    if (zneed > (unsigned long long)zcap) return fail(OG_EINVAL, "zcap is below the " + std::to_string(zneed) + " bytes of these files' zlib streams");
    size_t at = 0;
    zoffsets[0] = 0;
    for (int i = 0; i < B; ++i) {
        const PngParsed& p = call.files[i];
        if (!p.info.status)
            for (const auto& c : p.idat) {
                memcpy(zblob + at, blob + offsets[i] + c.first, c.second);
                at += c.second;
            }
        zoffsets[i + 1] = (int64_t)at;
    }
    if (!call.pals.empty()) memcpy(pals, call.pals.data(), call.pals.size());
    if (B) memcpy(recs, call.recs.data(), (size_t)B * sizeof(og_png_rec));
    *npals = (int)(call.pals.size() / 768);
    totals[0] = call.out_total;
    totals[1] = call.raw_total;
    totals[2] = call.max_pixels;
    if (!call.first_refusal.empty()) g_err = call.first_refusal;
    return OG_OK;
}

#ifndef OG_PNG_HOST_ONLY
og_png* og_png_create(void) { return new og_png(); }

void og_png_destroy(og_png* h) {
    og_stream_destroy(h, [h] { png_free(h); });
}

int og_png_sync(og_png* h) { return og_stream_sync(h); }

int og_png_set_chunk(og_png* h, int chunk) { return og_stream_set_chunk(h, chunk, kPngMaxChunk); }

int og_png_set_palettes(og_png* h, const uint8_t* pals, int npals) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (npals < 0 || npals > kPngMaxPalettes) return fail(OG_EINVAL, "npals must be 0.." + std::to_string(kPngMaxPalettes));
    if (npals > 0 && !pals) return fail(OG_EINVAL, "null palettes");
    int rc = og_stream_ready(h);
    if (rc) return rc;
    OG_SCOPE(h);
    return png_upload_pals(h, pals, npals);
}

int og_png_decode_u8_dev(og_png* h, const uint8_t* zblob_dev, const int64_t* zoffsets_dev, const og_png_rec* recs_dev, int B, int channels,
                         long long raw_bytes, int max_pixels, uint8_t* out_dev, size_t cap, int32_t* status_dev) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (B < 0 || B > 65535) return fail(OG_EINVAL, "B must be 0..65535 (one micro-batch)");
    int rc = check_png_channels(channels);
    if (rc) return rc;
    if (raw_bytes < 0 || raw_bytes > (1ll << 40)) return fail(OG_EINVAL, "raw_bytes must be 0..2^40");
    if (max_pixels < 1 || max_pixels > kMjpegMaxPixels) return fail(OG_EINVAL, "max_pixels must be 1.." + std::to_string(kMjpegMaxPixels));
    if (cap > (size_t)1 << 40) return fail(OG_EINVAL, "cap is above 2^40 bytes");
    OG_ALIGN(zoffsets_dev);
    OG_ALIGN(recs_dev);
    OG_ALIGN(status_dev);
    if (B == 0) return OG_OK;
    if (!zblob_dev || !zoffsets_dev || !recs_dev || !out_dev || !status_dev) return fail(OG_EINVAL, "null buffer");
    if (h->npals < 0) return fail(OG_ESTATE, "og_png_set_palettes has not been called");
    if ((rc = og_stream_ready(h))) return rc;
    OG_SCOPE(h);
    if ((rc = h->d_ws.grow(h, (size_t)png_ws_bytes(raw_bytes, B), "png"))) return rc;
    rc = png_batch(h->stream, h->d_ws, h->d_pals, h->npals, zblob_dev, (const long long*)zoffsets_dev, recs_dev, B, channels, raw_bytes, max_pixels,
                   out_dev, (long long)cap, (long long)cap, status_dev);
    if (rc) og_stream_drain(h);
    return rc;
}

int og_png_decode_stream(og_png* h, const uint8_t* blob, const int64_t* offsets, int B, int channels, uint8_t* out_host_or_null,
                         uint8_t* out_dev_or_null, size_t cap, int64_t* out_offsets, int32_t* hw, int32_t* status) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (B < 0) return fail(OG_EINVAL, "bad B");
    int rc = check_png_channels(channels);
    if (rc) return rc;
    OG_ALIGN(offsets);
    OG_ALIGN(out_offsets);
    OG_ALIGN(hw);
    OG_ALIGN(status);
    if (!out_offsets) return fail(OG_EINVAL, "out_offsets is null");
    if (B == 0) {
        out_offsets[0] = 0;
        return OG_OK;
    }
    if (!blob || !offsets || !status || !hw) return fail(OG_EINVAL, "null buffer");
    PngCall call;
    if ((rc = png_records(blob, offsets, B, channels, &call))) return rc;
    if ((unsigned long long)cap < (unsigned long long)call.out_total)
        return fail(OG_EINVAL, "cap is below the sum of H * W * channels = " + std::to_string(call.out_total) + " bytes");
    if (call.out_total > 0 && !out_host_or_null && !out_dev_or_null) return fail(OG_EINVAL, "no place for the pixels");
    for (int i = 0; i < B; ++i) {
        out_offsets[i] = call.recs[i].out_offset;
        hw[2 * i] = call.recs[i].H;
        hw[2 * i + 1] = call.recs[i].W;
    }
    out_offsets[B] = call.out_total;
    if (call.out_total == 0) {   // every file refused: nothing to run
        for (int i = 0; i < B; ++i) status[i] = call.recs[i].status;
        g_err = call.first_refusal;
        return OG_OK;
    }
    if ((rc = og_stream_ready(h))) return rc;
    OG_SCOPE(h);
    if ((rc = png_upload_pals(h, call.pals.data(), (int)(call.pals.size() / 768)))) return rc;
    // the micro-batches: [cuts[k], cuts[k + 1])
    std::vector<long long> raw_sizes((size_t)B), zsizes((size_t)B);
    for (int i = 0; i < B; ++i) {
        raw_sizes[i] = call.recs[i].status ? 0 : call.files[i].info.raw_bytes;
        zsizes[i] = call.recs[i].status ? 0 : call.files[i].info.zlib_bytes;
    }
    std::vector<int> cuts{0};
    while (cuts.back() < B) cuts.push_back(png_batch_end(raw_sizes.data(), cuts.back(), B, h->chunk));
    size_t in_max = 0, out_max = 0, ws_max = 0;
    int nb_max = 0;
    for (size_t k = 0; k + 1 < cuts.size(); ++k) {
        const int b0 = cuts[k], b1 = cuts[k + 1], nb = b1 - b0;
        long long zsum = 0, rsum = 0;
        for (int i = b0; i < b1; ++i) {
            zsum += zsizes[i];
            rsum += raw_sizes[i];
        }
        in_max = std::max(in_max, (size_t)(nb + 1) * 8 + (size_t)nb * sizeof(og_png_rec) + (size_t)zsum);
        out_max = std::max(out_max, (size_t)(out_offsets[b1] - out_offsets[b0]));
        ws_max = std::max(ws_max, (size_t)png_ws_bytes(rsum, nb));
        nb_max = std::max(nb_max, nb);
    }
    const bool to_host = out_host_or_null != nullptr, own_out = !out_dev_or_null;
    if ((rc = h->d_ws.grow(h, ws_max, "png"))) return rc;
    if ((rc = h->d_in.grow(h, in_max, "png"))) return rc;
    if (own_out && (rc = h->d_out.grow(h, out_max, "png"))) return rc;
    if ((rc = h->d_status.grow(h, (size_t)nb_max * 4, "png"))) return rc;
    for (auto& s : h->slots) {
        if ((rc = s.h_in.grow(h, in_max, "png"))) return rc;
        if (to_host && (rc = s.h_out.grow(h, out_max, "png"))) return rc;
        if ((rc = s.h_status.grow(h, (size_t)nb_max * 4, "png"))) return rc;
        if (!s.ev) HIPCHK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    }
    const hipStream_t st = h->stream;

    auto retire = [&](og_png::Slot& s) -> int {
        if (s.b0 < 0) return OG_OK;
        const int b0 = s.b0;
        s.b0 = -1;
        HIPCHK(hipEventSynchronize(s.ev));
        if (to_host) memcpy(out_host_or_null + out_offsets[b0], s.h_out, (size_t)(out_offsets[b0 + s.nb] - out_offsets[b0]));
        memcpy(status + b0, s.h_status, (size_t)s.nb * 4);
        return OG_OK;
    };
    auto fill = [&](og_png::Slot& s, int k, int) -> int {
        const int b0 = cuts[(size_t)k], nb = cuts[(size_t)k + 1] - b0;
        long long* zoff = (long long*)s.h_in.p;
        og_png_rec* recs = (og_png_rec*)(s.h_in + (size_t)(nb + 1) * 8);
        uint8_t* bytes = (uint8_t*)(recs + nb);
        const size_t head = (size_t)(bytes - s.h_in);
        const long long out0 = out_offsets[b0], out_bytes = out_offsets[b0 + nb] - out0, raw0 = call.recs[b0].raw_offset;
        long long at = 0, rsum = 0, maxpix = 1;
        zoff[0] = 0;
        for (int i = 0; i < nb; ++i) {
            const PngParsed& p = call.files[b0 + i];
            recs[i] = call.recs[b0 + i];
            recs[i].out_offset -= out0;
            recs[i].raw_offset -= raw0;
            if (!recs[i].status) {
                for (const auto& c : p.idat) {   // the IDAT payloads joined: the device never sees a chunk header
                    memcpy(bytes + at, blob + offsets[b0 + i] + c.first, c.second);
                    at += (long long)c.second;
                }
                rsum += raw_sizes[b0 + i];
                maxpix = std::max(maxpix, (long long)recs[i].H * recs[i].W);
            }
            zoff[i + 1] = at;
        }
        HIPCHK(hipMemcpyAsync(h->d_in, s.h_in, head + (size_t)at, hipMemcpyHostToDevice, st));
        uint8_t* dst = own_out ? h->d_out.p : out_dev_or_null + out0;
        const int rc2 = png_batch(st, h->d_ws, h->d_pals, h->npals, h->d_in + head, (const long long*)h->d_in.p,
                                  (const og_png_rec*)(h->d_in + (size_t)(nb + 1) * 8), nb, channels, rsum, maxpix, dst, out_bytes, out_bytes, h->d_status);
        if (rc2) return rc2;
        if (to_host && out_bytes) HIPCHK(hipMemcpyAsync(s.h_out, dst, (size_t)out_bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(s.h_status, h->d_status, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(s.ev, st));
        s.b0 = b0;
        s.nb = nb;
        return OG_OK;
    };

    if ((rc = og_two_slot((int)cuts.size() - 1, 1, h->slots, retire, fill, [h] { og_stream_drain(h); }))) return rc;
    if (!call.first_refusal.empty()) g_err = call.first_refusal;
    return OG_OK;
}

int og_png_plan(const int32_t* forms, int B, int channels, int chunk, char* out, size_t cap, long long* workspace_bytes) {
    if (!out || cap == 0 || B < 1 || !forms) return fail(OG_EINVAL, "bad argument");
    OG_ALIGN(forms);
    int rc = check_png_channels(channels);
    if (rc) return rc;
    if ((rc = og_check_chunk(chunk, kPngMaxChunk))) return rc;
    std::vector<long long> raw_sizes((size_t)B), out_offsets((size_t)B + 1, 0);
    for (int i = 0; i < B; ++i) {
        const int H = forms[4 * i], W = forms[4 * i + 1], ctype = forms[4 * i + 2], depth = forms[4 * i + 3];
        if (H <= 0 || W <= 0 || (long long)H * W > kMjpegMaxPixels) return fail(OG_EINVAL, "bad H/W in form " + std::to_string(i));
        if (!og_png_form_ok(ctype, depth)) return fail(OG_EINVAL, "colour type and depth of form " + std::to_string(i) + " are not decoded");
        raw_sizes[i] = (long long)H * (1 + og_png_rb(W, ctype, depth));
        out_offsets[i + 1] = out_offsets[i] + (long long)H * W * channels;
    }
    const uintptr_t gap = (uintptr_t)1 << 40;   // placeholder bases: nothing dereferences them in a dry run
    uint8_t* pixels = (uint8_t*)(1 * gap);
    int32_t* status = (int32_t*)(2 * gap);
    Plan plan;
    plan.bases = {{"out", pixels}, {"status", status}};
    g_plan = &plan;
    long long ws_max = 0, side_max = 0;
    for (int b0 = 0; b0 < B && !rc;) {
        const int b1 = png_batch_end(raw_sizes.data(), b0, B, chunk), nb = b1 - b0;
        long long rsum = 0, maxpix = 1;
        for (int i = b0; i < b1; ++i) {
            rsum += raw_sizes[i];
            maxpix = std::max(maxpix, (long long)forms[4 * i] * forms[4 * i + 1]);
        }
        const long long out_bytes = out_offsets[b1] - out_offsets[b0];
        ws_max = std::max(ws_max, png_ws_bytes(rsum, nb));
        side_max = std::max(side_max, out_bytes + (long long)nb * (4 + 8 + (long long)sizeof(og_png_rec)) + 8);
        rc = png_batch(nullptr, (uint8_t*)(3 * gap), (const uint8_t*)(4 * gap), 1, (const uint8_t*)(5 * gap), (const long long*)(6 * gap),
                       (const og_png_rec*)(7 * gap), nb, channels, rsum, maxpix, pixels + out_offsets[b0], out_bytes, out_bytes, status + b0);
        b0 = b1;
    }
    g_plan = nullptr;
    if (rc) return rc;
    if (workspace_bytes) *workspace_bytes = ws_max + side_max + 768;
    return og_plan_text(plan, kPlanWrites, out, cap);
}
#endif   // OG_PNG_HOST_ONLY

}  // extern "C"
