// PNG files encoded on the device (include_enc/openglottal_hip_pnge.h): filter, run-length tokens, one dynamic Huffman block per
// segment, the files placed densely with their CRCs.  Included by og_api.hip after og_png.inc, whose inline functions it calls; the
// kernels live here too.  A handle of its own on the streaming base of og_stream.inc: one stream, the workspace of ONE micro-batch, two
// pinned host slots.  Per micro-batch: k_pnge_filter (a wave per row), k_pnge_segment (a workgroup per segment), k_pnge_offsets (one
// workgroup), k_pnge_place (a workgroup per segment).  The host twin and the kernels call the same inline functions and agree byte for byte.
// With OG_PNG_HOST_ONLY defined (after og_png.inc, in the same translation unit) only the twin is compiled, no HIP
// (tools/pnge_host_check.cpp builds it under sanitizers).
#include "../../include_enc/openglottal_hip_pnge.h"

constexpr int kPngeMinSeg = 64, kPngeMaxSeg = 32768, kPngeMaxChunk = 1024;
constexpr int kPngeFixed = 57;      // signature 8, IHDR 25, IDAT 12, IEND 12
constexpr int kPngeBefore = 43;     // signature, IHDR, IDAT length and type, the zlib header
constexpr int kPngeSlotPad = 16;    // a segment's slot is S + 16 bytes
constexpr int kPngeThreads = 1024;
constexpr uint32_t kPngeCrcPoly = 0xEDB88320u;

// the histogram, the scratch of the code construction and the code of one segment: in LDS in the kernel, on the stack in the twin
struct OgPngeCode {
    uint32_t hist[288];
    uint32_t weight[572];   // the tree's node weights; afterwards [1..15]: the first canonical code of each length
    uint16_t parent[572];   // a node's parent, then its depth
    uint16_t sorted[288];   // the used symbols by (count, symbol) ascending
    uint16_t code[288];     // bit-reversed: ready for an LSB-first bit string
    uint16_t blc[16];       // codes per length
    uint8_t len[288];
    // the block header: the code-length code over 0..18 and the run-length coded sequence of the hlit + 1 lengths
    uint32_t clhist[19];
    uint16_t clcode[19];
    uint8_t cllen[19];
    uint8_t clsym[288], clext[288];
    int nused, hlit, ncl, hclen, hdr_bits;
};

// ---- the arithmetic: host twin and kernels ---------------------------------------------------------------------------------------
// byte x of an unfiltered scanline: C = 3 frames are stored B G R and written R G B
OG_PNG_HD int og_pnge_src(const uint8_t* row, long long x, int C) {
    if (C == 1) return row[x];
    const long long p = x / 3;
    return row[3 * p + 2 - (x - 3 * p)];
}
// v and its neighbours a (left), b (up), c (up-left); up: the row above, or null for row 0
OG_PNG_HD void og_pnge_taps(const uint8_t* cur, const uint8_t* up, long long x, int C, int* v, int* a, int* b, int* c) {
    *v = og_pnge_src(cur, x, C);
    *a = x >= C ? og_pnge_src(cur, x - C, C) : 0;
    *b = up ? og_pnge_src(up, x, C) : 0;
    *c = (up && x >= C) ? og_pnge_src(up, x - C, C) : 0;
}
OG_PNG_HD int og_pnge_filt(int ft, int v, int a, int b, int c) { return (v - og_png_recon(ft, 0, a, b, c)) & 255; }
OG_PNG_HD int og_pnge_cost(int fb) { return fb < 128 ? fb : 256 - fb; }
// the type with the least cost, ties to the lower type
OG_PNG_HD int og_pnge_best(const unsigned long long* cost) {
    int best = 0;
    for (int ft = 1; ft < 5; ++ft)
        if (cost[ft] < cost[best]) best = ft;
    return best;
}

// length 3..258 -> its code 0..28 (lit/len symbol 257 + code), the count and value of its extra bits
OG_PNG_HD int og_pnge_len_sym(int L, int* ebits, int* eval) {
    *ebits = 0;
    *eval = 0;
    if (L == 258) return 28;
    const int m = L - 3;
    if (m < 8) return m;
    const int e = 29 - __builtin_clz((unsigned)m);   // floor(log2 m) - 2: 1..5
    *ebits = e;
    *eval = m & ((1 << e) - 1);
    return 4 * e + (m >> e);
}

// the tokens of one run: byte v once and then R more times.  f(symbol, extra bits, extra value); a symbol above 256 is a match at distance 1
template <class F>
OG_PNG_HD void og_pnge_run(int v, int R, F&& f) {
    f(v, 0, 0);
    for (int q = R / 258; q > 0; --q) f(285, 0, 0);
    int r = R % 258;
    if (r >= 3) {
        int eb, ev;
        const int ls = og_pnge_len_sym(r, &eb, &ev);
        f(257 + ls, eb, ev);
    } else {
        for (; r > 0; --r) f(v, 0, 0);
    }
}

// the place of symbol s among the used ones in (count, symbol) ascending order; -1: unused
OG_PNG_HD int og_pnge_rank(const uint32_t* hist, int nsym, int s) {
    const uint32_t f = hist[s];
    if (!f) return -1;
    int r = 0;
    for (int t = 0; t < nsym; ++t) {
        const uint32_t g = hist[t];
        r += (g != 0 && (g < f || (g == f && t < s))) ? 1 : 0;
    }
    return r;
}

OG_PNG_HD uint32_t og_pnge_rev(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// hist over nsym symbols, c->sorted and c->nused (>= 2) -> len and code, no length above maxlen.  Serial: one thread of the
// workgroup, or the twin.  See CODE in the header.
OG_PNG_HD void og_pnge_build(OgPngeCode* c, const uint32_t* hist, int nsym, int maxlen, uint8_t* len, uint16_t* codes) {
    const int n = c->nused;
    for (int i = 0; i < n; ++i) c->weight[i] = hist[c->sorted[i]];
    int li = 0, ii = n, nf = n;
    for (int m = 0; m + 1 < n; ++m) {
        const int a = (li < n && (ii >= nf || c->weight[li] <= c->weight[ii])) ? li++ : ii++;
        const int b = (li < n && (ii >= nf || c->weight[li] <= c->weight[ii])) ? li++ : ii++;
        c->weight[nf] = c->weight[a] + c->weight[b];
        c->parent[a] = c->parent[b] = (uint16_t)nf;
        ++nf;
    }
    c->parent[2 * n - 2] = 0;   // the root; a parent lies above its children, so depths can replace parents from the top
    for (int k = 2 * n - 3; k >= 0; --k) c->parent[k] = (uint16_t)(c->parent[c->parent[k]] + 1);
    for (int l = 0; l < 16; ++l) c->blc[l] = 0;
    for (int k = 0; k < n; ++k) {
        const int d = c->parent[k] < maxlen ? c->parent[k] : maxlen;
        c->blc[d] = (uint16_t)(c->blc[d] + 1);
    }
    uint32_t total = 0;
    for (int l = 1; l <= maxlen; ++l) total += (uint32_t)c->blc[l] << (maxlen - l);
    for (int turn = 0; turn < 288 && total > (1u << maxlen); ++turn) {   // the limiter
        c->blc[maxlen] = (uint16_t)(c->blc[maxlen] - 1);
        for (int l = maxlen - 1; l > 0; --l)
            if (c->blc[l]) {
                c->blc[l] = (uint16_t)(c->blc[l] - 1);
                c->blc[l + 1] = (uint16_t)(c->blc[l + 1] + 2);
                break;
            }
        --total;
    }
    for (int s = 0; s < nsym; ++s) len[s] = 0;
    int idx = 0;
    for (int l = maxlen; l >= 1; --l)
        for (int k = 0; k < c->blc[l]; ++k) len[c->sorted[idx++]] = (uint8_t)l;
    uint32_t code = 0;
    c->blc[0] = 0;
    for (int l = 1; l <= maxlen; ++l) {
        code = (code + c->blc[l - 1]) << 1;
        c->weight[l] = code;
    }
    for (int s = 0; s < nsym; ++s) {
        const int l = len[s];
        codes[s] = 0;
        if (!l) continue;
        codes[s] = (uint16_t)og_pnge_rev(c->weight[l], l);
        c->weight[l] += 1;
    }
}

// one symbol of the code-length sequence
OG_PNG_HD void og_pnge_cl_emit(OgPngeCode* c, int sym, int ext) {
    c->clsym[c->ncl] = (uint8_t)sym;
    c->clext[c->ncl] = (uint8_t)ext;
    c->ncl += 1;
    c->clhist[sym] += 1;
}
OG_PNG_HD int og_pnge_cl_extra(int sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }
// RFC 1951's order of the code-length code's own lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
OG_PNG_HD int og_pnge_cl_order(int i) {
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 |
                        11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (int)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31);
}

// The lit/len code from c->hist, c->sorted, c->nused, and the whole block header after it: hlit, the hlit lit/len lengths and the one
// distance length (1) as a run-length coded sequence, the code-length code (at most 7 bits) over its symbols, hclen, hdr_bits.
// Serial.  See BLOCK HEADER in the header.
OG_PNG_HD void og_pnge_code(OgPngeCode* c) {
    og_pnge_build(c, c->hist, 286, 15, c->len, c->code);
    c->hlit = 257;
    for (int s = 257; s < 286; ++s)
        if (c->len[s]) c->hlit = s + 1;
    for (int s = 0; s < 19; ++s) c->clhist[s] = 0;
    c->ncl = 0;
    const int total = c->hlit + 1;
    for (int i = 0; i < total;) {
        const int v = i < c->hlit ? c->len[i] : 1;
        int r = 1;
        while (i + r < total && (i + r < c->hlit ? c->len[i + r] : 1) == v) ++r;
        i += r;
        if (v == 0) {
            for (; r >= 11; r -= (r < 138 ? r : 138)) og_pnge_cl_emit(c, 18, (r < 138 ? r : 138) - 11);
            if (r >= 3) {
                og_pnge_cl_emit(c, 17, r - 3);
                r = 0;
            }
        } else {
            og_pnge_cl_emit(c, v, 0);
            for (--r; r >= 3; r -= (r < 6 ? r : 6)) og_pnge_cl_emit(c, 16, (r < 6 ? r : 6) - 3);
        }
        for (; r > 0; --r) og_pnge_cl_emit(c, v, 0);
    }
    c->nused = 0;
    for (int s = 0; s < 19; ++s) c->nused += c->clhist[s] ? 1 : 0;
    if (c->nused < 2) c->clhist[c->clhist[0] ? 1 : 0] = 1;   // a complete code needs two symbols
    c->nused = 0;
    for (int s = 0; s < 19; ++s) {
        const int r = og_pnge_rank(c->clhist, 19, s);
        if (r >= 0) {
            c->sorted[r] = (uint16_t)s;
            c->nused += 1;
        }
    }
    og_pnge_build(c, c->clhist, 19, 7, c->cllen, c->clcode);
    c->hclen = 4;
    for (int i = 4; i < 19; ++i)
        if (c->cllen[og_pnge_cl_order(i)]) c->hclen = i + 1;
    int bits = 17 + 3 * c->hclen;
    for (int i = 0; i < c->ncl; ++i) bits += c->cllen[c->clsym[i]] + og_pnge_cl_extra(c->clsym[i]);
    c->hdr_bits = bits;
}

// k <= 32 bits of v (the bits above k are 0) into an LSB-first bit string of zeroed 32-bit words
OG_PNG_HD void og_pnge_put(uint32_t* words, long long bit, uint32_t v, int k) {
    (void)k;
    const uint64_t x = (uint64_t)v << (bit & 31);
    uint32_t* w = words + (bit >> 5);
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
#if defined(__HIP_DEVICE_COMPILE__)
    if (lo) atomicOr(w, lo);
    if (hi) atomicOr(w + 1, hi);
#else
    if (lo) w[0] |= lo;
    if (hi) w[1] |= hi;
#endif
}

// the block's header, c->hdr_bits bits from bit 0.  Serial.
OG_PNG_HD void og_pnge_hdr_put(uint32_t* words, const OgPngeCode* c, bool final) {
    og_pnge_put(words, 0, (final ? 1u : 0u) | 2u << 1, 3);
    og_pnge_put(words, 3, (uint32_t)(c->hlit - 257), 5);
    og_pnge_put(words, 8, 0, 5);
    og_pnge_put(words, 13, (uint32_t)(c->hclen - 4), 4);
    long long pos = 17;
    for (int i = 0; i < c->hclen; ++i, pos += 3) og_pnge_put(words, pos, c->cllen[og_pnge_cl_order(i)], 3);
    for (int i = 0; i < c->ncl; ++i) {
        const int sym = c->clsym[i], l = c->cllen[sym], e = og_pnge_cl_extra(sym);
        og_pnge_put(words, pos, (uint32_t)c->clcode[sym] | (uint32_t)c->clext[i] << l, l + e);
        pos += l + e;
    }
}
OG_PNG_HD int og_pnge_tok_bits(const OgPngeCode* c, int sym, int eb) { return c->len[sym] + eb + (sym > 256 ? 1 : 0); }
OG_PNG_HD void og_pnge_tok_put(uint32_t* words, long long bit, const OgPngeCode* c, int sym, int eb, int ev) {
    og_pnge_put(words, bit, (uint32_t)c->code[sym] | (uint32_t)ev << c->len[sym], og_pnge_tok_bits(c, sym, eb));   // (the distance code is one 0 bit)
}
// bytes of a dynamic block of total_bits bits with what closes it
OG_PNG_HD long long og_pnge_dyn_bytes(long long total_bits, bool final) {
    if (final || (total_bits & 7) == 0) return (total_bits + 7) >> 3;
    return ((total_bits + 3 + 7) >> 3) + 4;
}
// the end-of-block code and, for a non-final block off the byte grid, the empty stored block
OG_PNG_HD void og_pnge_close(uint32_t* words, const OgPngeCode* c, long long tok_end, bool final) {
    og_pnge_put(words, tok_end, c->code[256], c->len[256]);
    const long long total_bits = tok_end + c->len[256];
    if (!final && (total_bits & 7)) og_pnge_put(words, ((total_bits + 3 + 7) >> 3) * 8, 0xFFFF0000u, 32);
}
// the five bytes before a stored block's data (the block starts on a byte)
OG_PNG_HD void og_pnge_stored_head(uint8_t* out, int n, bool final) {
    out[0] = final ? 1 : 0;
    out[1] = (uint8_t)(n & 255);
    out[2] = (uint8_t)(n >> 8);
    out[3] = (uint8_t)(~n & 255);
    out[4] = (uint8_t)((~n >> 8) & 255);
}

// CRC-32 of PNG and zlib: crc of p[0, n) continued from crc (0 at the start)
OG_PNG_HD uint32_t og_pnge_crc(uint32_t crc, const uint8_t* p, long long n) {
    uint32_t c = ~crc;
    for (long long i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (kPngeCrcPoly & (0u - (c & 1u)));
    }
    return ~c;
}
// a * b modulo the CRC polynomial, bit 31 the coefficient of x^0
OG_PNG_HD uint32_t og_pnge_gfmul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ (kPngeCrcPoly & (0u - (b & 1u)));
    }
    return p;
}
// the CRC of A as it counts in the CRC of A B, |B| = nbytes: crc(A B) = og_pnge_crc_shift(crc(A), |B|) ^ crc(B)
OG_PNG_HD uint32_t og_pnge_crc_shift(uint32_t crc, long long nbytes) {
    uint32_t r = 0x80000000u, base = 0x00800000u;   // 1 and x^8
    for (long long n = nbytes; n > 0; n >>= 1) {
        if (n & 1) r = og_pnge_gfmul(r, base);
        base = og_pnge_gfmul(base, base);
    }
    return og_pnge_gfmul(r, crc);
}
OG_PNG_HD void og_pnge_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}
// the 43 bytes before the first segment: signature, IHDR with its CRC, IDAT's length and type, the zlib header
OG_PNG_HD void og_pnge_file_head(uint8_t* p, int H, int W, int C, uint32_t idat_len) {
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    for (int i = 0; i < 8; ++i) p[i] = sig[i];
    og_pnge_be32(p + 8, 13);
    p[12] = 'I'; p[13] = 'H'; p[14] = 'D'; p[15] = 'R';
    og_pnge_be32(p + 16, (uint32_t)W);
    og_pnge_be32(p + 20, (uint32_t)H);
    p[24] = 8;
    p[25] = C == 3 ? 2 : 0;
    p[26] = p[27] = p[28] = 0;
    og_pnge_be32(p + 29, og_pnge_crc(0, p + 12, 17));
    og_pnge_be32(p + 33, idat_len);
    p[37] = 'I'; p[38] = 'D'; p[39] = 'A'; p[40] = 'T';
    p[41] = 0x78;
    p[42] = 0x01;
}
// the CRC of "IDAT" and the zlib header: where the join over the segments starts
OG_PNG_HD uint32_t og_pnge_idat_crc0() {
    const uint8_t b[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
    return og_pnge_crc(0, b, 6);
}
// the 20 bytes behind the last segment: Adler-32, IDAT's CRC (crc: of everything up to the Adler-32), IEND
OG_PNG_HD void og_pnge_file_tail(uint8_t* p, uint32_t adler, uint32_t crc) {
    og_pnge_be32(p, adler);
    og_pnge_be32(p + 4, og_pnge_crc(crc, p, 4));
    og_pnge_be32(p + 8, 0);
    p[12] = 'I'; p[13] = 'E'; p[14] = 'N'; p[15] = 'D';
    og_pnge_be32(p + 16, og_pnge_crc(0, p + 12, 4));
}

// the tight box of label > 0 from the extremes of x and y (x1 < 0: no pixel): x0 y0 x1 + 1 y1 + 1, or 0 0 0 0
OG_PNG_HD void og_pnge_bbox(int x0, int y0, int x1, int y1, int32_t* box4) {
    const bool any = x1 >= 0;
    box4[0] = any ? x0 : 0;
    box4[1] = any ? y0 : 0;
    box4[2] = any ? x1 + 1 : 0;
    box4[3] = any ? y1 + 1 : 0;
}

#ifndef OG_PNG_HOST_ONLY
// ---- kernels ---------------------------------------------------------------------------------------------------------------------
// A workgroup per label [H,W] u8: the extremes of x and y over label > 0, a lane per pixel in strides, then a tree in LDS; boxes
// [B][4] int32 written by thread 0 with plain stores.
__global__ __launch_bounds__(256) void k_label_bbox(const uint8_t* __restrict__ labels, int H, int W, int32_t* __restrict__ boxes) {
    __shared__ int s_v[4][256];
    const int t = threadIdx.x;
    const uint8_t* p = labels + (long long)blockIdx.x * H * W;
    int x0 = W, y0 = H, x1 = -1, y1 = -1;
    for (int i = t; i < H * W; i += 256)
        if (p[i] > 0) {
            const int y = i / W, x = i - y * W;
            x0 = min(x0, x);
            y0 = min(y0, y);
            x1 = max(x1, x);
            y1 = max(y1, y);
        }
    s_v[0][t] = x0;
    s_v[1][t] = y0;
    s_v[2][t] = x1;
    s_v[3][t] = y1;
    __syncthreads();
#pragma unroll
    for (int d = 128; d > 0; d >>= 1) {
        if (t < d) {
            s_v[0][t] = min(s_v[0][t], s_v[0][t + d]);
            s_v[1][t] = min(s_v[1][t], s_v[1][t + d]);
            s_v[2][t] = max(s_v[2][t], s_v[2][t + d]);
            s_v[3][t] = max(s_v[3][t], s_v[3][t + d]);
        }
        __syncthreads();
    }
    if (t == 0) og_pnge_bbox(s_v[0][0], s_v[1][0], s_v[2][0], s_v[3][0], boxes + 4 * (long long)blockIdx.x);
}

// A wave per row: grid ceil(rows / 4), rows = nb * H.  raw: nb streams of raw_pitch bytes; parts [rows][2]: the row's share of the
// Adler-32 sums of its file (og_png_adler_part's s1 and s2, weights counted from the end of the file's stream).
__global__ __launch_bounds__(256) void k_pnge_filter(const uint8_t* __restrict__ frames, long long rows, int H, int W, int C, long long raw_pitch,
                                                     uint8_t* raw, uint32_t* __restrict__ parts) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long long f = row / H, rb = (long long)W * C, L = 1 + rb;
    const int r = (int)(row - f * H);
    const uint8_t* cur = frames + row * rb;
    const uint8_t* up = r ? cur - rb : nullptr;
    unsigned long long cost[5] = {0, 0, 0, 0, 0};
    for (long long x = lane; x < rb; x += 64) {
        int v, a, b, c;
        og_pnge_taps(cur, up, x, C, &v, &a, &b, &c);
#pragma unroll
        for (int ft = 0; ft < 5; ++ft) cost[ft] += (unsigned)og_pnge_cost(og_pnge_filt(ft, v, a, b, c));
    }
#pragma unroll
    for (int ft = 0; ft < 5; ++ft)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cost[ft] += __shfl_xor(cost[ft], o);
    const int best = og_pnge_best(cost);
    uint8_t* dst = raw + f * raw_pitch + r * L;
    for (long long i = lane; i < L; i += 64) {   // lane i mod 64 writes byte i and, below, reads it back
        int fb = best;
        if (i > 0) {
            int v, a, b, c;
            og_pnge_taps(cur, up, i - 1, C, &v, &a, &b, &c);
            fb = og_pnge_filt(best, v, a, b, c);
        }
        dst[i] = (uint8_t)fb;
    }
    uint32_t s1, s2;
    og_png_adler_part<64>(dst, L, lane, &s1, &s2);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    if (lane == 0) {
        const long long after = (long long)(H - 1 - r) * L;   // the stream's bytes behind this row: every weight grows by that
        s1 %= kAdlerMod;
        parts[2 * row] = s1;
        parts[2 * row + 1] = (uint32_t)((s2 % kAdlerMod + (unsigned long long)(after % kAdlerMod) * s1) % kAdlerMod);
    }
}

// the runs that start in [first, hi) of a segment in LDS; the last of them may end behind hi, at nxt
template <class F>
__device__ __forceinline__ void pnge_walk(const uint8_t* seg, int first, int hi, int nxt, F&& f) {
    for (int j = first; j < hi;) {
        const int v = seg[j];
        int e = j + 1;
        while (e < hi && seg[e] == v) ++e;
        if (e == hi) e = nxt;
        og_pnge_run(v, e - j - 1, f);
        j = e;
    }
}

// A workgroup per (segment, file): grid (nseg, nb).  slots: S + 16 bytes per segment; lens, crcs [nb * nseg].
__global__ __launch_bounds__(kPngeThreads) void k_pnge_segment(const uint8_t* __restrict__ raw, long long raw_pitch, long long N, int S, int nseg,
                                                               uint8_t* __restrict__ slots, int* __restrict__ lens, uint32_t* __restrict__ crcs) {
    __shared__ uint32_t s_seg[kPngeMaxSeg / 4];
    __shared__ uint32_t s_out[(kPngeMaxSeg + kPngeSlotPad) / 4];
    __shared__ OgPngeCode s_c;
    __shared__ uint32_t s_scan[kPngeThreads];
    __shared__ uint32_t s_crc;
    const int k = blockIdx.x, t = threadIdx.x;
    const long long i = (long long)blockIdx.y * nseg + k, o = (long long)k * S;
    const int n = (int)(N - o < S ? N - o : S);
    const bool final = k == nseg - 1;
    const uint32_t* src = (const uint32_t*)(raw + blockIdx.y * raw_pitch + o);   // (raw_pitch and S are multiples of 16)
    for (int j = t; j < (n + 3) >> 2; j += kPngeThreads) s_seg[j] = src[j];
    for (int j = t; j < (n + kPngeSlotPad) >> 2; j += kPngeThreads) s_out[j] = 0;
    for (int j = t; j < 288; j += kPngeThreads) s_c.hist[j] = j == 256 ? 1 : 0;
    if (t == 0) {
        s_c.nused = 0;
        s_crc = 0;
    }
    __syncthreads();
    const uint8_t* seg = (const uint8_t*)s_seg;
    const int per = (n + kPngeThreads - 1) / kPngeThreads, lo = min(t * per, n), hi = min(lo + per, n);
    int first = n;   // the first run start in this thread's stretch
    for (int j = hi - 1; j >= lo; --j)
        if (j == 0 || seg[j] != seg[j - 1]) first = j;
    s_scan[t] = (uint32_t)first;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < kPngeThreads; d <<= 1) {   // suffix minimum
        const uint32_t a = t + d < kPngeThreads ? s_scan[t + d] : (uint32_t)n;
        __syncthreads();
        s_scan[t] = min(s_scan[t], a);
        __syncthreads();
    }
    const int nxt = t + 1 < kPngeThreads ? (int)s_scan[t + 1] : n;   // the first run start behind this stretch
    pnge_walk(seg, first, hi, nxt, [&](int sym, int, int) { atomicAdd(&s_c.hist[sym], 1u); });
    __syncthreads();
    if (t < 286) {
        const int r = og_pnge_rank(s_c.hist, 286, t);
        if (r >= 0) {
            s_c.sorted[r] = (uint16_t)t;
            atomicAdd(&s_c.nused, 1);
        }
    }
    __syncthreads();
    if (t == 0) og_pnge_code(&s_c);
    __syncthreads();
    uint32_t bits = 0;
    pnge_walk(seg, first, hi, nxt, [&](int sym, int eb, int) { bits += (uint32_t)og_pnge_tok_bits(&s_c, sym, eb); });
    s_scan[t] = bits;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < kPngeThreads; d <<= 1) {   // prefix sum
        const uint32_t a = t >= d ? s_scan[t - d] : 0;
        __syncthreads();
        s_scan[t] += a;
        __syncthreads();
    }
    const long long hdr = s_c.hdr_bits, tok_end = hdr + s_scan[kPngeThreads - 1];
    const long long dyn = og_pnge_dyn_bytes(tok_end + s_c.len[256], final);
    int len;
    if (dyn < 5 + n) {
        if (t == 0) og_pnge_hdr_put(s_out, &s_c, final);
        long long pos = hdr + s_scan[t] - bits;
        pnge_walk(seg, first, hi, nxt, [&](int sym, int eb, int ev) {
            og_pnge_tok_put(s_out, pos, &s_c, sym, eb, ev);
            pos += og_pnge_tok_bits(&s_c, sym, eb);
        });
        if (t == 0) og_pnge_close(s_out, &s_c, tok_end, final);
        len = (int)dyn;
    } else {
        uint8_t* out8 = (uint8_t*)s_out;
        if (t == 0) og_pnge_stored_head(out8, n, final);
        for (int j = t; j < n; j += kPngeThreads) out8[5 + j] = seg[j];
        len = 5 + n;
    }
    __syncthreads();
    const int cper = (len + kPngeThreads - 1) / kPngeThreads, clo = min(t * cper, len), chi = min(clo + cper, len);
    if (chi > clo) atomicXor(&s_crc, og_pnge_crc_shift(og_pnge_crc(0, (const uint8_t*)s_out + clo, chi - clo), len - chi));
    uint32_t* dst = (uint32_t*)(slots + i * (S + kPngeSlotPad));
    for (int j = t; j < (len + 3) >> 2; j += kPngeThreads) dst[j] = s_out[j];
    __syncthreads();
    if (t == 0) {
        lens[i] = len;
        crcs[i] = s_crc;
    }
}

// One workgroup, a thread per file (nb <= 1024).  seg_off [nb * nseg]: a segment's place behind the zlib header; file_off [nb]: the
// file's place in the caller's buffer; file_crc: IDAT's CRC up to the Adler-32; file_adler.
__global__ __launch_bounds__(kPngeThreads) void k_pnge_offsets(const int* __restrict__ lens, const uint32_t* __restrict__ crcs,
                                                               const uint32_t* __restrict__ parts, int nseg, int nb, int H, long long N, int first,
                                                               long long* total, int32_t* __restrict__ sizes, long long* __restrict__ file_off,
                                                               int* __restrict__ seg_off, uint32_t* __restrict__ file_crc,
                                                               uint32_t* __restrict__ file_adler) {
    __shared__ long long ssum[kPngeThreads];
    const int t = threadIdx.x;
    long long size = 0;
    if (t < nb) {
        long long z = 0;
        uint32_t crc = og_pnge_idat_crc0();
        for (int k = 0; k < nseg; ++k) {
            const long long i = (long long)t * nseg + k;
            const int len = lens[i];
            seg_off[i] = (int)z;
            crc = og_pnge_crc_shift(crc, len) ^ crcs[i];
            z += len;
        }
        unsigned long long s1 = 0, s2 = 0;
        for (int r = 0; r < H; ++r) {
            s1 += parts[2 * ((long long)t * H + r)];
            s2 += parts[2 * ((long long)t * H + r) + 1];
        }
        file_crc[t] = crc;
        file_adler[t] = og_png_adler_join((uint32_t)(s1 % kAdlerMod), (uint32_t)(s2 % kAdlerMod), N);
        size = kPngeFixed + 2 + z + 4;
    }
    ssum[t] = size;
    const long long base = first ? 0 : *total;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < kPngeThreads; d <<= 1) {
        const long long a = t >= d ? ssum[t - d] : 0;
        __syncthreads();
        ssum[t] += a;
        __syncthreads();
    }
    if (t < nb) {
        file_off[t] = base + ssum[t] - size;
        sizes[t] = (int32_t)size;
    }
    if (t == 0) *total = base + ssum[kPngeThreads - 1];
}

// A workgroup per (segment, file): grid (nseg, nb).
__global__ __launch_bounds__(256) void k_pnge_place(const uint8_t* __restrict__ slots, const int* __restrict__ lens, const int* __restrict__ seg_off,
                                                    const long long* __restrict__ file_off, const uint32_t* __restrict__ file_crc,
                                                    const uint32_t* __restrict__ file_adler, int nseg, int S, int H, int W, int C,
                                                    uint8_t* __restrict__ out) {
    const int k = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    const long long i = (long long)f * nseg + k;
    const int len = lens[i];
    const uint8_t* src = slots + i * (S + kPngeSlotPad);
    uint8_t* file = out + file_off[f];
    uint8_t* dst = file + kPngeBefore + seg_off[i];
    for (int j = t; j < len; j += 256) dst[j] = src[j];
    if (t != 0) return;
    if (k == 0) {
        const long long last = (long long)f * nseg + nseg - 1;
        og_pnge_file_head(file, H, W, C, (uint32_t)(2 + seg_off[last] + lens[last] + 4));
    }
    if (k == nseg - 1) og_pnge_file_tail(dst + len, file_adler[f], file_crc[f]);
}
#endif   // OG_PNG_HOST_ONLY

// ---- host side -------------------------------------------------------------------------------------------------------------------
#ifndef OG_PNG_HOST_ONLY
struct og_pnge : OgStreamHandle {
    int segment = kPngeMaxSeg;
    // each buffer holds the bytes of the largest micro-batch run so far
    OgBuf<uint8_t> d_ws;     // raw streams, slots, offsets, Adler parts, lengths, CRCs
    OgBuf<uint8_t> d_in, d_out;
    OgBuf<uint8_t> d_meta;   // streamed entry: total (8 bytes), then the sizes
    struct Slot {
        OgBuf<uint8_t> h_in{true}, h_out{true}, h_meta{true};
        hipEvent_t ev = nullptr;
        int b0 = -1, nb = 0;
        long long at = 0, bytes = 0;   // where in the caller's out, how many
    } slots[2];
};
#endif

namespace {

struct PngeGeom {
    int H, W, C, S, nseg;
    long long rb, N, raw_pitch;
};
int check_pnge_shape(int H, int W, int C, int S) {
    if (C != 1 && C != 3) return fail(OG_EINVAL, "C must be 1 (gray) or 3 (B G R)");
    if (H < 1 || W < 1 || (long long)H * W > kMjpegMaxPixels) return fail(OG_EINVAL, "H and W must be positive and H * W at most " + std::to_string(kMjpegMaxPixels));
    if (S < kPngeMinSeg || S > kPngeMaxSeg || (S & (S - 1))) return fail(OG_EINVAL, "the segment must be a power of two, 64..32768 bytes");
    return OG_OK;
}
PngeGeom pnge_geom(int H, int W, int C, int S) {
    PngeGeom g;
    g.H = H;
    g.W = W;
    g.C = C;
    g.S = S;
    g.rb = (long long)W * C;
    g.N = (long long)H * (1 + g.rb);
    g.nseg = (int)((g.N + S - 1) / S);
    g.raw_pitch = (g.N + 15) & ~15ll;
    return g;
}
long long pnge_zbound(long long n, int S) { return 2 + n + 5 * ((n + S - 1) / S) + 4; }
long long pnge_bound(const PngeGeom& g) { return kPngeFixed + pnge_zbound(g.N, g.S); }

// one segment -> out (room for 5 + n bytes); returns its bytes.  words: scratch of (n + 16) / 4 words.
long long pnge_segment_host(const uint8_t* seg, int n, bool final, uint8_t* out, std::vector<uint32_t>& words) {
    OgPngeCode c;
    for (int s = 0; s < 288; ++s) c.hist[s] = s == 256 ? 1 : 0;
    auto runs = [&](auto&& f) {
        for (int j = 0; j < n;) {
            int e = j + 1;
            while (e < n && seg[e] == seg[j]) ++e;
            og_pnge_run(seg[j], e - j - 1, f);
            j = e;
        }
    };
    runs([&](int sym, int, int) { c.hist[sym] += 1; });
    c.nused = 0;
    for (int s = 0; s < 286; ++s) {
        const int r = og_pnge_rank(c.hist, 286, s);
        if (r >= 0) {
            c.sorted[r] = (uint16_t)s;
            c.nused += 1;
        }
    }
    og_pnge_code(&c);
    long long tok = 0;
    runs([&](int sym, int eb, int) { tok += og_pnge_tok_bits(&c, sym, eb); });
    const long long hdr = c.hdr_bits, tok_end = hdr + tok;
    const long long dyn = og_pnge_dyn_bytes(tok_end + c.len[256], final);
    if (dyn >= 5 + n) {
        og_pnge_stored_head(out, n, final);
        memcpy(out + 5, seg, (size_t)n);
        return 5 + n;
    }
    words.assign((size_t)((n + kPngeSlotPad) >> 2), 0u);
    og_pnge_hdr_put(words.data(), &c, final);
    long long pos = hdr;
    runs([&](int sym, int eb, int ev) {
        og_pnge_tok_put(words.data(), pos, &c, sym, eb, ev);
        pos += og_pnge_tok_bits(&c, sym, eb);
    });
    og_pnge_close(words.data(), &c, tok_end, final);
    for (long long j = 0; j < dyn; ++j) out[j] = (uint8_t)(words[(size_t)(j >> 2)] >> (8 * (j & 3)));
    return dyn;
}

// n raw bytes -> the segments back to back (no zlib header or trailer); *crc: IDAT's CRC continued over them
long long pnge_segments_host(const uint8_t* raw, long long n, int S, uint8_t* out, uint32_t* crc) {
    std::vector<uint32_t> words;
    long long at = 0;
    for (long long o = 0; o < n; o += S) {
        const int m = (int)(n - o < S ? n - o : S);
        const long long len = pnge_segment_host(raw + o, m, o + S >= n, out + at, words);
        if (crc) *crc = og_pnge_crc_shift(*crc, len) ^ og_pnge_crc(0, out + at, len);
        at += len;
    }
    return at;
}

void pnge_filter_host(const uint8_t* frame, const PngeGeom& g, uint8_t* raw) {
    for (int r = 0; r < g.H; ++r) {
        const uint8_t* cur = frame + r * g.rb;
        const uint8_t* up = r ? cur - g.rb : nullptr;
        unsigned long long cost[5] = {0, 0, 0, 0, 0};
        for (long long x = 0; x < g.rb; ++x) {
            int v, a, b, c;
            og_pnge_taps(cur, up, x, g.C, &v, &a, &b, &c);
            for (int ft = 0; ft < 5; ++ft) cost[ft] += (unsigned)og_pnge_cost(og_pnge_filt(ft, v, a, b, c));
        }
        const int best = og_pnge_best(cost);
        uint8_t* dst = raw + r * (1 + g.rb);
        dst[0] = (uint8_t)best;
        for (long long x = 0; x < g.rb; ++x) {
            int v, a, b, c;
            og_pnge_taps(cur, up, x, g.C, &v, &a, &b, &c);
            dst[1 + x] = (uint8_t)og_pnge_filt(best, v, a, b, c);
        }
    }
}

// the twin of the four launches on one frame: the file's bytes
long long pnge_file_host(const uint8_t* frame, const PngeGeom& g, uint8_t* out) {
    std::vector<uint8_t> raw((size_t)g.N);
    pnge_filter_host(frame, g, raw.data());
    uint32_t crc = og_pnge_idat_crc0();
    const long long z = pnge_segments_host(raw.data(), g.N, g.S, out + kPngeBefore, &crc);
    uint32_t s1, s2;
    og_png_adler_part<1>(raw.data(), g.N, 0, &s1, &s2);
    og_pnge_file_head(out, g.H, g.W, g.C, (uint32_t)(2 + z + 4));
    og_pnge_file_tail(out + kPngeBefore + z, og_png_adler_join(s1, s2, g.N), crc);
    return kPngeFixed + 2 + z + 4;
}

#ifndef OG_PNG_HOST_ONLY
// device workspace: per frame and of a micro-batch (every part a multiple of 16 bytes)
long long pnge_frame_ws(const PngeGeom& g) { return g.raw_pitch + (long long)g.nseg * (g.S + kPngeSlotPad + 12) + 8ll * g.H + 24; }
long long pnge_ws_bytes(const PngeGeom& g, int nb) {
    auto up = [](long long v) { return (v + 15) & ~15ll; };
    const long long n = (long long)nb * g.nseg;
    return nb * g.raw_pitch + n * (g.S + kPngeSlotPad) + up(8ll * nb) + up(8ll * nb * g.H) + 3 * up(4 * n) + 2 * up(4ll * nb);
}
int pnge_chunk(int chunk, const PngeGeom& g) {
    const long long fit = kMjpegBatchBytes / pnge_frame_ws(g);
    return (int)(fit < 1 ? 1 : (fit < chunk ? fit : chunk));
}

void pnge_free(og_pnge* h) {
    og_release(h->d_ws, h->d_in, h->d_out, h->d_meta);
    for (auto& s : h->slots) {
        og_release(s.h_in, s.h_out, s.h_meta);
        if (s.ev) (void)hipEventDestroy(s.ev);
    }
}

// One micro-batch of nb resident frames.  ws: the handle's workspace (a placeholder in a dry run).  `first`: the files start at
// out[0]; otherwise at out[*total].  sizes: of these nb frames.  cap_end: what the plan reports as the end of the writes to out.
int pnge_batch(hipStream_t st, uint8_t* ws, const uint8_t* src, int nb, const PngeGeom& g, uint8_t* out, int32_t* sizes, long long* total,
               bool first, long long cap_end) {
    auto up = [](long long v) { return (v + 15) & ~15ll; };
    const long long n = (long long)nb * g.nseg, rows = (long long)nb * g.H;
    uint8_t* raw = ws;
    uint8_t* slots = raw + nb * g.raw_pitch;
    long long* file_off = (long long*)(slots + n * (g.S + kPngeSlotPad));
    uint32_t* parts = (uint32_t*)((uint8_t*)file_off + up(8ll * nb));
    int* lens = (int*)((uint8_t*)parts + up(8 * rows));
    uint32_t* crcs = (uint32_t*)((uint8_t*)lens + up(4 * n));
    int* seg_off = (int*)((uint8_t*)crcs + up(4 * n));
    uint32_t* file_crc = (uint32_t*)((uint8_t*)seg_off + up(4 * n));
    uint32_t* file_adler = (uint32_t*)((uint8_t*)file_crc + up(4ll * nb));
    plan_need(pnge_ws_bytes(g, nb), 0);
    OG_LAUNCH(k_pnge_filter, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, src, rows, g.H, g.W, g.C, g.raw_pitch, raw, parts);
    OG_LAUNCH(k_pnge_segment, dim3((unsigned)g.nseg, (unsigned)nb), dim3(kPngeThreads), 0, st, (const uint8_t*)raw, g.raw_pitch, g.N, g.S, g.nseg, slots,
              lens, crcs);
    if (g_plan)   // static LDS: stated, so that the plan tells the truth
        g_plan->recs.back().lds = (unsigned)(kPngeMaxSeg + kPngeMaxSeg + kPngeSlotPad + sizeof(OgPngeCode) + 4 * kPngeThreads + 4);
    OG_LAUNCH(k_pnge_offsets, dim3(1), dim3(kPngeThreads), 0, st, (const int*)lens, (const uint32_t*)crcs, (const uint32_t*)parts, g.nseg, nb, g.H, g.N,
              first ? 1 : 0, total, sizes, file_off, seg_off, file_crc, file_adler);
    if (g_plan) {
        g_plan->recs.back().lds = 8 * kPngeThreads;
        plan_write("sizes", sizes, (long long)nb * 4);
        plan_write("total", total, 8);
    }
    OG_LAUNCH(k_pnge_place, dim3((unsigned)g.nseg, (unsigned)nb), dim3(256), 0, st, (const uint8_t*)slots, (const int*)lens, (const int*)seg_off,
              (const long long*)file_off, (const uint32_t*)file_crc, (const uint32_t*)file_adler, g.nseg, g.S, g.H, g.W, g.C, out);
    if (g_plan) plan_write("out", out, cap_end);
    return OG_OK;
}

int check_pnge(og_pnge* h, int B, int H, int W, int C, size_t cap) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (B < 0) return fail(OG_EINVAL, "bad B");
    const int rc = check_pnge_shape(H, W, C, h->segment);
    if (rc) return rc;
    const unsigned long long need = (unsigned long long)B * (unsigned long long)pnge_bound(pnge_geom(H, W, C, h->segment));
    if ((unsigned long long)cap < need) return fail(OG_EINVAL, "cap is below B * og_pnge_bound(H, W, C, S) = " + std::to_string(need) + " bytes");
    return OG_OK;
}
#endif   // OG_PNG_HOST_ONLY

}  // namespace

extern "C" {

long long og_pnge_limit(int which) {
    switch (which) {
        case 0: return kMjpegMaxPixels;
        case 1: return kPngeMaxChunk;
        case 2: return kPngeMinSeg;
        case 3: return kPngeMaxSeg;
        case 4: return kPngeMaxSeg;
        case 5: return 128;
        case 6: return kPngeFixed;
        case 7: return (long long)(kPngeMaxSeg + kPngeMaxSeg + kPngeSlotPad + sizeof(OgPngeCode) + 4 * kPngeThreads + 4);
        default: return -1;
    }
}

long long og_pnge_bound(int H, int W, int C, int S) {
    if (check_pnge_shape(H, W, C, S)) return -1;
    return pnge_bound(pnge_geom(H, W, C, S));
}

int og_pnge_filter_host(const uint8_t* frame, int H, int W, int C, uint8_t* out, size_t cap) {
    const int rc = check_pnge_shape(H, W, C, kPngeMaxSeg);
    if (rc) return rc;
    if (!frame || !out) return fail(OG_EINVAL, "null buffer");
    const PngeGeom g = pnge_geom(H, W, C, kPngeMaxSeg);
    if ((unsigned long long)cap < (unsigned long long)g.N) return fail(OG_EINVAL, "cap is below H * (1 + W * C) = " + std::to_string(g.N) + " bytes");
    pnge_filter_host(frame, g, out);
    return OG_OK;
}

int og_pnge_deflate_host(const uint8_t* raw, size_t n, int S, uint8_t* out, size_t cap, size_t* size) {
    const int rc = check_pnge_shape(1, 1, 1, S);
    if (rc) return rc;
    if (!raw || !out || !size) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(size);
    if (n < 1 || n > (size_t)1 << 30) return fail(OG_EINVAL, "n must be 1..2^30 bytes");
    const long long need = pnge_zbound((long long)n, S);
    if ((unsigned long long)cap < (unsigned long long)need) return fail(OG_EINVAL, "cap is below 6 + n + 5 * ceil(n / S) = " + std::to_string(need) + " bytes");
    out[0] = 0x78;
    out[1] = 0x01;
    const long long z = pnge_segments_host(raw, (long long)n, S, out + 2, nullptr);
    uint32_t s1, s2;
    og_png_adler_part<1>(raw, (long long)n, 0, &s1, &s2);
    og_pnge_be32(out + 2 + z, og_png_adler_join(s1, s2, (long long)n));
    *size = (size_t)(2 + z + 4);
    return OG_OK;
}

int og_pnge_encode_host(const uint8_t* frame, int H, int W, int C, int S, uint8_t* out, size_t cap, int* size) {
    const int rc = check_pnge_shape(H, W, C, S);
    if (rc) return rc;
    if (!frame || !out || !size) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(size);
    const PngeGeom g = pnge_geom(H, W, C, S);
    if ((unsigned long long)cap < (unsigned long long)pnge_bound(g))
        return fail(OG_EINVAL, "cap is below og_pnge_bound(H, W, C, S) = " + std::to_string(pnge_bound(g)) + " bytes");
    *size = (int)pnge_file_host(frame, g, out);
    return OG_OK;
}

int og_pnge_label_bbox_host(const uint8_t* label, int H, int W, int32_t* box4) {
    if (!label || !box4) return fail(OG_EINVAL, "null buffer");
    if (H < 1 || W < 1 || (long long)H * W > kMjpegMaxPixels) return fail(OG_EINVAL, "bad H/W");
    OG_ALIGN(box4);
    int x0 = W, y0 = H, x1 = -1, y1 = -1;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            if (label[(size_t)y * W + x] > 0) {
                x0 = x < x0 ? x : x0;
                y0 = y < y0 ? y : y0;
                x1 = x > x1 ? x : x1;
                y1 = y > y1 ? y : y1;
            }
    og_pnge_bbox(x0, y0, x1, y1, box4);
    return OG_OK;
}

#ifndef OG_PNG_HOST_ONLY
og_pnge* og_pnge_create(void) { return new og_pnge(); }

void og_pnge_destroy(og_pnge* h) {
    og_stream_destroy(h, [h] { pnge_free(h); });
}

int og_pnge_sync(og_pnge* h) { return og_stream_sync(h); }

int og_pnge_set_chunk(og_pnge* h, int chunk) { return og_stream_set_chunk(h, chunk, kPngeMaxChunk); }

int og_pnge_set_segment(og_pnge* h, int S) {
    if (!h) return fail(OG_EINVAL, "null handle");
    const int rc = check_pnge_shape(1, 1, 1, S);
    if (rc) return rc;
    h->segment = S;
    return OG_OK;
}

int og_pnge_encode_u8_dev(og_pnge* h, const uint8_t* frames_dev, int B, int H, int W, int C, uint8_t* out_dev, size_t cap, int32_t* sizes_dev,
                          long long* total_dev) {
    int rc = check_pnge(h, B, H, W, C, cap);
    if (rc) return rc;
    OG_ALIGN(sizes_dev);
    OG_ALIGN(total_dev);
    if (B == 0) return OG_OK;
    if (!frames_dev || !out_dev || !sizes_dev || !total_dev) return fail(OG_EINVAL, "null buffer");
    if ((rc = og_stream_ready(h))) return rc;
    OG_SCOPE(h);
    const PngeGeom g = pnge_geom(H, W, C, h->segment);
    const int chunk = pnge_chunk(h->chunk, g), cb = chunk < B ? chunk : B;
    if ((rc = h->d_ws.grow(h, (size_t)pnge_ws_bytes(g, cb), "pnge"))) return rc;
    const size_t fb = (size_t)H * W * C;
    for (int b0 = 0; b0 < B && !rc; b0 += chunk) {
        const int nb = (B - b0 < chunk) ? B - b0 : chunk;
        rc = pnge_batch(h->stream, h->d_ws, frames_dev + b0 * fb, nb, g, out_dev, sizes_dev + b0, total_dev, b0 == 0, 0);
    }
    if (rc) og_stream_drain(h);
    return rc;
}

int og_pnge_encode_stream_u8(og_pnge* h, const uint8_t* frames, int B, int H, int W, int C, uint8_t* out, size_t cap, int32_t* sizes,
                             long long* total) {
    int rc = check_pnge(h, B, H, W, C, cap);
    if (rc) return rc;
    OG_ALIGN(sizes);
    OG_ALIGN(total);
    if (B > 0 && (!frames || !out || !sizes)) return fail(OG_EINVAL, "null buffer");
    if (!total) return fail(OG_EINVAL, "total is null");
    if (B == 0) {
        *total = 0;
        return OG_OK;
    }
    if ((rc = og_stream_ready(h))) return rc;
    OG_SCOPE(h);
    const PngeGeom g = pnge_geom(H, W, C, h->segment);
    const int chunk = pnge_chunk(h->chunk, g), cb = chunk < B ? chunk : B;
    const long long bound = pnge_bound(g);
    const size_t fb = (size_t)H * W * C, meta = 8 + (size_t)cb * 4;
    if ((rc = h->d_ws.grow(h, (size_t)pnge_ws_bytes(g, cb), "pnge"))) return rc;
    if ((rc = h->d_in.grow(h, cb * fb, "pnge"))) return rc;
    if ((rc = h->d_out.grow(h, (size_t)cb * bound, "pnge"))) return rc;
    if ((rc = h->d_meta.grow(h, meta, "pnge"))) return rc;
    for (auto& s : h->slots) {
        if ((rc = s.h_in.grow(h, cb * fb, "pnge"))) return rc;
        if ((rc = s.h_meta.grow(h, meta, "pnge"))) return rc;
        if (!s.ev) HIPCHK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    }
    const hipStream_t st = h->stream;
    long long at = 0;

    auto retire = [&](og_pnge::Slot& s) -> int {
        if (s.b0 < 0) return OG_OK;
        s.b0 = -1;
        HIPCHK(hipEventSynchronize(s.ev));
        memcpy(out + s.at, s.h_out, (size_t)s.bytes);
        return OG_OK;
    };
    auto fill = [&](og_pnge::Slot& s, int b0, int nb) -> int {
        memcpy(s.h_in, frames + (size_t)b0 * fb, nb * fb);
        HIPCHK(hipMemcpyAsync(h->d_in, s.h_in, nb * fb, hipMemcpyHostToDevice, st));
        const int rc2 = pnge_batch(st, h->d_ws, h->d_in, nb, g, h->d_out, (int32_t*)(h->d_meta + 8), (long long*)h->d_meta.p, true, 0);
        if (rc2) return rc2;
        HIPCHK(hipMemcpyAsync(s.h_meta, h->d_meta, 8 + (size_t)nb * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(s.ev, st));
        HIPCHK(hipEventSynchronize(s.ev));   // the micro-batch's one number: its bytes
        const long long bytes = *(const long long*)s.h_meta.p;
        if (bytes < 0 || bytes > (long long)nb * bound) return fail(OG_EHIP, "the device reported an impossible size");
        memcpy(sizes + b0, s.h_meta + 8, (size_t)nb * 4);
        if ((size_t)bytes > s.h_out.cap || !s.h_out) {   // (grows drain the stream: nothing of this slot is in flight)
            const int rc3 = s.h_out.grow(h, ((size_t)bytes + (1u << 20)) & ~(size_t)((1u << 20) - 1), "pnge");
            if (rc3) return rc3;
        }
        HIPCHK(hipMemcpyAsync(s.h_out, h->d_out, (size_t)bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(s.ev, st));
        s.b0 = b0;
        s.nb = nb;
        s.at = at;
        s.bytes = bytes;
        at += bytes;
        return OG_OK;
    };

    rc = og_two_slot(B, chunk, h->slots, retire, fill, [h] { og_stream_drain(h); });
    if (!rc) *total = at;
    return rc;
}

int og_pnge_label_bbox_u8_dev(og_pnge* h, const uint8_t* labels_dev, int B, int H, int W, int32_t* boxes_dev) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (B < 0 || B > 65535 * 1024) return fail(OG_EINVAL, "bad B");
    if (H < 1 || W < 1 || (long long)H * W > kMjpegMaxPixels) return fail(OG_EINVAL, "bad H/W");
    OG_ALIGN(boxes_dev);
    if (B == 0) return OG_OK;
    if (!labels_dev || !boxes_dev) return fail(OG_EINVAL, "null buffer");
    int rc = og_stream_ready(h);
    if (rc) return rc;
    OG_SCOPE(h);
    OG_LAUNCH(k_label_bbox, dim3((unsigned)B), dim3(256), 0, h->stream, labels_dev, H, W, boxes_dev);
    return OG_OK;
}

int og_pnge_crop_tiles_u8_dev(og_pnge* h, const uint8_t* frames_dev, int B, int H, int W, int channels, const int32_t* boxes_dev, int size,
                              uint8_t* tiles_dev) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (B < 0 || B > 65535) return fail(OG_EINVAL, "B must be 0..65535");
    if (H < 1 || W < 1 || size < 1 || H > kResizeMaxSide || W > kResizeMaxSide || size > kResizeMaxSide)
        return fail(OG_EINVAL, "frame and tile sides must be 1.." + std::to_string(kResizeMaxSide));
    if (channels != 1 && channels != 3) return fail(OG_EINVAL, "channels must be 1 (gray) or 3 (BGR)");
    OG_ALIGN(boxes_dev);
    if (B == 0) return OG_OK;
    if (!frames_dev || !boxes_dev || !tiles_dev) return fail(OG_EINVAL, "null buffer");
    int rc = og_stream_ready(h);
    if (rc) return rc;
    OG_SCOPE(h);
    return enqueue_crop_in(h->stream, channels, frames_dev, B, H, W, boxes_dev, size, tiles_dev);
}

int og_pnge_plan(int B, int H, int W, int C, int S, int chunk, char* out, size_t cap, long long* workspace_bytes) {
    if (!out || cap == 0 || B < 1) return fail(OG_EINVAL, "bad argument");
    int rc = check_pnge_shape(H, W, C, S);
    if (rc) return rc;
    if ((rc = og_check_chunk(chunk, kPngeMaxChunk))) return rc;
    const PngeGeom g = pnge_geom(H, W, C, S);
    const int mb = pnge_chunk(chunk, g), cb = mb < B ? mb : B;
    const long long bound = pnge_bound(g);
    if (workspace_bytes) *workspace_bytes = pnge_ws_bytes(g, cb) + (long long)cb * ((long long)H * W * C + bound + 4) + 8;
    const uintptr_t gap = (uintptr_t)1 << 40;   // placeholder bases: nothing dereferences them in a dry run
    uint8_t* dst = (uint8_t*)(1 * gap);
    int32_t* sz = (int32_t*)(2 * gap);
    long long* tot = (long long*)(3 * gap);
    Plan plan;
    plan.bases = {{"out", dst}, {"sizes", sz}, {"total", tot}};
    g_plan = &plan;
    for (int b0 = 0; b0 < B && !rc; b0 += mb) {
        const int nb = (B - b0 < mb) ? B - b0 : mb;
        // the files of frames [b0, b0 + nb) end no later than (b0 + nb) * bound bytes into the caller's out
        rc = pnge_batch(nullptr, (uint8_t*)(4 * gap), (const uint8_t*)(5 * gap), nb, g, dst, sz + b0, tot, b0 == 0, (long long)(b0 + nb) * bound);
    }
    g_plan = nullptr;
    if (rc) return rc;
    return og_plan_text(plan, kPlanWrites, out, cap);
}
#endif   // OG_PNG_HOST_ONLY

}  // extern "C"
