// Baseline JPEG on the device (include/openglottal_hip_mjpeg.h): the frames k_overlay leaves become complete JPEG files, the chunks of
// a Motion-JPEG AVI.  Included by og_api.hip, as og_overlay.inc is; the kernels live here too.  A handle of its own: one stream, the
// workspace of ONE micro-batch, two pinned host slots.  Per micro-batch: k_mjpeg_transform (coefficients), k_mjpeg_entropy (a wave per
// restart interval, its bytes into its slot), k_mjpeg_offsets (prefix sum over intervals and frames), k_mjpeg_place (dense files in
// the caller's buffer).  Every slot, length and offset a launch reads was written by the launch before it, so a handle carries nothing
// from call to call.  All arithmetic is integer: the host twins and the kernels call the same inline functions and agree byte for byte.
#include "../../include/openglottal_hip_mjpeg.h"

#define OG_JPEG_HD __host__ __device__ inline

constexpr int kJpegRi = 16;                                  // MCUs per restart interval
constexpr int kJpegBlocks = kJpegRi * 3;                     // blocks per interval: a lane each
constexpr int kJpegBlockBytes = 2 * ((63 * 26 + 22 + 7) / 8);   // 416: a block after byte stuffing, worst case
constexpr int kJpegSlot = kJpegBlocks * kJpegBlockBytes + 4;    // 19972: an interval and its marker, a multiple of 4
constexpr int kJpegBitWords = (kJpegBlocks * (63 * 26 + 22) + 7 + 31) / 32 + 1;   // the interval's bit string before stuffing
constexpr int kJpegCoefStride = 66;                          // int16 per block in LDS: 33 dwords, so lanes hit different banks
constexpr int kJpegHdrLen = 629;
constexpr long long kMjpegMaxPixels = 1ll << 24;
constexpr int kMjpegMaxChunk = 1024;
constexpr long long kMjpegBatchBytes = 256ll << 20;          // of workspace per micro-batch

// what the kernels read beside the frames: built on the host for a (quality, H, W), one copy on the device per handle
struct MjpegTab {
    uint16_t q[2][64];        // quantisation tables, natural order
    uint8_t zzpos[64];        // natural index -> zigzag position
    uint32_t huff[2][272];    // code << 8 | length; [0, 256) AC symbols, 256 + category DC; table 0 luminance, 1 chrominance
    uint8_t hdr[640];         // SOI through SOS
};

// ---- the arithmetic: host twin and kernels ---------------------------------------------------------------------------------------
// BGR -> Y, Cb, Cr with 4 fraction bits, level shifted (|.| <= 2048)
OG_JPEG_HD void og_jpeg_ycc(int b, int g, int r, int* y, int* cb, int* cr) {
    *y = ((19595 * r + 38470 * g + 7471 * b + 2048) >> 12) - 2048;
    *cb = (-11059 * r - 21709 * g + 32768 * b + 2048) >> 12;
    *cr = (32768 * r - 27439 * g - 5329 * b + 2048) >> 12;
}

// round(2^14 * C(u)/2 * cos((2x+1) u pi / 16)); folds to a literal wherever u and x are known at compile time
OG_JPEG_HD constexpr int og_jpeg_dct_c(int u, int x) {
    constexpr int mag[9] = {5793, 8035, 7568, 6811, 5793, 4551, 3135, 1598, 0};   // u = 0: 2^14 / (2 sqrt 2); k: 2^13 cos(k pi / 16)
    int k = ((2 * x + 1) * u) % 32;
    if (k > 16) k = 32 - k;
    const bool neg = k > 8;
    if (neg) k = 16 - k;
    return neg ? -mag[k] : mag[k];
}

// one 1-D pass: out[u] = (sum_x c(u,x) in[x] + half) >> shift
OG_JPEG_HD void og_jpeg_dct8(const int* in, int* out, int shift) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        int acc = 1 << (shift - 1);
#pragma unroll
        for (int x = 0; x < 8; ++x) acc += og_jpeg_dct_c(u, x) * in[x];
        out[u] = acc >> shift;
    }
}

// s [8][8] samples of og_jpeg_ycc -> out [8][8] (row v, column u) coefficients with 4 fraction bits
OG_JPEG_HD void og_jpeg_fdct8x8(const int* s, int* out) {
    int t[64], col[8], res[8];
    for (int y = 0; y < 8; ++y) og_jpeg_dct8(s + 8 * y, t + 8 * y, 12);
    for (int u = 0; u < 8; ++u) {
        for (int y = 0; y < 8; ++y) col[y] = t[8 * y + u];
        og_jpeg_dct8(col, res, 16);
        for (int v = 0; v < 8; ++v) out[8 * v + u] = res[v];
    }
}

// a coefficient with 4 fraction bits over q: round half away from zero; AC clamped to +-1023
OG_JPEG_HD int og_jpeg_quant(int c, int q, bool ac) {
    const int a = c < 0 ? -c : c;
    int v = (a + 8 * q) / (16 * q);
    if (ac && v > 1023) v = 1023;
    return c < 0 ? -v : v;
}

OG_JPEG_HD int og_jpeg_bitlen(int a) { return a ? 32 - __builtin_clz((unsigned)a) : 0; }

// the codes of one block, in order, to put(bits, count), count <= 26: DC difference, then runs, ZRL and EOB
template <class Coef, class Put>
OG_JPEG_HD void og_jpeg_block(Coef coef, int pred, const uint32_t* huff, Put put) {
    const int d = coef(0) - pred;
    int cat = og_jpeg_bitlen(d < 0 ? -d : d);
    uint32_t e = huff[256 + cat];
    put(((e >> 8) << cat) | (uint32_t)((d < 0 ? d - 1 : d) & ((1 << cat) - 1)), (int)(e & 255) + cat);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = coef(k);
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run >= 16; run -= 16) {   // at most three
            e = huff[0xF0];
            put(e >> 8, (int)(e & 255));
        }
        cat = og_jpeg_bitlen(v < 0 ? -v : v);
        e = huff[(run << 4) | cat];
        put(((e >> 8) << cat) | (uint32_t)((v < 0 ? v - 1 : v) & ((1 << cat) - 1)), (int)(e & 255) + cat);
        run = 0;
    }
    if (run) {
        e = huff[0];
        put(e >> 8, (int)(e & 255));
    }
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------
constexpr int kJpegTransformLds = 32 * (3 * 8 * 9 + 96) * 4;   // per 8-lane group: a padded [3][8][9] int tile, 96 dwords of coefficients

// 8 lanes per pixel block.  A lane loads one row of 8 pixels (six aligned dwords where the row allows it), converts, runs the row
// pass; after the transpose through the padded tile it runs the column pass of column `r`, quantises and drops the values at their
// zigzag places; then the group's 384 bytes go out as dwords, lane after lane.
__global__ __launch_bounds__(256) void k_mjpeg_transform(const uint8_t* __restrict__ frames, long long nblocks, int M, int mx, int H, int W,
                                                         const MjpegTab* __restrict__ tab, int16_t* __restrict__ coefs) {
    extern __shared__ uint32_t lds_t[];
    int* tile = (int*)lds_t;                 // [32][3][8][9]
    uint32_t* stage = lds_t + 32 * 216;      // [32][96]
    const int g = threadIdx.x >> 3, r = threadIdx.x & 7;
    const long long blk = (long long)blockIdx.x * 32 + g;
    const bool valid = blk < nblocks;
    int* tg = tile + g * 216;
    if (valid) {
        const long long f = blk / M;
        const int m = (int)(blk - f * M), by = m / mx, bx = m - by * mx;
        const int y = min(by * 8 + r, H - 1), x0 = bx * 8;
        const uint8_t* row = frames + ((f * H + y) * W) * 3;
        int px[24];
        if (x0 + 8 <= W && (((uintptr_t)(row + 3 * x0)) & 3) == 0) {
            const uint32_t* p = (const uint32_t*)(row + 3 * x0);
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const uint32_t w = p[j];
#pragma unroll
                for (int i = 0; i < 4; ++i) px[4 * j + i] = (int)((w >> (8 * i)) & 255);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint8_t* p = row + 3 * min(x0 + i, W - 1);
                px[3 * i] = p[0];
                px[3 * i + 1] = p[1];
                px[3 * i + 2] = p[2];
            }
        }
        int s[3][8], o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) og_jpeg_ycc(px[3 * i], px[3 * i + 1], px[3 * i + 2], &s[0][i], &s[1][i], &s[2][i]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            og_jpeg_dct8(s[c], o, 12);
#pragma unroll
            for (int u = 0; u < 8; ++u) tg[(c * 8 + r) * 9 + u] = o[u];
        }
    }
    __syncthreads();
    if (valid) {
        int16_t* sg = (int16_t*)(stage + g * 96);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int col[8], o[8];
#pragma unroll
            for (int y = 0; y < 8; ++y) col[y] = tg[(c * 8 + y) * 9 + r];
            og_jpeg_dct8(col, o, 16);
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                const int n = 8 * v + r;
                sg[c * 64 + tab->zzpos[n]] = (int16_t)og_jpeg_quant(o[v], tab->q[c ? 1 : 0][n], n != 0);
            }
        }
    }
    __syncthreads();
    if (valid) {
        uint32_t* dst = (uint32_t*)(coefs + blk * 192);
#pragma unroll
        for (int k = 0; k < 12; ++k) dst[r + 8 * k] = stage[g * 96 + r + 8 * k];
    }
}

constexpr int kJpegEntropyLds = (kJpegBlocks * (kJpegCoefStride / 2) + kJpegBitWords + kJpegSlot / 4 + 544 + 64) * 4;

// inclusive prefix sum over the wave's 64 lanes through LDS; every lane calls it
__device__ inline int og_jpeg_scan64(int* s, int t, int v) {
    s[t] = v;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int a = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += a;
        __syncthreads();
    }
    return s[t];
}

// `n` bits (n <= 26) at bit `pos` of the MSB-first string; lanes share words, so the bits are OR-ed in
__device__ inline void og_jpeg_put(uint32_t* bits, int pos, uint32_t v, int n) {
    const int w = pos >> 5, room = 32 - (pos & 31);
    if (n <= room) {
        atomicOr(&bits[w], v << (room - n));
    } else {
        atomicOr(&bits[w], v >> (n - room));
        atomicOr(&bits[w + 1], v << (32 - (n - room)));
    }
}

// One wave per restart interval k of frame f: grid (nI, nb).
__global__ __launch_bounds__(64) void k_mjpeg_entropy(const int16_t* __restrict__ coefs, int M, int nI, const MjpegTab* __restrict__ tab,
                                                      uint8_t* __restrict__ slots, int* __restrict__ lens) {
    extern __shared__ uint32_t lds_e[];
    uint32_t* sc32 = lds_e;                                        // coefficients, kJpegCoefStride int16 per block
    uint32_t* sbits = sc32 + kJpegBlocks * (kJpegCoefStride / 2);
    uint32_t* sout32 = sbits + kJpegBitWords;
    uint32_t* shuff = sout32 + kJpegSlot / 4;
    int* sscan = (int*)(shuff + 544);
    const int16_t* sc = (const int16_t*)sc32;
    uint8_t* sout = (uint8_t*)sout32;
    const int k = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    const int m0 = k * kJpegRi, nblk = 3 * min(kJpegRi, M - m0);
    const uint32_t* src = (const uint32_t*)(coefs + ((long long)f * M + m0) * 192);
    for (int i = t; i < nblk * 32; i += 64) sc32[(i >> 5) * (kJpegCoefStride / 2) + (i & 31)] = src[i];
    for (int i = t; i < 544; i += 64) shuff[i] = tab->huff[0][i];
    for (int i = t; i < kJpegBitWords; i += 64) sbits[i] = 0;
    __syncthreads();

    const bool active = t < nblk;
    const uint32_t* huff = shuff + ((t % 3) ? 272 : 0);
    const int pred = (active && t >= 3) ? sc[(t - 3) * kJpegCoefStride] : 0;
    const int16_t* mine = sc + t * kJpegCoefStride;
    int nbits = 0;
    if (active) og_jpeg_block([mine](int i) { return (int)mine[i]; }, pred, huff, [&nbits](uint32_t, int n) { nbits += n; });
    const int incl = og_jpeg_scan64(sscan, t, nbits);
    const int total = sscan[63];
    __syncthreads();
    if (active) {
        int pos = incl - nbits;
        og_jpeg_block([mine](int i) { return (int)mine[i]; }, pred, huff, [&pos, sbits](uint32_t v, int n) {
            og_jpeg_put(sbits, pos, v, n);
            pos += n;
        });
    }
    const int pad = (8 - (total & 7)) & 7;
    if (t == 0 && pad) og_jpeg_put(sbits, total, (1u << pad) - 1, pad);
    __syncthreads();

    const int nbytes = (total + 7) >> 3, span = (nbytes + 63) >> 6;
    const int lo = min(t * span, nbytes), hi = min(lo + span, nbytes);
    int ff = 0;
    for (int j = lo; j < hi; ++j) ff += ((sbits[j >> 2] >> (24 - 8 * (j & 3))) & 255) == 255;
    const int ffincl = og_jpeg_scan64(sscan, t, ff);
    int len = nbytes + sscan[63];
    int o = lo + ffincl - ff;
    for (int j = lo; j < hi; ++j) {
        const uint32_t b = (sbits[j >> 2] >> (24 - 8 * (j & 3))) & 255;
        sout[o++] = (uint8_t)b;
        if (b == 255) sout[o++] = 0;
    }
    if (k != nI - 1) {
        if (t == 0) {
            sout[len] = 0xFF;
            sout[len + 1] = (uint8_t)(0xD0 + (k & 7));
        }
        len += 2;
    }
    __syncthreads();
    const long long i = (long long)f * nI + k;
    uint32_t* dst = (uint32_t*)(slots + i * kJpegSlot);
    for (int j = t; j < (len + 3) >> 2; j += 64) dst[j] = sout32[j];
    if (t == 0) lens[i] = len;
}

// One workgroup: off[i] = where interval i goes in the caller's buffer, sizes[f], and the running total.  n = nb * nI.
__global__ __launch_bounds__(1024) void k_mjpeg_offsets(const int* __restrict__ lens, int n, int nI, int nb, int first, long long* total,
                                                        int32_t* __restrict__ sizes, long long* off) {
    __shared__ long long ssum[1024];
    const int t = threadIdx.x, per = (n + 1023) >> 10;
    const int lo = min(t * per, n), hi = min(lo + per, n);
    long long s = 0;
    for (int i = lo; i < hi; ++i) s += lens[i];
    ssum[t] = s;
    const long long base = first ? 0 : *total;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < 1024; d <<= 1) {
        const long long a = t >= d ? ssum[t - d] : 0;
        __syncthreads();
        ssum[t] += a;
        __syncthreads();
    }
    long long run = ssum[t] - s;
    const long long end = base + (long long)nb * (kJpegHdrLen + 2) + ssum[1023];
    for (int i = lo; i < hi; ++i) {
        const int f = i / nI;
        __hip_atomic_store(&off[i], base + (long long)(f + 1) * kJpegHdrLen + 2ll * f + run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        run += lens[i];
    }
    __syncthreads();
    for (int f = t; f < nb; f += 1024) {
        const long long a = __hip_atomic_load(&off[(long long)f * nI], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - kJpegHdrLen;
        const long long b =
            f + 1 < nb ? __hip_atomic_load(&off[(long long)(f + 1) * nI], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - kJpegHdrLen : end;
        sizes[f] = (int32_t)(b - a);
    }
    if (t == 0) *total = end;
}

// A workgroup per interval: grid (nI, nb).
__global__ __launch_bounds__(256) void k_mjpeg_place(const uint8_t* __restrict__ slots, const int* __restrict__ lens,
                                                     const long long* __restrict__ off, int nI, const MjpegTab* __restrict__ tab,
                                                     uint8_t* __restrict__ out) {
    const int k = blockIdx.x, t = threadIdx.x;
    const long long i = (long long)blockIdx.y * nI + k;
    const int len = lens[i];
    const uint8_t* src = slots + i * kJpegSlot;
    uint8_t* dst = out + off[i];
    for (int j = t; j < len; j += 256) dst[j] = src[j];
    if (k == 0)
        for (int j = t; j < kJpegHdrLen; j += 256) dst[j - kJpegHdrLen] = tab->hdr[j];
    if (k == nI - 1 && t < 2) dst[len + t] = t ? 0xD9 : 0xFF;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct og_mjpeg : OgStreamHandle {
    int quality = 75;
    MjpegTab* d_tab = nullptr;
    int tab_q = 0, tab_H = 0, tab_W = 0;   // what d_tab holds
    // each buffer holds the bytes of the largest micro-batch run so far
    OgBuf<uint8_t> d_ws;   // coefficients, slots, lengths, offsets
    OgBuf<uint8_t> d_in, d_out;
    OgBuf<uint8_t> d_meta;   // streamed entry: total (8 bytes), then the sizes
    struct Slot {
        OgBuf<uint8_t> h_in{true}, h_out{true}, h_meta{true};
        hipEvent_t ev = nullptr;
        int b0 = -1, nb = 0;
        long long at = 0, bytes = 0;   // where in the caller's out, how many
    } slots[2];
};

namespace {

#include "og_jpeg_annexk.inc"

struct MjpegGeom {
    int mx, my, M, nI;
};
MjpegGeom mjpeg_geom(int H, int W) {
    MjpegGeom g;
    g.mx = (W + 7) / 8;
    g.my = (H + 7) / 8;
    g.M = g.mx * g.my;
    g.nI = (g.M + kJpegRi - 1) / kJpegRi;
    return g;
}
long long mjpeg_bound(int H, int W) {
    const MjpegGeom g = mjpeg_geom(H, W);
    return kJpegHdrLen + (long long)g.M * 3 * kJpegBlockBytes + 2ll * g.nI + 2;
}
// device workspace per frame: coefficients, slots, lengths, offsets (each part a multiple of 4 bytes; offsets kept 8-aligned by the layout)
long long mjpeg_frame_ws(const MjpegGeom& g) { return (long long)g.M * 384 + (long long)g.nI * (kJpegSlot + 12); }
int mjpeg_chunk(int chunk, const MjpegGeom& g) {
    const long long fit = kMjpegBatchBytes / mjpeg_frame_ws(g);
    return (int)(fit < 1 ? 1 : (fit < chunk ? fit : chunk));
}

void mjpeg_huff(const uint8_t* bits, const uint8_t* vals, uint32_t* out) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = (code++ << 8) | (uint32_t)len;
        code <<= 1;
    }
}

void mjpeg_build_tab(int quality, int H, int W, MjpegTab* t) {
    memset(t, 0, sizeof *t);
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 64; ++i) {
            const int v = (kJpegBaseQ[c][i] * s + 50) / 100;
            t->q[c][i] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
    for (int k = 0; k < 64; ++k) t->zzpos[kJpegZigzag[k]] = (uint8_t)k;
    for (int c = 0; c < 2; ++c) {
        mjpeg_huff(kJpegAcBits[c], kJpegAcVals[c], t->huff[c]);
        uint32_t dc[16] = {0};
        mjpeg_huff(kJpegDcBits[c], kJpegDcVals, dc);
        for (int i = 0; i < 12; ++i) t->huff[c][256 + i] = dc[i];
    }
    uint8_t* p = t->hdr;
    auto put = [&p](std::initializer_list<int> v) {
        for (int b : v) *p++ = (uint8_t)b;
    };
    put({0xFF, 0xD8});
    put({0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int c = 0; c < 2; ++c) {
        put({0xFF, 0xDB, 0, 67, c});
        for (int k = 0; k < 64; ++k) *p++ = (uint8_t)t->q[c][kJpegZigzag[k]];
    }
    put({0xFF, 0xC0, 0, 17, 8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int c = 0; c < 2; ++c) {
        put({0xFF, 0xC4, 0, 2 + 1 + 16 + 12, c});
        for (int i = 0; i < 16; ++i) *p++ = kJpegDcBits[c][i];
        for (int i = 0; i < 12; ++i) *p++ = kJpegDcVals[i];
        put({0xFF, 0xC4, 0, 2 + 1 + 16 + 162, 0x10 | c});
        for (int i = 0; i < 16; ++i) *p++ = kJpegAcBits[c][i];
        for (int i = 0; i < 162; ++i) *p++ = kJpegAcVals[c][i];
    }
    put({0xFF, 0xDD, 0, 4, kJpegRi >> 8, kJpegRi & 255});
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    static_assert(sizeof t->hdr >= kJpegHdrLen, "header buffer");
}

int check_jpeg_shape(int H, int W) {
    if (H <= 0 || W <= 0) return fail(OG_EINVAL, "bad H/W");
    if (H > 65535 || W > 65535) return fail(OG_EINVAL, "H and W must fit SOF0's 16 bits");
    if ((long long)H * W > kMjpegMaxPixels) return fail(OG_EINVAL, "H*W above " + std::to_string(kMjpegMaxPixels) + " pixels");
    return OG_OK;
}
int check_jpeg_quality(int quality) {
    if (quality < 1 || quality > 100) return fail(OG_EINVAL, "quality must be 1..100");
    return OG_OK;
}

void mjpeg_coefficients_host(const uint8_t* frame, int H, int W, const MjpegTab& t, int16_t* out) {
    const MjpegGeom g = mjpeg_geom(H, W);
    for (int m = 0; m < g.M; ++m) {
        const int by = m / g.mx, bx = m - by * g.mx;
        int s[3][64], c16[64];
        for (int r = 0; r < 8; ++r)
            for (int i = 0; i < 8; ++i) {
                const int y = std::min(by * 8 + r, H - 1), x = std::min(bx * 8 + i, W - 1);
                const uint8_t* p = frame + ((size_t)y * W + x) * 3;
                og_jpeg_ycc(p[0], p[1], p[2], &s[0][8 * r + i], &s[1][8 * r + i], &s[2][8 * r + i]);
            }
        for (int c = 0; c < 3; ++c) {
            og_jpeg_fdct8x8(s[c], c16);
            int16_t* o = out + ((size_t)m * 3 + c) * 64;
            for (int n = 0; n < 64; ++n) o[t.zzpos[n]] = (int16_t)og_jpeg_quant(c16[n], t.q[c ? 1 : 0][n], n != 0);
        }
    }
}

// the scan of one frame from its coefficients, interval by interval as k_mjpeg_entropy does it; returns the end
uint8_t* mjpeg_scan_host(const int16_t* coefs, const MjpegGeom& g, const MjpegTab& t, uint8_t* p) {
    for (int k = 0; k < g.nI; ++k) {
        const int m0 = k * kJpegRi, nm = std::min(kJpegRi, g.M - m0);
        uint64_t acc = 0;
        int have = 0;
        auto byte = [&p](uint32_t b) {
            *p++ = (uint8_t)b;
            if (b == 255) *p++ = 0;
        };
        auto put = [&](uint32_t v, int n) {
            acc = (acc << n) | v;
            have += n;
            for (; have >= 8; have -= 8) byte((uint32_t)(acc >> (have - 8)) & 255);
        };
        for (int b = 0; b < 3 * nm; ++b) {
            const int16_t* mine = coefs + ((size_t)m0 * 3 + b) * 64;
            og_jpeg_block([mine](int i) { return (int)mine[i]; }, b >= 3 ? mine[-192] : 0, t.huff[(b % 3) ? 1 : 0], put);
        }
        if (have) put((1u << (8 - have)) - 1, 8 - have);
        if (k != g.nI - 1) {
            *p++ = 0xFF;
            *p++ = (uint8_t)(0xD0 + (k & 7));
        }
    }
    return p;
}

// the tables and the header of (quality, H, W) on the device
int mjpeg_ensure_tab(og_mjpeg* h, int H, int W) {
    if (h->d_tab && h->tab_q == h->quality && h->tab_H == H && h->tab_W == W) return OG_OK;
    MjpegTab t;
    mjpeg_build_tab(h->quality, H, W, &t);
    h->tab_q = 0;
    HIPCHK(hipStreamSynchronize(h->stream));   // (launches in flight read the old tables; the pageable source must outlive the copy)
    if (!h->d_tab) HIPCHK(hipMalloc((void**)&h->d_tab, sizeof(MjpegTab)));
    HIPCHK(hipMemcpy(h->d_tab, &t, sizeof t, hipMemcpyHostToDevice));
    h->tab_q = h->quality;
    h->tab_H = H;
    h->tab_W = W;
    return OG_OK;
}

void mjpeg_free(og_mjpeg* h) {
    if (h->d_tab) (void)hipFree(h->d_tab);
    og_release(h->d_ws, h->d_in, h->d_out, h->d_meta);
    for (auto& s : h->slots) {
        og_release(s.h_in, s.h_out, s.h_meta);
        if (s.ev) (void)hipEventDestroy(s.ev);
    }
}

// One micro-batch of nb resident frames.  ws: the handle's workspace (a placeholder in a dry run).  `first`: the files start at
// out[0]; otherwise at out[*total].  sizes: of these nb frames.  cap_end: what the plan reports as the end of the writes to out.
int mjpeg_batch(hipStream_t st, uint8_t* ws, const MjpegTab* tab, const uint8_t* src, int nb, int H, int W, uint8_t* out, int32_t* sizes,
                long long* total, bool first, long long cap_end) {
    const MjpegGeom g = mjpeg_geom(H, W);
    const long long nblocks = (long long)nb * g.M, n = (long long)nb * g.nI;
    int16_t* coefs = (int16_t*)ws;
    uint8_t* slots = ws + nblocks * 384;
    long long* off = (long long*)(slots + ((n * kJpegSlot + 7) & ~7ll));
    int* lens = (int*)(off + n);
    plan_need((long long)nb * mjpeg_frame_ws(g) + 8, 0);
    OG_LAUNCH(k_mjpeg_transform, dim3((unsigned)((nblocks + 31) / 32)), dim3(256), kJpegTransformLds, st, src, nblocks, g.M, g.mx, H, W, tab, coefs);
    OG_LAUNCH(k_mjpeg_entropy, dim3((unsigned)g.nI, (unsigned)nb), dim3(64), kJpegEntropyLds, st, (const int16_t*)coefs, g.M, g.nI, tab, slots,
              lens);
    OG_LAUNCH(k_mjpeg_offsets, dim3(1), dim3(1024), 0, st, (const int*)lens, (int)n, g.nI, nb, first ? 1 : 0, total, sizes, off);
    if (g_plan) {
        plan_write("sizes", sizes, (long long)nb * 4);
        plan_write("total", total, 8);
    }
    OG_LAUNCH(k_mjpeg_place, dim3((unsigned)g.nI, (unsigned)nb), dim3(256), 0, st, (const uint8_t*)slots, (const int*)lens, (const long long*)off,
              g.nI, tab, out);
    if (g_plan) plan_write("out", out, cap_end);
    return OG_OK;
}

int check_mjpeg(og_mjpeg* h, int B, int H, int W, size_t cap) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (B < 0) return fail(OG_EINVAL, "bad B");
    const int rc = check_jpeg_shape(H, W);
    if (rc) return rc;
    if ((unsigned long long)cap < (unsigned long long)B * (unsigned long long)mjpeg_bound(H, W))
        return fail(OG_EINVAL, "cap is below B * og_jpeg_bound(H, W) = " + std::to_string((long long)B * mjpeg_bound(H, W)) + " bytes");
    return OG_OK;
}

}  // namespace

extern "C" {

long long og_mjpeg_limit(int which) {
    switch (which) {
        case 0: return kMjpegMaxPixels;
        case 1: return kJpegRi;
        case 2: return kMjpegMaxChunk;
        case 3: return 1;
        case 4: return 100;
        case 5: return kJpegSlot;
        case 6: return kJpegHdrLen;
        case 7: return 75;
        default: return -1;
    }
}

long long og_jpeg_bound(int H, int W) {
    if (check_jpeg_shape(H, W)) return -1;
    return mjpeg_bound(H, W);
}

int og_jpeg_tables_host(int quality, int H, int W, uint8_t* qlum64, uint8_t* qchroma64, uint8_t* header_or_null, size_t header_cap,
                        int* header_len_or_null) {
    int rc = check_jpeg_quality(quality);
    if (rc || (rc = check_jpeg_shape(H, W))) return rc;
    if (!qlum64 || !qchroma64) return fail(OG_EINVAL, "null table");
    OG_ALIGN(header_len_or_null);
    if (header_or_null && header_cap < (size_t)kJpegHdrLen) return fail(OG_EINVAL, "header_cap is below " + std::to_string(kJpegHdrLen) + " bytes");
    MjpegTab t;
    mjpeg_build_tab(quality, H, W, &t);
    for (int i = 0; i < 64; ++i) {
        qlum64[i] = (uint8_t)t.q[0][i];
        qchroma64[i] = (uint8_t)t.q[1][i];
    }
    if (header_or_null) memcpy(header_or_null, t.hdr, kJpegHdrLen);
    if (header_len_or_null) *header_len_or_null = kJpegHdrLen;
    return OG_OK;
}

int og_jpeg_coefficients_host(const uint8_t* frame, int H, int W, int quality, int16_t* out) {
    int rc = check_jpeg_quality(quality);
    if (rc || (rc = check_jpeg_shape(H, W))) return rc;
    if (!frame || !out) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(out);
    MjpegTab t;
    mjpeg_build_tab(quality, H, W, &t);
    mjpeg_coefficients_host(frame, H, W, t, out);
    return OG_OK;
}

int og_jpeg_encode_host(const uint8_t* frame, int H, int W, int quality, uint8_t* out, size_t cap, int* size) {
    int rc = check_jpeg_quality(quality);
    if (rc || (rc = check_jpeg_shape(H, W))) return rc;
    if (!frame || !out || !size) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(size);
    if ((unsigned long long)cap < (unsigned long long)mjpeg_bound(H, W))
        return fail(OG_EINVAL, "cap is below og_jpeg_bound(H, W) = " + std::to_string(mjpeg_bound(H, W)) + " bytes");
    MjpegTab t;
    mjpeg_build_tab(quality, H, W, &t);
    const MjpegGeom g = mjpeg_geom(H, W);
    std::vector<int16_t> coefs((size_t)g.M * 192);
    mjpeg_coefficients_host(frame, H, W, t, coefs.data());
    memcpy(out, t.hdr, kJpegHdrLen);
    uint8_t* p = mjpeg_scan_host(coefs.data(), g, t, out + kJpegHdrLen);
    *p++ = 0xFF;
    *p++ = 0xD9;
    *size = (int)(p - out);
    return OG_OK;
}

og_mjpeg* og_mjpeg_create(void) { return new og_mjpeg(); }

void og_mjpeg_destroy(og_mjpeg* h) {
    og_stream_destroy(h, [h] { mjpeg_free(h); });
}

int og_mjpeg_sync(og_mjpeg* h) { return og_stream_sync(h); }

int og_mjpeg_set_chunk(og_mjpeg* h, int chunk) { return og_stream_set_chunk(h, chunk, kMjpegMaxChunk); }

int og_mjpeg_set_quality(og_mjpeg* h, int quality) {
    if (!h) return fail(OG_EINVAL, "null handle");
    const int rc = check_jpeg_quality(quality);
    if (rc) return rc;
    h->quality = quality;
    return OG_OK;
}

int og_mjpeg_encode_u8_dev(og_mjpeg* h, const uint8_t* frames_dev, int B, int H, int W, uint8_t* out_dev, size_t cap, int32_t* sizes_dev,
                           long long* total_dev) {
    int rc = check_mjpeg(h, B, H, W, cap);
    if (rc) return rc;
    OG_ALIGN(sizes_dev);
    OG_ALIGN(total_dev);
    if (B == 0) return OG_OK;
    if (!frames_dev || !out_dev || !sizes_dev || !total_dev) return fail(OG_EINVAL, "null buffer");
    if ((rc = og_stream_ready(h))) return rc;
    OG_SCOPE(h);
    const MjpegGeom g = mjpeg_geom(H, W);
    const int chunk = mjpeg_chunk(h->chunk, g), cb = chunk < B ? chunk : B;
    if ((rc = mjpeg_ensure_tab(h, H, W))) return rc;
    if ((rc = h->d_ws.grow(h, (size_t)cb * mjpeg_frame_ws(g) + 8, "mjpeg"))) return rc;
    const size_t fb = (size_t)H * W * 3;
    for (int b0 = 0; b0 < B && !rc; b0 += chunk) {
        const int nb = (B - b0 < chunk) ? B - b0 : chunk;
        rc = mjpeg_batch(h->stream, h->d_ws, h->d_tab, frames_dev + b0 * fb, nb, H, W, out_dev, sizes_dev + b0, total_dev, b0 == 0, 0);
    }
    if (rc) og_stream_drain(h);
    return rc;
}

int og_mjpeg_encode_stream_u8(og_mjpeg* h, const uint8_t* frames, int B, int H, int W, uint8_t* out, size_t cap, int32_t* sizes,
                              long long* total) {
    int rc = check_mjpeg(h, B, H, W, cap);
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
    const MjpegGeom g = mjpeg_geom(H, W);
    const int chunk = mjpeg_chunk(h->chunk, g), cb = chunk < B ? chunk : B;
    const size_t fb = (size_t)H * W * 3, meta = 8 + (size_t)cb * 4;
    if ((rc = mjpeg_ensure_tab(h, H, W))) return rc;
    if ((rc = h->d_ws.grow(h, (size_t)cb * mjpeg_frame_ws(g) + 8, "mjpeg"))) return rc;
    if ((rc = h->d_in.grow(h, cb * fb, "mjpeg"))) return rc;
    if ((rc = h->d_out.grow(h, (size_t)cb * mjpeg_bound(H, W), "mjpeg"))) return rc;
    if ((rc = h->d_meta.grow(h, meta, "mjpeg"))) return rc;
    for (auto& s : h->slots) {
        if ((rc = s.h_in.grow(h, cb * fb, "mjpeg"))) return rc;
        if ((rc = s.h_meta.grow(h, meta, "mjpeg"))) return rc;
        if (!s.ev) HIPCHK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    }
    const hipStream_t st = h->stream;
    long long at = 0;

    auto retire = [&](og_mjpeg::Slot& s) -> int {
        if (s.b0 < 0) return OG_OK;
        s.b0 = -1;
        HIPCHK(hipEventSynchronize(s.ev));
        memcpy(out + s.at, s.h_out, (size_t)s.bytes);
        return OG_OK;
    };
    auto fill = [&](og_mjpeg::Slot& s, int b0, int nb) -> int {
        memcpy(s.h_in, frames + (size_t)b0 * fb, nb * fb);
        HIPCHK(hipMemcpyAsync(h->d_in, s.h_in, nb * fb, hipMemcpyHostToDevice, st));
        const int rc2 = mjpeg_batch(st, h->d_ws, h->d_tab, h->d_in, nb, H, W, h->d_out, (int32_t*)(h->d_meta + 8), (long long*)h->d_meta.p, true, 0);
        if (rc2) return rc2;
        HIPCHK(hipMemcpyAsync(s.h_meta, h->d_meta, 8 + (size_t)nb * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(s.ev, st));
        HIPCHK(hipEventSynchronize(s.ev));   // the micro-batch's one number: its bytes
        const long long bytes = *(const long long*)s.h_meta.p;
        if (bytes < 0 || bytes > (long long)nb * mjpeg_bound(H, W)) return fail(OG_EHIP, "the device reported an impossible size");
        memcpy(sizes + b0, s.h_meta + 8, (size_t)nb * 4);
        if ((size_t)bytes > s.h_out.cap || !s.h_out) {   // (grows drain the stream: nothing of this slot is in flight)
            const int rc3 = s.h_out.grow(h, ((size_t)bytes + (1u << 20)) & ~(size_t)((1u << 20) - 1), "mjpeg");
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

int og_mjpeg_plan(int B, int H, int W, int chunk, char* out, size_t cap, long long* workspace_bytes) {
    if (!out || cap == 0 || B < 1) return fail(OG_EINVAL, "bad argument");
    int rc = check_jpeg_shape(H, W);
    if (rc) return rc;
    if ((rc = og_check_chunk(chunk, kMjpegMaxChunk))) return rc;
    const MjpegGeom g = mjpeg_geom(H, W);
    const int mb = mjpeg_chunk(chunk, g), cb = mb < B ? mb : B;
    const long long bound = mjpeg_bound(H, W);
    if (workspace_bytes)
        *workspace_bytes = (long long)cb * mjpeg_frame_ws(g) + 8 + (long long)cb * ((long long)H * W * 3 + bound + 4) + 8 + (long long)sizeof(MjpegTab);
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
        rc = mjpeg_batch(nullptr, (uint8_t*)(4 * gap), (const MjpegTab*)(5 * gap), (const uint8_t*)(6 * gap), nb, H, W, dst, sz + b0, tot, b0 == 0,
                         (long long)(b0 + nb) * bound);
    }
    g_plan = nullptr;
    if (rc) return rc;
    return og_plan_text(plan, kPlanWrites, out, cap);
}

}  // extern "C"
