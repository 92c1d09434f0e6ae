// Split entropy decode (include/split/openglottal_hip_mjps.h): a scan WITHOUT restart markers decoded by many lanes.  Included by
// og_api.hip after og_mjpd.inc, whose reader (og_jpegd_seek / og_jpegd_tell make it restartable), symbol decoder, MjpdTab and MjpdForm
// it reuses.  The data of a frame is cut into subsequences of `sub` bytes, a lane each; a lane owns the symbols whose first bit lies in
// its subsequence.  The header states the algorithm, its exactness and its bound; the inline functions below are what the kernel
// k_mjps_entropy and the host twin (og_jpegs_decode_host, the lanes walked in a loop) both call.
// With OG_MJPD_HOST_ONLY defined (after og_mjpd.inc in the same translation unit) only the twin is built: tools/mjps_host_fuzz.cpp.
#include "../../include/split/openglottal_hip_mjps.h"

constexpr int kMjpsLanes = 256;            // lanes of a window: the workgroup
constexpr int kMjpsWindow = 32768;         // bytes of a window at most: lanes = min(256, 32768 / sub)
constexpr int kMjpsSlack = 16;             // bytes staged behind a window: a lane's last symbol runs past its end (see og_jpegs_lane)
constexpr int kMjpsSubDefault = 128, kMjpsSubMin = 4, kMjpsSubMax = 1024;   // the default: measured, DESIGN section 24
constexpr int kMjpsNoError = 0x7FFFFFFF;

// the parse state between two symbols
struct OgJpegsState {
    int32_t pos;    // raw byte index in the scan of the data byte that holds the next bit (never a stuffed 00)
    int32_t info;   // bit (3 bits, 0 the highest) | block in the MCU << 3 (3) | zigzag index << 6 (6; 0: a DC symbol is next) | dead status << 12
};
OG_JPEG_HD bool og_jpegs_same(const OgJpegsState& a, const OgJpegsState& b) { return a.pos == b.pos && a.info == b.info; }
OG_JPEG_HD int og_jpegs_dead(const OgJpegsState& s) { return s.info >> 12; }

// what a lane found for its entry: the blocks it starts and the sum of their DC differences per component (modulo 2^32)
struct OgJpegsLane {
    int32_t nblk;
    uint32_t dc[3];
};

enum { kMjpsCount = 0, kMjpsWrite = 1, kMjpsErase = 2 };

OG_JPEG_HD int og_jpegs_bpm(const MjpdForm& g) { return g.ncomp == 1 ? 1 : g.hs[0] * g.vs[0] + 2; }
OG_JPEG_HD int og_jpegs_lanes(int sub) { return kMjpsWindow / sub < kMjpsLanes ? kMjpsWindow / sub : kMjpsLanes; }

// where block `cb` of the scan (stream order) lies among the frame's coefficients, and its component: og_jpegd_interval's address
OG_JPEG_HD long long og_jpegs_block(const MjpdForm& g, int bpm, int cb, int* comp) {
    const int m = cb / bpm, j = cb - m * bpm, nl = bpm - (g.ncomp == 1 ? 0 : 2);
    const int c = j < nl ? 0 : j - nl + 1;
    const int by = c ? 0 : j / g.hs[0], bx = c ? 0 : j - by * g.hs[0];
    const int myi = m / g.mx, mxi = m - myi * g.mx;
    // (selected, not indexed: a chroma component has one block per MCU)
    const int hs = c ? 1 : g.hs[0], vs = c ? 1 : g.vs[0];
    const int bw = c == 0 ? g.bw[0] : c == 1 ? g.bw[1] : g.bw[2], boff = c == 0 ? g.boff[0] : c == 1 ? g.boff[1] : g.boff[2];
    *comp = c;
    return ((long long)boff + (long long)(myi * vs + by) * bw + mxi * hs + bx) * 64;
}

// does the next bit lie in a data byte before `end`?  Every unconsumed bit lies before s.pos, so s.pos <= end answers without a walk.
OG_JPEG_HD bool og_jpegs_before(const OgJpegdBits& s, long long end) {
    if (s.nb > 0 && s.pos <= end) return true;
    long long q;
    int bit;
    og_jpegd_tell(s, &q, &bit);
    return q < end;
}

// the first 0xFF of bytes[0, n) that is no stuffed pair (the next byte is not 00, or lies at or past `len`, the scan's end seen from
// bytes[0]): og_jpegd_fill's rule.  A byte at n - 1 whose follower is not in bytes[0, n) and not past the scan is left to the next window.
OG_JPEG_HD bool og_jpegs_is_end(const uint8_t* bytes, long long n, long long len, long long i) {
    return bytes[i] == 0xFF && (i + 1 >= len || (i + 1 < n && bytes[i + 1] != 0));
}

// the speculative entry of a lane whose subsequence starts at bytes[q], q > 0: its first data byte, block 0, DC next
OG_JPEG_HD OgJpegsState og_jpegs_guess(const uint8_t* bytes, long long q, long long origin) {
    if (bytes[q] == 0 && bytes[q - 1] == 0xFF) q += 1;
    return OgJpegsState{(int32_t)(origin + q), 0};
}

// One lane, one pass.  bytes[0, n): the window's data (bytes[0] is raw byte `origin` of the scan, n ends at the data end or at the
// staged bytes); the lane decodes from `in` while the next symbol starts before bytes[end] and returns the state behind its last
// symbol.  An entry at or past `end`, or a dead one, passes through.
//   kMjpsCount  no block index is known: nothing is written, *res counts.  Missing bits (status 1: the data has ended) leave "dead".
//               An invalid code, a run that leaves the block or a category out of range (2, 3, 4) END THE BLOCK and the parse goes on
//               (an invalid code also drops one bit): a speculative parse in the wrong phase meets them all the time -- nine 1-bits
//               are no DC code -- and a dead exit that the next rounds have to take back travels as fast as the right states behind
//               it and so costs a round per lane (the header, ROUNDS).
//   kMjpsWrite  `base` blocks start before this lane and pred[] are the DC predictors at its entry: coefficients go where
//               og_jpegd_interval puts them, up to block `total`.  Strict: at the lane's first error, the DC range check included, it
//               stops and returns (4 * block + phase) * 8 + status, phase 0 a DC symbol, 1 the DC range, 2 an AC symbol: keys are
//               ordered as og_jpegd_interval meets the errors.  kMjpsNoError otherwise.
//   kMjpsErase  the same walk storing 0, without the range check (it may walk further than the write did: over coefficients that only
//               this lane's symbols address, which are 0 then).
// READS bytes[i] only for i < n.  With `end` + kMjpsSlack <= n or n at the data end: the reader holds at most 32 bits, a symbol with its
// value bits has at most 27, so behind a symbol that starts in bytes[end - 1] the reader has taken at most 6 data bytes, 12 raw ones.
OG_JPEG_HD OgJpegsState og_jpegs_lane(const uint8_t* bytes, long long n, long long origin, OgJpegsState in, long long end, const MjpdTab* t,
                                      const MjpdForm& g, int mode, int base, const uint32_t* pred_in, int total, int16_t* coefs, OgJpegsLane* res,
                                      int* err) {
    res->nblk = 0;
    res->dc[0] = res->dc[1] = res->dc[2] = 0;
    *err = kMjpsNoError;
    const long long q0 = (long long)in.pos - origin;
    if (og_jpegs_dead(in) || q0 >= end) return in;
    OgJpegdBits s;
    og_jpegd_seek(s, bytes, n, q0, in.info & 7);
    const int bpm = og_jpegs_bpm(g), nl = bpm - (g.ncomp == 1 ? 0 : 2);
    int blk = (in.info >> 3) & 7, k = (in.info >> 6) & 63;
    int cb = base - (k > 0 ? 1 : 0);   // the block the next symbol belongs to
    int c = blk < nl ? 0 : blk - nl + 1;
    uint32_t p0 = pred_in[0], p1 = pred_in[1], p2 = pred_in[2], d0 = 0, d1 = 0, d2 = 0;   // (scalars: no indexed private array)
    int16_t* dst = nullptr;
    int have = -1;
    for (;;) {
        if (mode != kMjpsCount) {
            if (cb >= total) break;
            if (have != cb) {
                dst = coefs + og_jpegs_block(g, bpm, cb, &c);
                have = cb;
            }
        }
        if (!og_jpegs_before(s, end)) break;
        int st = 0, phase = 2;
        if (k == 0) {
            phase = 0;
            const int sym = og_jpegd_symbol(s, t, t->dcsel[c] & 3);
            int diff = 0;
            if (sym < 0) st = -sym;
            else if (sym > 11) st = 4;
            else if (sym) diff = og_jpegd_receive(s, sym, &st);
            if (!st) {
                const uint32_t d = (uint32_t)diff;
                res->nblk += 1;
                d0 += c == 0 ? d : 0;
                d1 += c == 1 ? d : 0;
                d2 += c == 2 ? d : 0;
                if (mode == kMjpsWrite) {
                    const int v = (int)((c == 0 ? p0 + d0 : c == 1 ? p1 + d1 : p2 + d2));
                    if (v < -2048 || v > 2047) {
                        st = 4;
                        phase = 1;
                    } else {
                        dst[0] = (int16_t)v;
                    }
                } else if (mode == kMjpsErase) {
                    dst[0] = 0;
                }
                k = 1;
            }
        } else {
            const int sym = og_jpegd_symbol(s, t, t->acsel[c] & 3);
            if (sym < 0) {
                st = -sym;
            } else {
                const int run = sym >> 4, size = sym & 15;
                if (size == 0) {
                    if (run != 15) k = 64;            // EOB
                    else if (k + 15 > 63) st = 3;
                    else k += 16;                     // ZRL: sixteen zeros
                } else {
                    k += run;
                    if (k > 63) st = 3;
                    else if (size > 10) st = 4;
                    else {
                        const int v = og_jpegd_receive(s, size, &st);
                        if (!st) {
                            if (mode != kMjpsCount) dst[t->zz[k] & 63] = mode == kMjpsWrite ? (int16_t)v : (int16_t)0;
                            k += 1;
                        }
                    }
                }
            }
        }
        if (st) {
            if (mode != kMjpsCount) {
                *err = ((cb * 4 + phase) << 3) | st;
                break;
            }
            if (st == 1) {
                res->nblk = 0;   // (a dead lane's counts are never used)
                return OgJpegsState{0, st << 12};
            }
            if (st == 2) s.nb -= 1;        // (og_jpegd_symbol consumed nothing and holds 16 bits or more: one bit is dropped, so the walk advances)
            res->nblk += k == 0 ? 1 : 0;   // (a block whose DC failed still counts as started: starts never fall behind ends)
            k = 64;
        }
        if (k >= 64) {
            k = 0;
            blk = blk + 1 == bpm ? 0 : blk + 1;
            c = blk < nl ? 0 : blk - nl + 1;
            cb += 1;
        }
    }
    res->dc[0] = d0;
    res->dc[1] = d1;
    res->dc[2] = d2;
    long long q;
    int bit;
    og_jpegd_tell(s, &q, &bit);
    return OgJpegsState{(int32_t)(origin + q), bit | (blk << 3) | (k << 6)};
}

#ifndef OG_MJPD_HOST_ONLY
// ---- kernel ----------------------------------------------------------------------------------------------------------------------
struct MjpsShared {
    MjpdTab tab;
    uint32_t words[(kMjpsWindow + kMjpsSlack + 8) / 4];   // the window's bytes, from the dword that holds its first one
    OgJpegsState exits[2][kMjpsLanes];                    // the lanes' exits of the last two rounds
    uint32_t part[4][4];                                  // per wave: blocks and the three DC sums
    int end, err, errlane;
};

// A workgroup of 256 lanes per frame (the header: KERNEL).  Every loop is bounded: windows by the scan's length, rounds by the lanes
// of the window, a lane's walk by its subsequence.
__global__ __launch_bounds__(256) void k_mjps_entropy(const uint8_t* __restrict__ blob, const long long* __restrict__ offsets,
                                                      const og_mjpd_rec* __restrict__ recs, const MjpdTab* __restrict__ tabs, MjpdForm g, int sub,
                                                      const int* __restrict__ mstat, int16_t* __restrict__ coefs, int32_t* __restrict__ status) {
    __shared__ MjpsShared sh;
    const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (mstat[f] != 0) return;   // (k_mjpd_markers' verdict, the same for every lane)
    const og_mjpd_rec rec = recs[f];
    {
        const uint32_t* src = (const uint32_t*)(tabs + rec.tabset);
        uint32_t* dst = (uint32_t*)&sh.tab;
        for (int j = t; j < (int)(sizeof(MjpdTab) / 4); j += 256) dst[j] = src[j];
    }
    const uint8_t* scan = blob + offsets[f] + rec.scan_offset;
    const int len = rec.scan_length;
    int16_t* mine = coefs + (long long)f * g.blocks * 64;
    const int L = og_jpegs_lanes(sub), bpm = og_jpegs_bpm(g), total = g.M * bpm;
    OgJpegsState carry{0, 0};
    int base = 0;
    uint32_t pred0[3] = {0, 0, 0};
    for (int w0 = 0; w0 < len || w0 == 0; w0 += L * sub) {
        // stage bytes [w0, w0 + S): whole dwords with aligned loads, the two edge dwords byte by byte
        const int S = min(len - w0, L * sub + kMjpsSlack);
        const uint8_t* src = scan + w0;
        const int a = (int)((uintptr_t)src & 3);
        if (t == 0) {
            sh.end = S;
            sh.err = kMjpsNoError;
        }
        for (int j = t; j < (a + S + 3) / 4; j += 256) {
            const int lo = 4 * j - a;
            uint32_t v = 0;
            if (lo >= 0 && lo + 4 <= S) {
                v = *(const uint32_t*)(src + lo);
            } else {
                for (int b = 0; b < 4; ++b)
                    if (lo + b >= 0 && lo + b < S) v |= (uint32_t)src[lo + b] << (8 * b);
            }
            sh.words[j] = v;
        }
        __syncthreads();
        const uint8_t* bytes = (const uint8_t*)sh.words + a;
        // the data end, if these bytes hold it: the lowest hit
        int hit = S;
        for (int i0 = 4 * t - a; i0 < S && hit == S; i0 += 1024) {
            const uint32_t v = ~sh.words[(i0 + a) >> 2];
            if (((v - 0x01010101u) & ~v & 0x80808080u) == 0) continue;   // no 0xFF among the four
            for (int b = 0; b < 4 && hit == S; ++b)
                if (i0 + b >= 0 && i0 + b < S && og_jpegs_is_end(bytes, S, (long long)len - w0, i0 + b)) hit = i0 + b;
        }
        if (hit < S) atomicMin(&sh.end, hit);
        __syncthreads();
        const int n = sh.end;                                       // bytes the readers may take
        const bool last = n <= L * sub;                             // the data ends in this window: its last lane runs to the end
        const int nl = last ? max(1, (n + sub - 1) / sub) : L;
        const bool active = t < nl;
        const long long end = (last && t == nl - 1) ? (1ll << 40) : (long long)(t + 1) * sub;
        OgJpegsState entry = carry, exit{0, 0};
        if (active && t > 0) entry = og_jpegs_guess(bytes, (long long)t * sub, w0);
        OgJpegsLane res{0, {0, 0, 0}};
        int err, cur = 0;
        // ROUNDS: at most nl.  Lane 0 is right from round 0 on, lane r from round r on.
        for (int r = 0; r < nl; ++r) {
            bool changed = active && r == 0;
            if (active && r > 0 && t > 0) {
                const OgJpegsState in = sh.exits[cur][t - 1];
                changed = !og_jpegs_same(in, entry);
                entry = in;
            }
            if (changed) exit = og_jpegs_lane(bytes, n, w0, entry, end, &sh.tab, g, kMjpsCount, 0, pred0, 0, nullptr, &res, &err);
            cur = r & 1;
            if (active) sh.exits[cur][t] = exit;
            if (!__syncthreads_or(changed)) break;
        }
        // exclusive scans over the lanes: the first block of each and its predictors
        uint32_t v[4] = {(uint32_t)res.nblk, res.dc[0], res.dc[1], res.dc[2]}, own[4];
        for (int j = 0; j < 4; ++j) {
            if (!active) v[j] = 0;
            own[j] = v[j];
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(v[j], d, 64);
                if (lane >= d) v[j] += up;
            }
            if (lane == 63) sh.part[w][j] = v[j];
        }
        __syncthreads();
        uint32_t before[4], all[4];
        for (int j = 0; j < 4; ++j) {
            before[j] = v[j] - own[j];
            all[j] = 0;
            for (int ww = 0; ww < 4; ++ww) {
                if (ww < w) before[j] += sh.part[ww][j];
                all[j] += sh.part[ww][j];
            }
        }
        const uint32_t pred[3] = {pred0[0] + before[1], pred0[1] + before[2], pred0[2] + before[3]};
        const int first = base + (int)before[0];
        // the write pass; the lowest key is the frame's first error, and the lanes behind it take back what they wrote
        OgJpegsLane unused;
        if (active) og_jpegs_lane(bytes, n, w0, entry, end, &sh.tab, g, kMjpsWrite, first, pred, total, mine, &unused, &err);
        else err = kMjpsNoError;
        if (err != kMjpsNoError) atomicMin(&sh.err, err);
        __syncthreads();
        const int verdict = sh.err;
        if (verdict != kMjpsNoError) {
            if (err == verdict) sh.errlane = t;
            __syncthreads();
            if (active && t > sh.errlane) og_jpegs_lane(bytes, n, w0, entry, end, &sh.tab, g, kMjpsErase, first, pred, total, mine, &unused, &err);
            if (t == 0) atomicMax(&status[f], verdict & 7);
            return;
        }
        carry = sh.exits[cur][nl - 1];
        base += (int)all[0];
        for (int j = 0; j < 3; ++j) pred0[j] += all[j + 1];
        if (last || og_jpegs_dead(carry) || base - (((carry.info >> 6) & 63) ? 1 : 0) >= total) return;
        __syncthreads();   // the next window overwrites what this one still read
    }
}
#endif   // OG_MJPD_HOST_ONLY

// ---- host side -------------------------------------------------------------------------------------------------------------------
namespace {

#ifndef OG_MJPD_HOST_ONLY
int mjps_lds_bytes() { return (int)sizeof(MjpsShared); }
static_assert(sizeof(MjpsShared) <= 65536, "the header: LDS of k_mjps_entropy");
int mjps_sub_of(int mode, int sub, int Ri) { return mode == 1 && Ri == 0 ? (sub ? sub : kMjpsSubDefault) : 0; }
#endif

int check_mjps_sub(int sub) {
    if (sub != 0 && (sub < kMjpsSubMin || sub > kMjpsSubMax || sub % 4 != 0))
        return fail(OG_EINVAL, "sub must be 0 (the default) or a multiple of 4 in " + std::to_string(kMjpsSubMin) + ".." + std::to_string(kMjpsSubMax));
    return OG_OK;
}

// The twin of k_mjps_entropy on one scan: the same windows, rounds, scans and passes, the lanes walked in a loop.  `lanes` per window
// (the kernel's is og_jpegs_lanes(sub)).  stats: lanes, windows, the most rounds of a window, lane decodes of the rounds.
int mjps_scan_host(const uint8_t* scan, int len, const MjpdTab& tab, const MjpdForm& g, int sub, int lanes, int16_t* coefs, int32_t* stats) {
    const int L = std::min(lanes, og_jpegs_lanes(sub)), bpm = og_jpegs_bpm(g), total = g.M * bpm;
    OgJpegsState carry{0, 0};
    int base = 0;
    uint32_t pred0[3] = {0, 0, 0};
    std::vector<OgJpegsState> entry((size_t)L), exits[2] = {std::vector<OgJpegsState>((size_t)L), std::vector<OgJpegsState>((size_t)L)};
    std::vector<OgJpegsLane> res((size_t)L);
    std::vector<int> err((size_t)L), first((size_t)L);
    std::vector<uint32_t> pred((size_t)L * 3);
    for (int w0 = 0; w0 < len || w0 == 0; w0 += L * sub) {
        const int S = std::min(len - w0, L * sub + kMjpsSlack);
        const uint8_t* bytes = scan + w0;
        int n = S;
        for (int i = 0; i < S && n == S; ++i)
            if (og_jpegs_is_end(bytes, S, (long long)len - w0, i)) n = i;
        const bool last = n <= L * sub;
        const int nl = last ? std::max(1, (n + sub - 1) / sub) : L;
        auto end_of = [&](int i) { return (last && i == nl - 1) ? (1ll << 40) : (long long)(i + 1) * sub; };
        int cur = 0, rounds = 0, e;
        for (int r = 0; r < nl; ++r) {   // ROUNDS: at most nl
            bool any = false;
            const int prev = cur;
            cur = r & 1;
            for (int i = 0; i < nl; ++i) {
                bool changed = r == 0;
                if (r == 0) {
                    entry[i] = i ? og_jpegs_guess(bytes, (long long)i * sub, w0) : carry;
                } else if (i > 0) {
                    changed = !og_jpegs_same(exits[prev][i - 1], entry[i]);
                    entry[i] = exits[prev][i - 1];
                }
                if (changed) {
                    exits[cur][i] = og_jpegs_lane(bytes, n, w0, entry[i], end_of(i), &tab, g, kMjpsCount, 0, pred0, 0, nullptr, &res[i], &e);
                    stats[3] += 1;
                } else {
                    exits[cur][i] = exits[prev][i];
                }
                any |= changed;
            }
            rounds = r + 1;
            if (!any) break;
        }
        stats[0] += nl;
        stats[1] += 1;
        stats[2] = std::max(stats[2], rounds);
        uint32_t run[4] = {(uint32_t)base, pred0[0], pred0[1], pred0[2]};
        for (int i = 0; i < nl; ++i) {
            first[i] = (int)run[0];
            for (int j = 0; j < 3; ++j) pred[3 * i + j] = run[j + 1];
            run[0] += (uint32_t)res[i].nblk;
            for (int j = 0; j < 3; ++j) run[j + 1] += res[i].dc[j];
        }
        OgJpegsLane unused;
        int verdict = kMjpsNoError, errlane = -1;
        for (int i = 0; i < nl; ++i) {
            og_jpegs_lane(bytes, n, w0, entry[i], end_of(i), &tab, g, kMjpsWrite, first[i], &pred[3 * i], total, coefs, &unused, &err[i]);
            if (err[i] < verdict) {
                verdict = err[i];
                errlane = i;
            }
        }
        if (verdict != kMjpsNoError) {
            for (int i = errlane + 1; i < nl; ++i)
                og_jpegs_lane(bytes, n, w0, entry[i], end_of(i), &tab, g, kMjpsErase, first[i], &pred[3 * i], total, coefs, &unused, &e);
            return verdict & 7;
        }
        carry = exits[cur][nl - 1];
        base = (int)run[0];
        for (int j = 0; j < 3; ++j) pred0[j] = run[j + 1];
        if (last || og_jpegs_dead(carry) || base - (((carry.info >> 6) & 63) ? 1 : 0) >= total) break;
    }
    return 0;
}

// mjpd_frame_host with the split pass in place of og_jpegd_interval; a file with restart markers takes mjpd_frame_host itself
int mjps_frame_host(const uint8_t* jpeg, const og_jpegd_info& info, const MjpdTab& tab, int sub, int lanes, uint8_t* out, int32_t* stats) {
    if (info.Ri != 0) return mjpd_frame_host(jpeg, info, tab, out);
    MjpdForm g;
    mjpd_form(info.H, info.W, info.sampling, &g);
    std::vector<int16_t> coefs((size_t)g.blocks * 64, 0);
    int ivl[2];
    const uint8_t* scan = jpeg + info.scan_offset;
    int st = mjpd_markers_host(scan, (int)info.scan_length, 1, ivl);
    if (!st) st = mjps_scan_host(scan, (int)info.scan_length, tab, g, sub, lanes, coefs.data(), stats);
    mjpd_pixels_host(coefs.data(), tab, g, out);
    return st;
}

}  // namespace

extern "C" {

long long og_mjps_limit(int which) {
    switch (which) {
        case 0: return kMjpsSubDefault;
        case 1: return kMjpsSubMin;
        case 2: return kMjpsSubMax;
        case 3: return kMjpsLanes;
        case 4: return kMjpsWindow;
#ifndef OG_MJPD_HOST_ONLY
        case 5: return (long long)sizeof(MjpsShared);
#endif
        default: return -1;
    }
}

int og_jpegs_decode_host(const uint8_t* jpeg, size_t size, int sub, int lanes, uint8_t* out_bgr, size_t cap, int* status, int32_t* stats) {
    if (!jpeg || !out_bgr || !status) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(status);
    OG_ALIGN(stats);
    int rc = check_mjps_sub(sub);
    if (rc) return rc;
    if (lanes < 1 || lanes > kMjpsLanes) return fail(OG_EINVAL, "lanes must be 1.." + std::to_string(kMjpsLanes));
    int32_t local[4] = {0, 0, 0, 0};
    MjpdParsed p;
    if (mjpd_parse(jpeg, size, &p)) {
        *status = 6;
        if (stats) memcpy(stats, local, sizeof local);
        return OG_OK;
    }
    const unsigned long long need = (unsigned long long)p.info.H * p.info.W * 3;
    if ((unsigned long long)cap < need) return fail(OG_EINVAL, "cap is below H * W * 3 = " + std::to_string(need) + " bytes");
    MjpdTab tab;
    mjpd_build_tab(p.spec, &tab);
    *status = mjps_frame_host(jpeg, p.info, tab, sub ? sub : kMjpsSubDefault, lanes, out_bgr, local);
    if (stats) memcpy(stats, local, sizeof local);
    return OG_OK;
}

#ifndef OG_MJPD_HOST_ONLY
int og_mjps_set_split(og_mjpd* h, int mode, int sub) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (mode != 0 && mode != 1) return fail(OG_EINVAL, "mode must be 0 (off) or 1 (split scans without restart markers)");
    const int rc = check_mjps_sub(sub);
    if (rc) return rc;
    h->split = mode;
    h->sub = sub;
    return OG_OK;
}

int og_mjps_plan(int B, int H, int W, int sampling, int Ri, int chunk, int mode, int sub, char* out, size_t cap, long long* workspace_bytes) {
    if (mode != 0 && mode != 1) return fail(OG_EINVAL, "mode must be 0 (off) or 1 (split scans without restart markers)");
    const int rc = check_mjps_sub(sub);
    if (rc) return rc;
    return mjpd_plan_text(B, H, W, sampling, Ri, chunk, mjps_sub_of(mode, sub, Ri), out, cap, workspace_bytes);
}
#endif   // OG_MJPD_HOST_ONLY

}  // extern "C"
