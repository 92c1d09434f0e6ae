// Detector ablation sweeps from one inference pass (include/openglottal_hip_sweep.h, DESIGN.md section 20): the confusion counts of
// every (confidence threshold, hold duration) configuration of the temporal detector from masks, ground truth and `best` rows that
// are already on the device, reading the masks once.  Included by og_api.hip, as og_overlay.inc is.  Kernels and entries live here;
// everything is plain C++ (the hazard audits of tests/test_isa_*.py run over these kernels as over every other of the build).
//
// Per micro-batch of nb frames, on the handle's one stream:
//   k_sweep_sat_rows   a wave per row: 64-lane inclusive scan of {P, T} over 64-pixel segments plus a carry -> row prefix sums into the
//                      table's rows 1..H, columns 1..W; zeroes row 0 and column 0; adds the row's totals to frame_counts
//   k_sweep_sat_cols   a lane per table column, rows in order: the running column sum makes the row prefixes a summed-area table
//   k_sweep_track      a lane per frame measures into LDS, then a lane per CONFIGURATION walks the frames through og_track_advance
//   k_sweep_lookup     a lane per (configuration, frame): four corners of the table -> {tp, n_pred, detected}
// pred and gt are read once each (by k_sweep_sat_rows).  Every entry of the table -- the zero border included -- is rewritten by
// every micro-batch, so nothing but the tracker states goes from call to call, whatever shapes the handle has seen.
#include "../../include/openglottal_hip_sweep.h"

// the detection gate of one configuration: the detector's "conf > conf_thres" (inclusive = 0) or sweep_bagls_conf.py:207's ">="
// (inclusive = 1), the f32 confidence compared AS A DOUBLE with the f64 threshold; conf < 0 (and NaN) is "no detection"
__host__ __device__ inline bool og_sweep_gate(float conf, double thr, int inclusive) {
    if (!(conf >= 0.0f)) return false;
    return inclusive ? (double)conf >= thr : (double)conf > thr;
}

// the table of frame f: (H+1) x (W+1) pairs {P, T}; entry (y, x) counts the pixels of rows < y and columns < x
__host__ __device__ inline long long og_sweep_table_elems(int H, int W) { return (long long)(H + 1) * (W + 1); }

constexpr int kSweepWavesPerBlock = 4;

// grid (ceil(H / 4), nb), 256 lanes: wave w of block bx owns row y = 4 * bx + w of frame blockIdx.y.  No barrier, so a wave past
// the last row simply leaves.  A lane's segment value packs P in bits 0..15 and T in bits 16..31: a 64-pixel segment counts at most
// 64 of each, so ONE scan serves both.  frame_counts has been zeroed by the caller on the same stream.
__global__ __launch_bounds__(256) void k_sweep_sat_rows(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, int H, int W,
                                                        uint2* __restrict__ tab, int32_t* __restrict__ frame_counts) {
    const int f = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int y = blockIdx.x * kSweepWavesPerBlock + (threadIdx.x >> 6);
    if (y >= H) return;
    const long long TW = W + 1;
    const uint8_t* pr = pred + ((long long)f * H + y) * W;
    const uint8_t* gr = gt + ((long long)f * H + y) * W;
    uint2* frame_tab = tab + (long long)f * og_sweep_table_elems(H, W);
    uint2* out = frame_tab + (long long)(y + 1) * TW;
    if (y == 0)
        for (int x = lane; x <= W; x += 64) frame_tab[x] = make_uint2(0u, 0u);   // row 0
    if (lane == 0) out[0] = make_uint2(0u, 0u);                                  // column 0
    unsigned cp = 0, ct = 0;
    int ng = 0;
    for (int x0 = 0; x0 < W; x0 += 64) {   // (the trip count is the same for every lane: the shuffles see the whole wave)
        const int x = x0 + lane;
        const bool in = x < W;
        const bool p = in && pr[x] > 0;
        const bool g = in && gr[x] > 0;
        int s = (p ? 1 : 0) | ((p && g) ? (1 << 16) : 0);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(s, o);
            if (lane >= o) s += v;
        }
        if (in) out[x + 1] = make_uint2(cp + (unsigned)(s & 0xffff), ct + (unsigned)(s >> 16));
        const int tot = __shfl(s, 63);
        cp += (unsigned)(tot & 0xffff);
        ct += (unsigned)(tot >> 16);
        ng += (int)__popcll(__ballot(g));
    }
    if (lane == 0) {
        if (ct) atomicAdd(&frame_counts[f * 3 + 0], (int)ct);
        if (cp) atomicAdd(&frame_counts[f * 3 + 1], (int)cp);
        if (ng) atomicAdd(&frame_counts[f * 3 + 2], ng);
    }
}

// grid (ceil((W + 1) / 256), nb): a lane per table column x in 0..W walks rows 1..H and leaves the running sum; neighbouring lanes
// touch neighbouring pairs, so every access of a wave is one run of 512 bytes.  Eight rows are requested before the first is
// used.  Column 0 is zero and stays zero.
__global__ __launch_bounds__(256) void k_sweep_sat_cols(int H, int W, uint2* __restrict__ tab) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x > W) return;
    const long long TW = W + 1;
    uint2* col = tab + (long long)blockIdx.y * og_sweep_table_elems(H, W) + x;
    unsigned ap = 0, at = 0;
    int r = 1;
    for (; r + 7 <= H; r += 8) {
        uint2 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = col[(long long)(r + k) * TW];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            ap += v[k].x;
            at += v[k].y;
            col[(long long)(r + k) * TW] = make_uint2(ap, at);
        }
    }
    for (; r <= H; ++r) {
        const uint2 v = col[(long long)r * TW];
        ap += v.x;
        at += v.y;
        col[(long long)r * TW] = make_uint2(ap, at);
    }
}

// grid ceil(C / 256), 256 lanes; mirrors k_track_boxes.  Per block of 256 frames a lane per frame measures its `best` row into LDS
// (the measurement does not depend on the configuration; every workgroup repeats it), and after the barrier lane c walks the block
// in frame order through og_track_advance with ITS threshold and hold: the state stays in registers, every lane reads the same LDS
// word at the same time (a broadcast).  Boxes go to the workspace as [C, nb, 4].  The sequential length is nb <= the chunk.
__global__ __launch_bounds__(256) void k_sweep_track(const float* __restrict__ best, const uint8_t* __restrict__ resets, int nb, int W, int H,
                                                     float max_shift, int padding, int inclusive, const double* __restrict__ thr,
                                                     const int32_t* __restrict__ hold, int n_hold, int C, OgTrackState* __restrict__ state,
                                                     int32_t* __restrict__ boxes) {
    __shared__ float s_cx[256], s_cy[256], s_conf[256];
    __shared__ int s_w[256], s_h[256], s_reset[256];
    const int tid = threadIdx.x;
    const int c = blockIdx.x * 256 + tid;
    const bool live = c < C;
    OgTrackState s{0.f, 0.f, 0, 0, 0, 0};
    OgTrackParams p{max_shift, padding, 0};
    double t = 0.0;
    if (live) {
        s = state[c];
        t = thr[c / n_hold];
        p.max_hold = hold[c % n_hold];
    }
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int n = nb - b0 < 256 ? nb - b0 : 256;
        if (tid < n) {
            float row[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) row[k] = best[(long long)(b0 + tid) * 5 + k];
            float cx, cy;
            int w, h;
            (void)og_track_measure(row, padding, cx, cy, w, h);
            s_cx[tid] = cx;
            s_cy[tid] = cy;
            s_w[tid] = w;
            s_h[tid] = h;
            s_conf[tid] = row[4];
            s_reset[tid] = (resets != nullptr && resets[b0 + tid] != 0) ? 1 : 0;
        }
        __syncthreads();
        if (live) {
            for (int i = 0; i < n; ++i) {
                if (s_reset[i]) s = OgTrackState{0.f, 0.f, 0, 0, 0, 0};
                int box[4];
                og_track_advance(s, og_sweep_gate(s_conf[i], t, inclusive), s_cx[i], s_cy[i], s_w[i], s_h[i], W, H, p, box);
                int32_t* o = boxes + ((long long)c * nb + b0 + i) * 4;
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = box[k];
            }
        }
        __syncthreads();   // (the next block's measurements overwrite what the walk has just read)
    }
    if (live) state[c] = s;
}

// grid ceil(C * nb / 256): a lane per (configuration, frame of the micro-batch).  It indexes the table ONLY with the box k_sweep_track
// stored, which is og_track_advance's NORMALISED box: og_slice_end clamps every coordinate to 0..W / 0..H, and the table has
// (H+1) x (W+1) entries, so no `best` row, however malformed, can make this kernel read outside the table; x1 < 0 is "no box".
// Results go to the caller's arrays of N frames at frame b0 + f.
__global__ __launch_bounds__(256) void k_sweep_lookup(const uint2* __restrict__ tab, const int32_t* __restrict__ boxes_ws, int nb, int H, int W,
                                                      int C, long long N, long long b0, int32_t* __restrict__ counts,
                                                      int32_t* __restrict__ boxes_out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)C * nb) return;
    const long long c = idx / nb;
    const int f = (int)(idx - c * nb);
    const int x1 = boxes_ws[idx * 4 + 0], y1 = boxes_ws[idx * 4 + 1], x2 = boxes_ws[idx * 4 + 2], y2 = boxes_ws[idx * 4 + 3];
    unsigned tp = 0, np_ = 0;
    if (x1 >= 0) {
        const long long TW = W + 1;
        const uint2* t = tab + (long long)f * og_sweep_table_elems(H, W);
        const uint2 a = t[y2 * TW + x2], b = t[y1 * TW + x2], d = t[y2 * TW + x1], e = t[y1 * TW + x1];
        np_ = a.x - b.x - d.x + e.x;
        tp = a.y - b.y - d.y + e.y;
    }
    const long long o = c * N + b0 + f;
    counts[o * 3 + 0] = (int32_t)tp;
    counts[o * 3 + 1] = (int32_t)np_;
    counts[o * 3 + 2] = x1 >= 0 ? 1 : 0;
    if (boxes_out != nullptr) {
        boxes_out[o * 4 + 0] = x1;
        boxes_out[o * 4 + 1] = y1;
        boxes_out[o * 4 + 2] = x2;
        boxes_out[o * 4 + 3] = y2;
    }
}

struct og_sweep : OgStreamHandle {   // ready: the stream, the states and the grid's device rows exist
    og_sweep() { chunk = 0; }   // 0: the default for the shape
    std::vector<double> thr;      // the grid of the last call; a call with another one resets the states
    std::vector<int32_t> hold;
    double* d_thr = nullptr;
    int32_t* d_hold = nullptr;
    OgTrackState* d_state = nullptr;
    // each buffer holds the bytes of the largest micro-batch run so far
    OgBuf<uint2> d_tab;
    OgBuf<int32_t> d_box;
    OgBuf<uint8_t> d_stage;
};

namespace {

constexpr long long kSweepMaxPixels = 4194304;
constexpr int kSweepMaxConf = 32, kSweepMaxHold = 32, kSweepMaxChunk = 4096;
constexpr long long kSweepTableBytes = 256ll << 20;   // of tables per micro-batch at the default chunk

int sweep_default_chunk(int H, int W) {
    const long long fit = kSweepTableBytes / (8 * og_sweep_table_elems(H, W));
    return (int)(fit < 1 ? 1 : (fit > kSweepMaxChunk ? kSweepMaxChunk : fit));
}
// the header's MEMORY formula, per frame of a micro-batch
long long sweep_frame_bytes(int H, int W, int C) { return 8 * og_sweep_table_elems(H, W) + 16ll * C; }

// everything that can be said without a handle or a device, in the order the header lists the arguments
int check_sweep(int N, int H, int W, const double* conf_thres, int n_conf, const int32_t* max_hold, int n_hold, float max_shift, int padding,
                int inclusive) {
    if (N < 0 || H <= 0 || W <= 0) return fail(OG_EINVAL, "bad N/H/W");
    if ((long long)H * W > kSweepMaxPixels) return fail(OG_EINVAL, "H*W above " + std::to_string(kSweepMaxPixels) + " pixels");
    if (n_conf < 1 || n_conf > kSweepMaxConf) return fail(OG_EINVAL, "n_conf must be 1.." + std::to_string(kSweepMaxConf));
    if (n_hold < 1 || n_hold > kSweepMaxHold) return fail(OG_EINVAL, "n_hold must be 1.." + std::to_string(kSweepMaxHold));
    if (inclusive != 0 && inclusive != 1) return fail(OG_EINVAL, "inclusive must be 0 or 1");
    if (!conf_thres || !max_hold) return fail(OG_EINVAL, "conf_thres / max_hold is null");
    OG_ALIGN(conf_thres);
    OG_ALIGN(max_hold);
    const og_track_params p{max_shift, padding, 0};
    int rc = check_track_params(&p);
    if (rc) return rc;
    for (int i = 0; i < n_hold; ++i)
        if (max_hold[i] < 0) return fail(OG_EINVAL, "max_hold[" + std::to_string(i) + "] must be >= 0");
    return OG_OK;
}

int sweep_ready(og_sweep* h) {
    if (h->ready) return OG_OK;
    const int rc = og_stream_ready(h);
    if (rc) return rc;
    hipError_t e = hipMalloc((void**)&h->d_thr, kSweepMaxConf * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_hold, kSweepMaxHold * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_state, (size_t)kSweepMaxConf * kSweepMaxHold * sizeof(OgTrackState));
    // (on the handle's stream: a non-blocking stream is not ordered after the null stream's work)
    if (e == hipSuccess) e = hipMemsetAsync(h->d_state, 0, (size_t)kSweepMaxConf * kSweepMaxHold * sizeof(OgTrackState), h->stream);
    if (e != hipSuccess) {
        if (h->d_thr) (void)hipFree(h->d_thr);
        if (h->d_hold) (void)hipFree(h->d_hold);
        if (h->d_state) (void)hipFree(h->d_state);
        (void)hipStreamDestroy(h->stream);
        h->d_thr = nullptr;
        h->d_hold = nullptr;
        h->d_state = nullptr;
        h->stream = nullptr;
        h->ready = false;
        return fail(e == hipErrorOutOfMemory ? OG_ENOMEM : OG_EHIP, std::string("og_sweep: ") + hipGetErrorString(e));
    }
    return OG_OK;
}

// the grid of this call on the device; another grid than the last call's clears every state
int sweep_set_grid(og_sweep* h, const double* conf_thres, int n_conf, const int32_t* max_hold, int n_hold) {
    const bool same = (int)h->thr.size() == n_conf && (int)h->hold.size() == n_hold &&
                      memcmp(h->thr.data(), conf_thres, (size_t)n_conf * sizeof(double)) == 0 &&
                      memcmp(h->hold.data(), max_hold, (size_t)n_hold * sizeof(int32_t)) == 0;
    if (same) return OG_OK;
    HIPCHK(hipStreamSynchronize(h->stream));   // launches in flight read the old rows
    h->thr.clear();
    h->hold.clear();
    HIPCHK(hipMemcpyAsync(h->d_thr, conf_thres, (size_t)n_conf * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_hold, max_hold, (size_t)n_hold * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->d_state, 0, (size_t)kSweepMaxConf * kSweepMaxHold * sizeof(OgTrackState), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));   // the caller's arrays have been read when the call returns
    h->thr.assign(conf_thres, conf_thres + n_conf);
    h->hold.assign(max_hold, max_hold + n_hold);
    return OG_OK;
}

// one micro-batch of nb resident frames; the results land at frame b0 of the caller's arrays of N frames
int sweep_batch(og_sweep* h, const uint8_t* pred, const uint8_t* gt, const float* best, const uint8_t* resets, int nb, int H, int W, int n_hold,
                int C, float max_shift, int padding, int inclusive, long long N, long long b0, int32_t* frame_counts, int32_t* counts,
                int32_t* boxes) {
    const hipStream_t st = h->stream;
    HIPCHK(hipMemsetAsync(frame_counts + 3 * b0, 0, (size_t)nb * 12, st));
    OG_LAUNCH(k_sweep_sat_rows, dim3((unsigned)((H + kSweepWavesPerBlock - 1) / kSweepWavesPerBlock), (unsigned)nb), dim3(256), 0, st, pred, gt, H,
              W, h->d_tab, frame_counts + 3 * b0);
    OG_LAUNCH(k_sweep_sat_cols, dim3((unsigned)((W + 1 + 255) / 256), (unsigned)nb), dim3(256), 0, st, H, W, h->d_tab);
    OG_LAUNCH(k_sweep_track, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, best, resets, nb, W, H, max_shift, padding, inclusive,
              (const double*)h->d_thr, (const int32_t*)h->d_hold, n_hold, C, h->d_state, h->d_box);
    OG_LAUNCH(k_sweep_lookup, dim3((unsigned)(((long long)C * nb + 255) / 256)), dim3(256), 0, st, (const uint2*)h->d_tab,
              (const int32_t*)h->d_box, nb, H, W, C, N, b0, counts, boxes);
    return OG_OK;
}

// device set-up shared by the two entries: the stream, the grid, the workspace of one micro-batch of cb frames
int sweep_prepare(og_sweep* h, int cb, int H, int W, const double* conf_thres, int n_conf, const int32_t* max_hold, int n_hold) {
    int rc = sweep_set_grid(h, conf_thres, n_conf, max_hold, n_hold);
    if (rc) return rc;
    const int C = n_conf * n_hold;
    if ((rc = h->d_tab.grow(h, (size_t)cb * 8 * (size_t)og_sweep_table_elems(H, W), "sweep"))) return rc;
    return h->d_box.grow(h, (size_t)cb * 16 * C, "sweep");
}

inline size_t sweep_up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

long long og_sweep_limit(int which) {
    return which == 0 ? kSweepMaxPixels : which == 1 ? kSweepMaxConf : which == 2 ? kSweepMaxHold : which == 3 ? kSweepMaxChunk : -1;
}

int og_sweep_host(const uint8_t* pred, const uint8_t* gt, const float* best, const uint8_t* resets_or_null, int N, int H, int W,
                  const double* conf_thres, int n_conf, const int32_t* max_hold, int n_hold, float max_shift_px, int padding, int inclusive,
                  og_track_state* states_inout_or_null, int32_t* frame_counts, int32_t* counts, int32_t* boxes_or_null) {
    int rc = check_sweep(N, H, W, conf_thres, n_conf, max_hold, n_hold, max_shift_px, padding, inclusive);
    if (rc) return rc;
    OG_ALIGN(best);
    OG_ALIGN(states_inout_or_null);
    OG_ALIGN(frame_counts);
    OG_ALIGN(counts);
    OG_ALIGN(boxes_or_null);
    if (N == 0) return OG_OK;
    if (!pred || !gt || !best || !frame_counts || !counts) return fail(OG_EINVAL, "null buffer");
    const size_t HW = (size_t)H * W;
    for (int i = 0; i < N; ++i) {
        int tp = 0, np_ = 0, ng = 0;
        const uint8_t *p = pred + i * HW, *g = gt + i * HW;
        for (size_t q = 0; q < HW; ++q) {
            tp += (p[q] > 0 && g[q] > 0) ? 1 : 0;
            np_ += p[q] > 0 ? 1 : 0;
            ng += g[q] > 0 ? 1 : 0;
        }
        frame_counts[3 * (size_t)i + 0] = tp;
        frame_counts[3 * (size_t)i + 1] = np_;
        frame_counts[3 * (size_t)i + 2] = ng;
    }
    for (int it = 0; it < n_conf; ++it)
        for (int ih = 0; ih < n_hold; ++ih) {
            const size_t c = (size_t)it * n_hold + ih;
            OgTrackState s{0.f, 0.f, 0, 0, 0, 0};
            if (states_inout_or_null) memcpy(&s, states_inout_or_null + c, sizeof s);
            const OgTrackParams prm{max_shift_px, padding, max_hold[ih]};
            for (int i = 0; i < N; ++i) {
                if (resets_or_null && resets_or_null[i]) s = OgTrackState{0.f, 0.f, 0, 0, 0, 0};
                float row[5];
                memcpy(row, best + 5 * (size_t)i, sizeof row);
                if (!og_sweep_gate(row[4], conf_thres[it], inclusive)) row[4] = -1.0f;   // the gate is applied to the row
                int box[4];
                og_track_step(s, row, W, H, prm, box);
                int tp = 0, np_ = 0;
                if (box[0] >= 0) {
                    const uint8_t *p = pred + i * HW, *g = gt + i * HW;
                    for (int y = box[1]; y < box[3]; ++y)
                        for (int x = box[0]; x < box[2]; ++x) {
                            const size_t q = (size_t)y * W + x;
                            np_ += p[q] > 0 ? 1 : 0;
                            tp += (p[q] > 0 && g[q] > 0) ? 1 : 0;
                        }
                }
                const size_t o = c * N + i;
                counts[o * 3 + 0] = tp;
                counts[o * 3 + 1] = np_;
                counts[o * 3 + 2] = box[0] >= 0 ? 1 : 0;
                if (boxes_or_null)
                    for (int k = 0; k < 4; ++k) boxes_or_null[o * 4 + k] = box[k];
            }
            if (states_inout_or_null) memcpy(states_inout_or_null + c, &s, sizeof s);
        }
    return OG_OK;
}

og_sweep* og_sweep_create(void) { return new og_sweep(); }

void og_sweep_destroy(og_sweep* h) {
    og_stream_destroy(h, [h] {
        (void)hipFree(h->d_thr);   // (the three of sweep_ready exist together)
        (void)hipFree(h->d_hold);
        (void)hipFree(h->d_state);
        og_release(h->d_tab, h->d_box, h->d_stage);
    });
}

int og_sweep_sync(og_sweep* h) { return og_stream_sync(h); }

int og_sweep_set_chunk(og_sweep* h, int chunk) { return og_stream_set_chunk(h, chunk, kSweepMaxChunk, true); }

int og_sweep_reset(og_sweep* h) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (!h->ready) return OG_OK;   // no state has been made yet: every configuration starts without a centre
    OG_SCOPE(h);
    HIPCHK(hipMemsetAsync(h->d_state, 0, (size_t)kSweepMaxConf * kSweepMaxHold * sizeof(OgTrackState), h->stream));
    return OG_OK;
}

int og_sweep_get_state(og_sweep* h, int c, og_track_state* state) {
    if (!h || !state) return fail(OG_EINVAL, "null argument");
    OG_ALIGN(state);
    if (c < 0 || (size_t)c >= h->thr.size() * h->hold.size()) return fail(OG_EINVAL, "c is not a configuration of the last call's grid");
    OG_SCOPE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(state, h->d_state + c, sizeof(OgTrackState), hipMemcpyDeviceToHost));
    return OG_OK;
}

int og_sweep_counts_u8_dev(og_sweep* h, const uint8_t* pred_dev, const uint8_t* gt_dev, const float* best_dev,
                           const uint8_t* resets_dev_or_null, int N, int H, int W, const double* conf_thres, int n_conf,
                           const int32_t* max_hold, int n_hold, float max_shift_px, int padding, int inclusive, int32_t* frame_counts_dev,
                           int32_t* counts_dev, int32_t* boxes_dev_or_null) {
    if (!h) return fail(OG_EINVAL, "null handle");
    int rc = check_sweep(N, H, W, conf_thres, n_conf, max_hold, n_hold, max_shift_px, padding, inclusive);
    if (rc) return rc;
    OG_ALIGN(best_dev);
    OG_ALIGN(frame_counts_dev);
    OG_ALIGN(counts_dev);
    OG_ALIGN(boxes_dev_or_null);
    if (N == 0) return OG_OK;
    if (!pred_dev || !gt_dev || !best_dev || !frame_counts_dev || !counts_dev) return fail(OG_EINVAL, "null buffer");
    if ((rc = sweep_ready(h))) return rc;
    OG_SCOPE(h);
    const int C = n_conf * n_hold;
    const int chunk = h->chunk ? h->chunk : sweep_default_chunk(H, W), cb = chunk < N ? chunk : N;
    if ((rc = sweep_prepare(h, cb, H, W, conf_thres, n_conf, max_hold, n_hold))) return rc;
    const size_t HW = (size_t)H * W;
    for (int b0 = 0; b0 < N && !rc; b0 += chunk) {
        const int nb = (N - b0 < chunk) ? N - b0 : chunk;
        rc = sweep_batch(h, pred_dev + b0 * HW, gt_dev + b0 * HW, best_dev + 5 * (size_t)b0, resets_dev_or_null ? resets_dev_or_null + b0 : nullptr,
                         nb, H, W, n_hold, C, max_shift_px, padding, inclusive, N, b0, frame_counts_dev, counts_dev, boxes_dev_or_null);
    }
    if (rc) og_stream_drain(h);
    return rc;
}

int og_sweep_counts_u8(og_sweep* h, const uint8_t* pred, const uint8_t* gt, const float* best, const uint8_t* resets_or_null, int N, int H,
                       int W, const double* conf_thres, int n_conf, const int32_t* max_hold, int n_hold, float max_shift_px, int padding,
                       int inclusive, int32_t* frame_counts, int32_t* counts, int32_t* boxes_or_null) {
    if (!h) return fail(OG_EINVAL, "null handle");
    int rc = check_sweep(N, H, W, conf_thres, n_conf, max_hold, n_hold, max_shift_px, padding, inclusive);
    if (rc) return rc;
    OG_ALIGN(best);
    OG_ALIGN(frame_counts);
    OG_ALIGN(counts);
    OG_ALIGN(boxes_or_null);
    if (N == 0) return OG_OK;
    if (!pred || !gt || !best || !frame_counts || !counts) return fail(OG_EINVAL, "null buffer");
    if ((rc = sweep_ready(h))) return rc;
    OG_SCOPE(h);
    const int C = n_conf * n_hold;
    const int chunk = h->chunk ? h->chunk : sweep_default_chunk(H, W), cb = chunk < N ? chunk : N;
    if ((rc = sweep_prepare(h, cb, H, W, conf_thres, n_conf, max_hold, n_hold))) return rc;
    const size_t HW = (size_t)H * W;
    // one staging buffer of a micro-batch: pred | gt | best | resets | frame_counts | counts [C,cb,3] | boxes [C,cb,4]
    const size_t o_pred = 0, o_gt = sweep_up256(o_pred + cb * HW), o_best = sweep_up256(o_gt + cb * HW),
                 o_res = sweep_up256(o_best + (size_t)cb * 20), o_fc = sweep_up256(o_res + (size_t)cb),
                 o_cnt = sweep_up256(o_fc + (size_t)cb * 12), o_box = sweep_up256(o_cnt + (size_t)C * cb * 12),
                 total = o_box + (size_t)C * cb * 16;
    if ((rc = h->d_stage.grow(h, total, "sweep"))) return rc;
    uint8_t* s = h->d_stage;
    const hipStream_t st = h->stream;
    std::vector<int32_t> h_cnt((size_t)C * cb * 3), h_box(boxes_or_null ? (size_t)C * cb * 4 : 0);
    auto run = [&](int b0, int nb) -> int {
        HIPCHK(hipMemcpyAsync(s + o_pred, pred + b0 * HW, nb * HW, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(s + o_gt, gt + b0 * HW, nb * HW, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(s + o_best, best + 5 * (size_t)b0, (size_t)nb * 20, hipMemcpyHostToDevice, st));
        if (resets_or_null) HIPCHK(hipMemcpyAsync(s + o_res, resets_or_null + b0, (size_t)nb, hipMemcpyHostToDevice, st));
        // the staged outputs are arrays of nb frames: stride nb, first frame 0
        const int rc2 = sweep_batch(h, s + o_pred, s + o_gt, (const float*)(s + o_best), resets_or_null ? s + o_res : nullptr, nb, H, W, n_hold, C,
                                    max_shift_px, padding, inclusive, nb, 0, (int32_t*)(s + o_fc), (int32_t*)(s + o_cnt),
                                    boxes_or_null ? (int32_t*)(s + o_box) : nullptr);
        if (rc2) return rc2;
        HIPCHK(hipMemcpyAsync(frame_counts + 3 * (size_t)b0, s + o_fc, (size_t)nb * 12, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_cnt.data(), s + o_cnt, (size_t)C * nb * 12, hipMemcpyDeviceToHost, st));
        if (boxes_or_null) HIPCHK(hipMemcpyAsync(h_box.data(), s + o_box, (size_t)C * nb * 16, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int c = 0; c < C; ++c) {
            memcpy(counts + ((size_t)c * N + b0) * 3, h_cnt.data() + (size_t)c * nb * 3, (size_t)nb * 12);
            if (boxes_or_null) memcpy(boxes_or_null + ((size_t)c * N + b0) * 4, h_box.data() + (size_t)c * nb * 4, (size_t)nb * 16);
        }
        return OG_OK;
    };
    for (int b0 = 0; b0 < N && !rc; b0 += chunk) rc = run(b0, (N - b0 < chunk) ? N - b0 : chunk);
    if (rc) og_stream_drain(h);
    return rc;
}

int og_sweep_plan(int N, int H, int W, int n_conf, int n_hold, int chunk, char* out, size_t cap, long long* workspace_bytes) {
    if (!out || cap == 0) return fail(OG_EINVAL, "bad argument");
    OG_ALIGN(workspace_bytes);
    if (N < 0 || H <= 0 || W <= 0) return fail(OG_EINVAL, "bad N/H/W");
    if ((long long)H * W > kSweepMaxPixels) return fail(OG_EINVAL, "H*W above " + std::to_string(kSweepMaxPixels) + " pixels");
    if (n_conf < 1 || n_conf > kSweepMaxConf) return fail(OG_EINVAL, "n_conf must be 1.." + std::to_string(kSweepMaxConf));
    if (n_hold < 1 || n_hold > kSweepMaxHold) return fail(OG_EINVAL, "n_hold must be 1.." + std::to_string(kSweepMaxHold));
    const int rc = og_check_chunk(chunk, kSweepMaxChunk, true);
    if (rc) return rc;
    const int mb = chunk ? chunk : sweep_default_chunk(H, W), cb = mb < N ? mb : N;
    std::string txt;
    int n = 0;
    for (int b0 = 0; b0 < N; b0 += mb, ++n) txt += std::to_string(b0) + "|" + std::to_string(N - b0 < mb ? N - b0 : mb) + "\n";
    if (txt.size() + 1 > cap) return fail(OG_EINVAL, "plan text does not fit the buffer");
    memcpy(out, txt.c_str(), txt.size() + 1);
    if (workspace_bytes) *workspace_bytes = (long long)cb * sweep_frame_bytes(H, W, n_conf * n_hold);
    return n;
}

}  // extern "C"
