// The training-free family (include/openglottal_hip_classic.h; tracker.py:117-232, eval_girafe.py:162-171): guided-VFT and
// YOLO+Otsu over frames on the device.  Included by og_api.hip, as og_crops.inc is.  A handle of its own (no network): one stream,
// the workspace of ONE micro-batch, two pinned host slots.  Per micro-batch of the guided-VFT pass: k_box_hist (ROI histograms),
// k_vft_thresholds (percentiles, then the recurrence in frame order from the handle's running threshold) and k_blobs (raw mask,
// hole fill, labelling, keys, top-n, paint, count: one workgroup per frame).  Everything is ordered by the one stream, so the
// threshold carried from micro-batch to micro-batch needs nothing else.  A handle in tiled mode (og_classic_set_tiled,
// include/openglottal_hip_classic_tiled.h) sends frames above 65 536 pixels, or all, through the k_tblob_* launches in k_blobs' place:
// many workgroups per frame, a launch boundary wherever they must see each other's results (classic_tblob_batch).
#include "../../include/openglottal_hip_classic.h"
#include "../../include/openglottal_hip_classic_tiled.h"

struct og_classic : OgStreamHandle {
    double beta = 0.7, percentile = 30.0;
    int n_comp = 2;
    int tiled = 0;   // og_classic_set_tiled: 0 off, 1 auto, 2 always
    bool seeded = false;
    double* d_state = nullptr;   // the running threshold: made with the stream (classic_ready)
    // workspace of one micro-batch
    size_t cap_nb = 0, cap_px = 0, cap_in = 0;   // frames; pixels and source bytes of the whole micro-batch
    bool cap_mask = false, cap_sel = false;
    uint8_t* d_in = nullptr;
    uint8_t* d_mask = nullptr;
    int* d_la = nullptr;
    int* d_lb = nullptr;
    uint32_t* d_hist = nullptr;
    int32_t* d_boxes = nullptr;
    double* d_thresh = nullptr;
    int32_t* d_cut = nullptr;
    int32_t* d_T = nullptr;
    int32_t* d_area = nullptr;
    int32_t* d_sel = nullptr;   // the tiled blob filter: the roots taken per frame
    struct Slot {
        uint8_t* h_in = nullptr;
        uint8_t* h_mask = nullptr;
        int32_t* h_boxes = nullptr;
        int32_t* h_area = nullptr;
        int32_t* h_T = nullptr;
        double* h_thresh = nullptr;
        hipEvent_t ev = nullptr;
        int b0 = -1, nb = 0;
    } slots[2];
};

namespace {

constexpr long long kClassicMaxPixels = 1ll << 16;   // 256 x 256: the largest frame k_blobs has been measured on (DESIGN section 15)
// the tiled blob filter (DESIGN section 18): the largest frame whose worst-case ladder has been launched and timed
constexpr long long kTiledMaxPixels = 1ll << 22;   // 2048 x 2048
constexpr int kClassicMaxChunk = 1024;
constexpr long long kClassicUploadBytes = 64ll << 20;

// bytes of device workspace per frame of a micro-batch (the header's MEMORY paragraph)
long long classic_frame_bytes(int H, int W, int ch, bool with_in, bool with_mask, bool tiled = false) {
    const long long HW = (long long)H * W;
    return (with_in ? HW * ch : 0) + (with_mask ? HW : 0) + 8 * HW + 1024 + 16 + 8 + 4 + 4 + 4 + (tiled ? 4 * kSelWords : 0);
}

// whether a frame of H x W goes through the tiled blob filter in this mode
bool classic_tiled(int mode, int H, int W) { return mode == 2 || (mode == 1 && (long long)H * W > kClassicMaxPixels); }
long long classic_max_pixels(int mode) { return mode ? kTiledMaxPixels : kClassicMaxPixels; }
// blocks per frame of k_box_hist: kHistBlocks up to 65 536 pixels, growing with the frame in the tiled modes
int classic_hist_blocks(int mode, int H, int W) {
    const long long HW = (long long)H * W;
    return (mode && HW > kClassicMaxPixels) ? (int)(kHistBlocks * ((HW + kClassicMaxPixels - 1) / kClassicMaxPixels)) : kHistBlocks;
}

int classic_chunk(int chunk, int H, int W, int ch) {
    const long long fit = kClassicUploadBytes / ((long long)H * W * ch);
    return (int)(fit < 1 ? 1 : (fit < chunk ? fit : chunk));
}

int check_classic(og_classic* h, int B, int H, int W, int ch) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (B < 0 || H <= 0 || W <= 0) return fail(OG_EINVAL, "bad B/H/W");
    if ((long long)H * W > classic_max_pixels(h->tiled)) return fail(OG_EINVAL, "H*W above " + std::to_string(classic_max_pixels(h->tiled)) + " pixels");
    if (ch != 1 && ch != 3) return fail(OG_EINVAL, "channels must be 1 (gray) or 3 (BGR)");
    return OG_OK;
}

int classic_ready(og_classic* h) {
    if (h->d_state) return OG_OK;
    const int rc = og_stream_ready(h);
    if (rc) return rc;
    HIPCHK(hipMalloc((void**)&h->d_state, sizeof(double)));
    return OG_OK;
}

void classic_free_ws(og_classic* h) {
    auto drop = [](bool pinned, auto*&... p) {   // free and forget: each pointer is listed once
        ((void)(!p ? hipSuccess : pinned ? hipHostFree(p) : hipFree(p)), ...);
        ((p = nullptr), ...);
    };
    drop(false, h->d_in, h->d_mask, h->d_la, h->d_lb, h->d_hist, h->d_boxes, h->d_thresh, h->d_cut, h->d_T, h->d_area, h->d_sel);
    for (auto& s : h->slots) {
        drop(true, s.h_in, s.h_mask, s.h_boxes, s.h_area, s.h_T, s.h_thresh);
        if (s.ev) (void)hipEventDestroy(s.ev);
        s.ev = nullptr;
        s.b0 = -1;
    }
    h->cap_nb = h->cap_px = h->cap_in = 0;
    h->cap_mask = h->cap_sel = false;
}

// the workspace of one micro-batch of nb frames; `in`: bytes of source frames per frame (0: resident frames), `host`: pinned slots too.
// Capacities are kept in BYTES of the micro-batch (nb * pixels, nb * in), never as separate maxima of nb and of the frame size: a
// handle that has seen many small frames and then a few large ones holds the larger of the two micro-batches, not their product.
int classic_ensure(og_classic* h, int nb, int H, int W, size_t in, bool want_mask, bool host) {
    const bool want_sel = classic_tiled(h->tiled, H, W);
    const size_t px = (size_t)nb * H * W, inb = (size_t)nb * in;
    const bool have_host = h->slots[0].ev != nullptr;
    if ((size_t)nb <= h->cap_nb && px <= h->cap_px && inb <= h->cap_in && (!want_mask || h->cap_mask) && (!want_sel || h->cap_sel) &&
        (!host || have_host))
        return OG_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t n = std::max((size_t)nb, h->cap_nb), p = std::max(px, h->cap_px), i = std::max(inb, h->cap_in);
    const bool m = want_mask || h->cap_mask, hs = host || have_host, sl = want_sel || h->cap_sel;
    classic_free_ws(h);
    auto dev = [&](void** q, size_t bytes) { return hipMalloc(q, bytes ? bytes : 1); };
    hipError_t e = hipSuccess;
    if (i && e == hipSuccess) e = dev((void**)&h->d_in, i);
    if (m && e == hipSuccess) e = dev((void**)&h->d_mask, p);
    if (e == hipSuccess) e = dev((void**)&h->d_la, p * 4);
    if (e == hipSuccess) e = dev((void**)&h->d_lb, p * 4);
    if (e == hipSuccess) e = dev((void**)&h->d_hist, n * 1024);
    if (e == hipSuccess) e = dev((void**)&h->d_boxes, n * 16);
    if (e == hipSuccess) e = dev((void**)&h->d_thresh, n * 8);
    if (e == hipSuccess) e = dev((void**)&h->d_cut, n * 4);
    if (e == hipSuccess) e = dev((void**)&h->d_T, n * 4);
    if (e == hipSuccess) e = dev((void**)&h->d_area, n * 4);
    if (sl && e == hipSuccess) e = dev((void**)&h->d_sel, n * 4 * kSelWords);
    for (auto& s : h->slots) {
        if (!hs) break;
        if (e == hipSuccess) e = hipHostMalloc((void**)&s.h_in, i ? i : 1, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void**)&s.h_mask, p, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void**)&s.h_boxes, n * 16, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void**)&s.h_area, n * 4, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void**)&s.h_T, n * 4, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void**)&s.h_thresh, n * 8, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.ev, hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        classic_free_ws(h);
        return fail(e == hipErrorOutOfMemory ? OG_ENOMEM : OG_EHIP, std::string("classic workspace: ") + hipGetErrorString(e));
    }
    h->cap_nb = n;
    h->cap_px = p;
    h->cap_in = i;
    h->cap_mask = m;
    h->cap_sel = sl;
    return OG_OK;
}

// ws: where the micro-batch's histograms, labels, thresholds and cuts live (the handle's, or placeholders in a dry run)
struct ClassicWs {
    uint32_t* hist;
    int* la;
    int* lb;
    double* state;
    double* thresh;
    int32_t* cut;
    int32_t* T;
    int32_t* sel = nullptr;   // tiled blob filter only
    int mode = 0;             // og_classic_set_tiled
};
ClassicWs classic_ws(const og_classic* h) { return {h->d_hist, h->d_la, h->d_lb, h->d_state, h->d_thresh, h->d_cut, h->d_T, h->d_sel, h->tiled}; }

int enqueue_box_hist(hipStream_t st, int mode, int ch, const uint8_t* src, int nb, int H, int W, const int32_t* boxes, uint32_t* hist) {
    if (!g_plan) HIPCHK(hipMemsetAsync(hist, 0, (size_t)nb * 1024, st));
    const dim3 grid((unsigned)classic_hist_blocks(mode, H, W), (unsigned)nb);
    if (ch == 3)
        OG_LAUNCH(k_box_hist<3>, grid, dim3(256), 0, st, src, H, W, boxes, hist);
    else
        OG_LAUNCH(k_box_hist<1>, grid, dim3(256), 0, st, src, H, W, boxes, hist);
    return OG_OK;
}

// the tiled blob filter over one micro-batch (the launch list of og_kernels.hpp): every launch boundary is a hand-off between the
// workgroups of a frame.  Grids: tiles x frames for the tile kernels, pixels x frames for the rest.
int classic_tblob_batch(hipStream_t st, const ClassicWs& ws, int n_comp, int ch, const uint8_t* src, int nb, int H, int W, const int32_t* boxes,
                        uint8_t* mask, int32_t* area) {
    const long long HW = (long long)H * W;
    const unsigned tiles = (unsigned)(((W + kBlobTile - 1) / kBlobTile) * (long long)((H + kBlobTile - 1) / kBlobTile));
    const dim3 gt(tiles, (unsigned)nb), gp((unsigned)((HW + 255) / 256), (unsigned)nb);
    const dim3 gk((unsigned)(((long long)(H + 1) * (W + 1) + 255) / 256), (unsigned)nb);
    plan_need((long long)nb * HW * 8 + (long long)nb * 4 * kSelWords, 0);   // the two label arrays and the roots taken, per frame
    if (ch == 3)
        OG_LAUNCH(k_tblob_background<3>, gt, dim3(kTileThreads), 0, st, src, H, W, boxes, ws.cut, ws.la);
    else
        OG_LAUNCH(k_tblob_background<1>, gt, dim3(kTileThreads), 0, st, src, H, W, boxes, ws.cut, ws.la);
    OG_LAUNCH(k_tblob_seams<false>, gt, dim3(kTileThreads), 0, st, H, W, boxes, ws.la, ws.lb);
    OG_LAUNCH(k_tblob_flatten, gp, dim3(256), 0, st, H, W, boxes, ws.la);
    OG_LAUNCH(k_tblob_border, gp, dim3(256), 0, st, H, W, boxes, ws.la);
    OG_LAUNCH(k_tblob_fill, gt, dim3(kTileThreads), 0, st, H, W, boxes, ws.la, ws.lb);
    OG_LAUNCH(k_tblob_seams<true>, gt, dim3(kTileThreads), 0, st, H, W, boxes, ws.la, ws.lb);
    OG_LAUNCH(k_tblob_flatten, gp, dim3(256), 0, st, H, W, boxes, ws.lb);
    OG_LAUNCH(k_tblob_keys, gk, dim3(256), 0, st, H, W, boxes, ws.la, ws.lb);
    OG_LAUNCH(k_tblob_select, dim3((unsigned)nb), dim3(kBlobThreads), 0, st, H, W, boxes, n_comp, ws.la, ws.lb, ws.sel);
    if (!g_plan) HIPCHK(hipMemsetAsync(area, 0, (size_t)nb * 4, st));
    OG_LAUNCH(k_tblob_paint, gp, dim3(256), 0, st, H, W, boxes, ws.lb, ws.sel, mask, area);
    if (g_plan) {
        plan_write("mask", mask, (long long)nb * HW);
        plan_write("area", area, (long long)nb * 4);
    }
    return OG_OK;
}

// one micro-batch of nb resident frames of the guided-VFT pass; thresholds and cuts are left in ws
int classic_vft_batch(hipStream_t st, const ClassicWs& ws, double beta, double q, int n_comp, int ch, const uint8_t* src, int nb, int H, int W,
                      const int32_t* boxes, uint8_t* mask, int32_t* area) {
    int rc = enqueue_box_hist(st, ws.mode, ch, src, nb, H, W, boxes, ws.hist);
    if (rc) return rc;
    OG_LAUNCH(k_vft_thresholds, dim3(1), dim3(256), 0, st, ws.hist, nb, q, beta, ws.state, ws.thresh, ws.cut);
    if (classic_tiled(ws.mode, H, W)) return classic_tblob_batch(st, ws, n_comp, ch, src, nb, H, W, boxes, mask, area);
    plan_need((long long)nb * H * W * 8, 0);   // the two label arrays of each frame
    if (ch == 3)
        OG_LAUNCH(k_blobs<3>, dim3((unsigned)nb), dim3(kBlobThreads), 0, st, src, H, W, boxes, ws.cut, n_comp, ws.la, ws.lb, mask, area);
    else
        OG_LAUNCH(k_blobs<1>, dim3((unsigned)nb), dim3(kBlobThreads), 0, st, src, H, W, boxes, ws.cut, n_comp, ws.la, ws.lb, mask, area);
    if (g_plan) {
        plan_write("mask", mask, (long long)nb * H * W);
        plan_write("area", area, (long long)nb * 4);
    }
    return OG_OK;
}

// one micro-batch of the Otsu pass; T is left in ws (area must be zero on entry: zeroed here)
int classic_otsu_batch(hipStream_t st, const ClassicWs& ws, int ch, const uint8_t* src, int nb, int H, int W, const int32_t* boxes,
                       uint8_t* mask, int32_t* area) {
    int rc = enqueue_box_hist(st, ws.mode, ch, src, nb, H, W, boxes, ws.hist);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(area, 0, (size_t)nb * 4, st));
    OG_LAUNCH(k_otsu_thresholds, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, st, ws.hist, nb, ws.T, ws.cut);
    const dim3 grid((unsigned)(((long long)H * W + 255) / 256), (unsigned)nb);
    if (ch == 3)
        OG_LAUNCH(k_threshold_in_box<3>, grid, dim3(256), 0, st, src, H, W, boxes, ws.cut, mask, area);
    else
        OG_LAUNCH(k_threshold_in_box<1>, grid, dim3(256), 0, st, src, H, W, boxes, ws.cut, mask, area);
    return OG_OK;
}

// the host entries of both passes: micro-batches through the two pinned slots.  otsu: T instead of thresh, no state.
int classic_stream_impl(og_classic* h, bool otsu, const uint8_t* frames, const uint8_t* const* frame_ptrs, int B, int H, int W, int ch,
                        const int32_t* boxes, uint8_t* mask, int32_t* area, double* thresh, int32_t* T) {
    int rc = check_classic(h, B, H, W, ch);
    if (rc) return rc;
    OG_ALIGN(frame_ptrs);
    OG_ALIGN(boxes);
    OG_ALIGN(area);
    OG_ALIGN(thresh);
    OG_ALIGN(T);
    if (!otsu && !h->seeded) return fail(OG_ESTATE, "no running threshold: call og_vft_guided_init_u8 or og_vft_guided_set_state first");
    if (B == 0) return OG_OK;
    if (!frames && !frame_ptrs) return fail(OG_EINVAL, "frames is null");
    if (!boxes || !area || (otsu && !T)) return fail(OG_EINVAL, "null buffer");
    if (frame_ptrs)
        for (int i = 0; i < B; ++i)
            if (!frame_ptrs[i]) return fail(OG_EINVAL, "frame_ptrs[" + std::to_string(i) + "] is null");
    if ((rc = classic_ready(h))) return rc;
    OG_SCOPE(h);
    const size_t HW = (size_t)H * W, fb = HW * ch;
    const int chunk = classic_chunk(h->chunk, H, W, ch), cb = chunk < B ? chunk : B;
    if ((rc = classic_ensure(h, cb, H, W, fb, mask != nullptr, true))) return rc;
    const ClassicWs ws = classic_ws(h);
    const hipStream_t st = h->stream;

    auto retire = [&](og_classic::Slot& s) -> int {
        if (s.b0 < 0) return OG_OK;
        const int b0 = s.b0, nb = s.nb;
        s.b0 = -1;
        HIPCHK(hipEventSynchronize(s.ev));
        memcpy(area + b0, s.h_area, (size_t)nb * 4);
        if (mask) memcpy(mask + b0 * HW, s.h_mask, nb * HW);
        if (thresh) memcpy(thresh + b0, s.h_thresh, (size_t)nb * 8);
        if (T) memcpy(T + b0, s.h_T, (size_t)nb * 4);
        return OG_OK;
    };
    auto fill = [&](og_classic::Slot& s, int b0, int nb) -> int {
        if (frame_ptrs)
            for (int j = 0; j < nb; ++j) memcpy(s.h_in + (size_t)j * fb, frame_ptrs[b0 + j], fb);
        else
            memcpy(s.h_in, frames + (size_t)b0 * fb, nb * fb);
        memcpy(s.h_boxes, boxes + 4 * (size_t)b0, (size_t)nb * 16);
        HIPCHK(hipMemcpyAsync(h->d_in, s.h_in, nb * fb, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(h->d_boxes, s.h_boxes, (size_t)nb * 16, hipMemcpyHostToDevice, st));
        const int rc2 = otsu ? classic_otsu_batch(st, ws, ch, h->d_in, nb, H, W, h->d_boxes, mask ? h->d_mask : nullptr, h->d_area)
                             : classic_vft_batch(st, ws, h->beta, h->percentile, h->n_comp, ch, h->d_in, nb, H, W, h->d_boxes,
                                                 mask ? h->d_mask : nullptr, h->d_area);
        if (rc2) return rc2;
        HIPCHK(hipMemcpyAsync(s.h_area, h->d_area, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
        if (mask) HIPCHK(hipMemcpyAsync(s.h_mask, h->d_mask, nb * HW, hipMemcpyDeviceToHost, st));
        if (thresh) HIPCHK(hipMemcpyAsync(s.h_thresh, h->d_thresh, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
        if (T) HIPCHK(hipMemcpyAsync(s.h_T, h->d_T, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(s.ev, st));
        s.b0 = b0;
        s.nb = nb;
        return OG_OK;
    };

    return og_two_slot(B, chunk, h->slots, retire, fill, [h] { og_stream_drain(h); });
}

int classic_dev_impl(og_classic* h, bool otsu, const uint8_t* src, int B, int H, int W, int ch, const int32_t* boxes, uint8_t* mask,
                     int32_t* area, double* thresh, int32_t* T) {
    int rc = check_classic(h, B, H, W, ch);
    if (rc) return rc;
    OG_ALIGN(boxes);
    OG_ALIGN(area);
    OG_ALIGN(thresh);
    OG_ALIGN(T);
    if (!otsu && !h->seeded) return fail(OG_ESTATE, "no running threshold: call og_vft_guided_init_u8 or og_vft_guided_set_state first");
    if (B == 0) return OG_OK;
    if (!src || !boxes || !area || (otsu && !T)) return fail(OG_EINVAL, "null buffer");
    if ((rc = classic_ready(h))) return rc;
    OG_SCOPE(h);
    const size_t HW = (size_t)H * W;
    const int chunk = classic_chunk(h->chunk, H, W, ch), cb = chunk < B ? chunk : B;
    if ((rc = classic_ensure(h, cb, H, W, 0, false, false))) return rc;
    const ClassicWs ws = classic_ws(h);
    for (int b0 = 0; b0 < B && !rc; b0 += chunk) {
        const int nb = (B - b0 < chunk) ? B - b0 : chunk;
        const uint8_t* s = src + b0 * HW * ch;
        uint8_t* m = mask ? mask + b0 * HW : nullptr;
        rc = otsu ? classic_otsu_batch(h->stream, ws, ch, s, nb, H, W, boxes + 4 * (size_t)b0, m, area + b0)
                  : classic_vft_batch(h->stream, ws, h->beta, h->percentile, h->n_comp, ch, s, nb, H, W, boxes + 4 * (size_t)b0, m, area + b0);
        if (!rc && thresh) HIPCHK(hipMemcpyAsync(thresh + b0, h->d_thresh, (size_t)nb * 8, hipMemcpyDeviceToDevice, h->stream));
        if (!rc && T) HIPCHK(hipMemcpyAsync(T + b0, h->d_T, (size_t)nb * 4, hipMemcpyDeviceToDevice, h->stream));
    }
    if (rc) og_stream_drain(h);
    return rc;
}

// sequential union-find by minimum index (the root of a set is its smallest member, as in the kernel)
int host_find(std::vector<int>& L, int x) {
    while (L[x] != x) x = L[x] = L[L[x]];
    return x;
}
void host_union(std::vector<int>& L, int a, int b) {
    a = host_find(L, a);
    b = host_find(L, b);
    if (a == b) return;
    if (a < b) L[b] = a;
    else L[a] = b;
}

}  // namespace

extern "C" {

long long og_classic_limit(int which) {
    return which == 0 ? kClassicMaxPixels : which == 1 ? kBlobMax : which == 2 ? kClassicMaxChunk : which == 3 ? kClassicUploadBytes : -1;
}

int og_percentile_host(const uint32_t* hist256, double q, double* out) {
    if (!hist256 || !out || !(q >= 0.0 && q <= 100.0)) return fail(OG_EINVAL, "bad argument");
    OG_ALIGN(hist256);
    OG_ALIGN(out);
    const long long n = og_hist_count(hist256);
    if (n < 1) return fail(OG_EINVAL, "empty histogram");
    *out = og_percentile_hist(hist256, n, q);
    return OG_OK;
}

int og_otsu_threshold_host(const uint32_t* hist256, int32_t* T) {
    if (!hist256 || !T) return fail(OG_EINVAL, "bad argument");
    OG_ALIGN(hist256);
    OG_ALIGN(T);
    const long long n = og_hist_count(hist256);
    if (n < 1) return fail(OG_EINVAL, "empty histogram");
    *T = og_otsu_hist(hist256, n);
    return OG_OK;
}

int og_box_hist_host(const uint8_t* frame, int H, int W, int channels, const int32_t* box4, uint32_t* hist256) {
    if (!frame || !box4 || !hist256 || H < 1 || W < 1 || (channels != 1 && channels != 3)) return fail(OG_EINVAL, "bad argument");
    OG_ALIGN(box4);
    OG_ALIGN(hist256);
    int r[4];
    const bool ok = og_roi(box4[0], box4[1], box4[2], box4[3], H, W, r);
    memset(hist256, 0, 1024);
    if (ok)
        for (int y = r[1]; y < r[3]; ++y)
            for (int x = r[0]; x < r[2]; ++x)
                ++hist256[channels == 3 ? og_gray_at<3>(frame, (long long)y * W + x) : og_gray_at<1>(frame, (long long)y * W + x)];
    return OG_OK;
}

int og_vft_step_host(double thresh, double beta, const uint32_t* hist256, double q, double* thresh_out, int32_t* cut_out) {
    if (!hist256 || !thresh_out || !cut_out || !(q >= 0.0 && q <= 100.0)) return fail(OG_EINVAL, "bad argument");
    OG_ALIGN(hist256);
    OG_ALIGN(thresh_out);
    OG_ALIGN(cut_out);
    const double t = og_vft_next(thresh, beta, hist256, q);
    *thresh_out = t;
    *cut_out = og_vft_cut(t);
    return OG_OK;
}

// the body of og_blobs_host and og_blobs_host_any: H * W fits an int
int blobs_host_impl(const uint8_t* mask, int H, int W, int n_components, uint8_t* out_mask_or_null, int32_t* area) {
    if (n_components < 1 || n_components > kBlobMax) return fail(OG_EINVAL, "n_components must be 1.." + std::to_string(kBlobMax));
    OG_ALIGN(area);
    const int N = H * W;
    std::vector<int> L(N);
    std::vector<uint8_t> filled(N), border(N, 0);
    for (int p = 0; p < N; ++p) L[p] = p;
    // background, 4-connected; border contact per root
    for (int p = 0; p < N; ++p) {
        if (mask[p]) continue;
        const int y = p / W, x = p - y * W;
        if (x > 0 && !mask[p - 1]) host_union(L, p, p - 1);
        if (y > 0 && !mask[p - W]) host_union(L, p, p - W);
    }
    for (int p = 0; p < N; ++p) {
        const int y = p / W, x = p - y * W;
        if (!mask[p] && (x == 0 || y == 0 || x == W - 1 || y == H - 1)) border[host_find(L, p)] = 1;
    }
    for (int p = 0; p < N; ++p) filled[p] = mask[p] || !border[host_find(L, p)];
    // the filled mask, 8-connected
    for (int p = 0; p < N; ++p) L[p] = p;
    for (int p = 0; p < N; ++p) {
        if (!filled[p]) continue;
        const int y = p / W, x = p - y * W;
        if (x > 0 && filled[p - 1]) host_union(L, p, p - 1);
        if (y > 0) {
            if (filled[p - W]) host_union(L, p, p - W);
            if (x > 0 && filled[p - W - 1]) host_union(L, p, p - W - 1);
            if (x < W - 1 && filled[p - W + 1]) host_union(L, p, p - W + 1);
        }
    }
    std::vector<unsigned> key(N, 0);
    for (int wy = 0; wy <= H; ++wy)
        for (int wx = 0; wx <= W; ++wx) {
            int cnt = 0, root = -1;
            for (int k = 0; k < 4; ++k) {
                const int y = wy - 1 + (k >> 1), x = wx - 1 + (k & 1);
                if (y < 0 || y >= H || x < 0 || x >= W || !filled[y * W + x]) continue;
                ++cnt;
                root = host_find(L, y * W + x);
            }
            if (og_window_key(cnt)) key[root] += og_window_key(cnt);
        }
    std::vector<unsigned long long> ranks;
    for (int p = 0; p < N; ++p)
        if (filled[p] && L[p] == p) ranks.push_back(og_blob_rank(key[p], (unsigned)p));
    std::sort(ranks.begin(), ranks.end(), [](unsigned long long a, unsigned long long b) { return a > b; });
    if ((int)ranks.size() > n_components) ranks.resize(n_components);
    std::vector<uint8_t> take(N, 0);
    for (unsigned long long r : ranks) take[og_blob_rank_first(r)] = 1;
    int cnt = 0;
    for (int p = 0; p < N; ++p) {
        const bool on = filled[p] && take[host_find(L, p)];
        if (out_mask_or_null) out_mask_or_null[p] = on ? 255 : 0;
        cnt += on ? 1 : 0;
    }
    *area = cnt;
    return OG_OK;
}

int og_blobs_host(const uint8_t* mask, int H, int W, int n_components, uint8_t* out_mask_or_null, int32_t* area) {
    if (!mask || !area || H < 1 || W < 1 || (long long)H * W > kClassicMaxPixels) return fail(OG_EINVAL, "bad argument");
    return blobs_host_impl(mask, H, W, n_components, out_mask_or_null, area);
}

int og_blobs_host_any(const uint8_t* mask, int H, int W, int n_components, uint8_t* out_mask_or_null, int32_t* area) {
    if (!mask || !area || H < 1 || W < 1 || (long long)H * W > (1ll << 30)) return fail(OG_EINVAL, "bad argument");
    return blobs_host_impl(mask, H, W, n_components, out_mask_or_null, area);
}

long long og_classic_tiled_limit(int which) { return which == 0 ? kTiledMaxPixels : which == 1 ? kBlobTile : -1; }

int og_classic_set_tiled(og_classic* h, int mode) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (mode < 0 || mode > 2) return fail(OG_EINVAL, "tiled mode must be 0 (off), 1 (auto) or 2 (always)");
    h->tiled = mode;
    return OG_OK;
}

og_classic* og_classic_create(void) { return new og_classic(); }

void og_classic_destroy(og_classic* h) {
    og_stream_destroy(h, [h] {
        classic_free_ws(h);
        (void)hipFree(h->d_state);
    });
}

int og_classic_sync(og_classic* h) { return og_stream_sync(h); }

int og_classic_set_chunk(og_classic* h, int chunk) { return og_stream_set_chunk(h, chunk, kClassicMaxChunk); }

int og_vft_guided_reset(og_classic* h, double beta, double percentile, int n_components) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (!(percentile >= 0.0 && percentile <= 100.0)) return fail(OG_EINVAL, "percentile must be 0..100");
    if (beta != beta) return fail(OG_EINVAL, "beta is NaN");
    if (n_components < 1 || n_components > kBlobMax) return fail(OG_EINVAL, "n_components must be 1.." + std::to_string(kBlobMax));
    h->beta = beta;
    h->percentile = percentile;
    h->n_comp = n_components;
    h->seeded = false;
    return OG_OK;
}

int og_vft_guided_set_state(og_classic* h, double thresh) {
    if (!h) return fail(OG_EINVAL, "null handle");
    int rc = classic_ready(h);
    if (rc) return rc;
    OG_SCOPE(h);
    HIPCHK(hipStreamSynchronize(h->stream));   // (the pageable source must outlive the copy)
    HIPCHK(hipMemcpy(h->d_state, &thresh, sizeof(double), hipMemcpyHostToDevice));
    h->seeded = true;
    return OG_OK;
}

int og_vft_guided_get_state(og_classic* h, double* thresh) {
    if (!h || !thresh) return fail(OG_EINVAL, "bad argument");
    OG_ALIGN(thresh);
    if (!h->seeded) return fail(OG_ESTATE, "no running threshold");
    OG_SCOPE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(thresh, h->d_state, sizeof(double), hipMemcpyDeviceToHost));
    return OG_OK;
}

int og_vft_guided_init_u8(og_classic* h, const uint8_t* frames, int n, int H, int W, int channels, const int32_t* box4_or_null,
                          double* thresh_out) {
    int rc = check_classic(h, n, H, W, channels);
    if (rc) return rc;
    OG_ALIGN(box4_or_null);
    OG_ALIGN(thresh_out);
    if (n < 1 || !frames) return fail(OG_EINVAL, "at least one frame is needed");
    if ((rc = classic_ready(h))) return rc;
    OG_SCOPE(h);
    const size_t fb = (size_t)H * W * channels;
    if ((rc = classic_ensure(h, 1, H, W, fb, false, true))) return rc;
    og_classic::Slot& s = h->slots[0];
    int r[4];
    const bool roi = box4_or_null && og_roi(box4_or_null[0], box4_or_null[1], box4_or_null[2], box4_or_null[3], H, W, r);
    const int32_t whole[4] = {0, 0, W, H};
    memcpy(s.h_boxes, roi ? box4_or_null : whole, 16);   // tracker.py:201: the whole frame when the ROI is empty
    memcpy(s.h_in, frames + (size_t)(n - 1) * fb, fb);
    HIPCHK(hipMemcpyAsync(h->d_in, s.h_in, fb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_boxes, s.h_boxes, 16, hipMemcpyHostToDevice, h->stream));
    rc = enqueue_box_hist(h->stream, h->tiled, channels, h->d_in, 1, H, W, h->d_boxes, h->d_hist);
    if (!rc) {
        hipLaunchKernelGGL(k_vft_seed, dim3(1), dim3(1), 0, h->stream, h->d_hist, h->percentile, h->d_state);
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) rc = fail(OG_EHIP, std::string("k_vft_seed: ") + hipGetErrorString(le));
    }
    if (!rc) {
        const hipError_t e = hipMemcpyAsync(s.h_thresh, h->d_state, 8, hipMemcpyDeviceToHost, h->stream);
        if (e != hipSuccess) rc = fail(OG_EHIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
    }
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (!rc && e != hipSuccess) rc = fail(OG_EHIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    if (rc) return rc;
    h->seeded = true;
    if (thresh_out) *thresh_out = *s.h_thresh;
    return OG_OK;
}

int og_vft_guided_stream_u8(og_classic* h, const uint8_t* frames, int B, int H, int W, int channels, const int32_t* boxes,
                            uint8_t* mask_or_null, int32_t* area, double* thresh_or_null) {
    return classic_stream_impl(h, false, frames, nullptr, B, H, W, channels, boxes, mask_or_null, area, thresh_or_null, nullptr);
}

int og_vft_guided_stream_frames_u8(og_classic* h, const uint8_t* const* frame_ptrs, int B, int H, int W, int channels,
                                   const int32_t* boxes, uint8_t* mask_or_null, int32_t* area, double* thresh_or_null) {
    if (!frame_ptrs && B > 0) return fail(OG_EINVAL, "frame_ptrs is null");
    return classic_stream_impl(h, false, nullptr, frame_ptrs, B, H, W, channels, boxes, mask_or_null, area, thresh_or_null, nullptr);
}

int og_vft_guided_u8_dev(og_classic* h, const uint8_t* frames_dev, int B, int H, int W, int channels, const int32_t* boxes_dev,
                         uint8_t* mask_dev_or_null, int32_t* area_dev, double* thresh_dev_or_null) {
    return classic_dev_impl(h, false, frames_dev, B, H, W, channels, boxes_dev, mask_dev_or_null, area_dev, thresh_dev_or_null, nullptr);
}

int og_otsu_in_box_u8(og_classic* h, const uint8_t* frames, int B, int H, int W, int channels, const int32_t* boxes, uint8_t* mask_or_null,
                      int32_t* area, int32_t* T) {
    return classic_stream_impl(h, true, frames, nullptr, B, H, W, channels, boxes, mask_or_null, area, nullptr, T);
}

int og_otsu_in_box_u8_dev(og_classic* h, const uint8_t* frames_dev, int B, int H, int W, int channels, const int32_t* boxes_dev,
                          uint8_t* mask_dev_or_null, int32_t* area_dev, int32_t* T_dev) {
    return classic_dev_impl(h, true, frames_dev, B, H, W, channels, boxes_dev, mask_dev_or_null, area_dev, nullptr, T_dev);
}

}  // extern "C"

namespace {
int classic_plan_impl(int B, int H, int W, int channels, int chunk, int mode, char* out, size_t cap, long long* workspace_bytes) {
    if (!out || cap == 0 || B < 1) return fail(OG_EINVAL, "bad argument");
    og_classic tmp;
    tmp.tiled = mode;
    int rc = check_classic(&tmp, B, H, W, channels);
    if (rc) return rc;
    if ((rc = og_check_chunk(chunk, kClassicMaxChunk))) return rc;
    const int mb = classic_chunk(chunk, H, W, channels), cb = mb < B ? mb : B;
    if (workspace_bytes) *workspace_bytes = (long long)cb * classic_frame_bytes(H, W, channels, true, true, classic_tiled(mode, H, W)) + 8;
    const uintptr_t gap = (uintptr_t)1 << 40;   // placeholder bases: nothing dereferences them in a dry run
    uint8_t* mask = (uint8_t*)(1 * gap);
    int32_t* area = (int32_t*)(2 * gap);
    const ClassicWs ws = {(uint32_t*)(3 * gap), (int*)(4 * gap), (int*)(5 * gap), (double*)(6 * gap), (double*)(7 * gap), (int32_t*)(8 * gap),
                          (int32_t*)(9 * gap), (int32_t*)(12 * gap), mode};
    Plan plan;
    plan.bases = {{"mask", mask}, {"area", area}};
    g_plan = &plan;
    for (int b0 = 0; b0 < B && !rc; b0 += mb)
        rc = classic_vft_batch(nullptr, ws, 0.7, 30.0, 2, channels, (const uint8_t*)(10 * gap), (B - b0 < mb) ? B - b0 : mb, H, W,
                               (const int32_t*)(11 * gap), mask, area);
    g_plan = nullptr;
    if (rc) return rc;
    return og_plan_text(plan, kPlanWrites, out, cap);
}
}  // namespace

extern "C" {

int og_classic_plan(int B, int H, int W, int channels, int chunk, char* out, size_t cap, long long* workspace_bytes) {
    return classic_plan_impl(B, H, W, channels, chunk, 0, out, cap, workspace_bytes);
}

int og_classic_plan_tiled(int B, int H, int W, int channels, int chunk, int mode, char* out, size_t cap, long long* workspace_bytes) {
    if (mode != 1 && mode != 2) return fail(OG_EINVAL, "tiled mode must be 1 (auto) or 2 (always)");
    return classic_plan_impl(B, H, W, channels, chunk, mode, out, cap, workspace_bytes);
}

}  // extern "C"
