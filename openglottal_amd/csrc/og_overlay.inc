// Annotated frames (include/openglottal_hip_overlay.h; scripts/infer.py:91-124): source, green fill, green outline and yellow box
// drawn on the device.  Included by og_api.hip, as og_classic.inc is.  A handle of its own: one stream, the workspace of ONE
// micro-batch, two pinned host slots.  Per micro-batch of an outlined style: the outside background of every mask through the tiled
// blob filter's labelling (k_tblob_background_mask, then the filter's own k_tblob_seams<false>, k_tblob_flatten and k_tblob_border
// over whole-frame windows -- one path at every frame size), then k_overlay, which reads source, mask, box and labels and writes BGR.
// Every pixel of the label array is rewritten by k_tblob_background_mask before anything reads it, so a handle carries nothing from
// call to call.
#include "../../include/openglottal_hip_overlay.h"

struct og_overlay : OgStreamHandle {
    // each buffer holds the bytes of the largest micro-batch run so far
    OgBuf<int> d_la;
    OgBuf<int32_t> d_wbox;   // {0, 0, W, H} per frame of the micro-batch, 16 bytes: the labelling's windows
    int wbox_H = 0, wbox_W = 0;
    OgBuf<uint8_t> d_in, d_mask, d_out;
    OgBuf<int32_t> d_boxes;
    struct Slot {
        OgBuf<uint8_t> h_in{true}, h_mask{true}, h_out{true};
        OgBuf<int32_t> h_boxes{true};
        hipEvent_t ev = nullptr;
        int b0 = -1, nb = 0;
    } slots[2];
};

namespace {

constexpr int kOverlayMaxChunk = 1024;
constexpr long long kOverlayBatchBytes = 64ll << 20;   // of out per micro-batch

int overlay_chunk(int chunk, int H, int W) {
    const long long fit = kOverlayBatchBytes / ((long long)H * W * 3);
    return (int)(fit < 1 ? 1 : (fit < chunk ? fit : chunk));
}
bool overlay_outlined(int style, const void* masks) { return style != kOverlayNone && masks != nullptr; }
// the header's MEMORY paragraph: device bytes per frame of a streamed micro-batch
long long overlay_frame_bytes(int H, int W, int ch, int style) {
    const long long HW = (long long)H * W;
    return HW * (ch + 1 + 3) + 16 + (style != kOverlayNone ? HW * 4 + 16 : 0);
}

int check_overlay(og_overlay* h, int B, int H, int W, int ch, int style) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (B < 0 || H <= 0 || W <= 0) return fail(OG_EINVAL, "bad B/H/W");
    if ((long long)H * W > kTiledMaxPixels) return fail(OG_EINVAL, "H*W above " + std::to_string(kTiledMaxPixels) + " pixels");
    if (ch != 1 && ch != 3) return fail(OG_EINVAL, "channels must be 1 (gray) or 3 (BGR)");
    if (style < 0 || style >= kOverlayStyles) return fail(OG_EINVAL, "style must be 0 (none), 1 (contour) or 2 (fill)");
    return OG_OK;
}

// the label array and the whole-frame windows of a micro-batch of nb frames
int overlay_ensure_labels(og_overlay* h, int nb, int H, int W) {
    int rc = h->d_la.grow(h, (size_t)nb * H * W * 4, "overlay");
    if (rc) return rc;
    if ((size_t)nb * 16 <= h->d_wbox.cap && h->wbox_H == H && h->wbox_W == W) return OG_OK;
    const size_t n = std::max((size_t)nb, h->d_wbox.cap / 16);
    h->wbox_H = h->wbox_W = 0;
    if ((rc = h->d_wbox.grow(h, n * 16, "overlay"))) return rc;
    std::vector<int32_t> whole(n * 4);
    for (size_t i = 0; i < n; ++i) {
        whole[4 * i] = whole[4 * i + 1] = 0;
        whole[4 * i + 2] = W;
        whole[4 * i + 3] = H;
    }
    HIPCHK(hipStreamSynchronize(h->stream));   // (launches in flight read the old windows; the pageable source must outlive the copy)
    HIPCHK(hipMemcpy(h->d_wbox, whole.data(), n * 16, hipMemcpyHostToDevice));
    h->wbox_H = H;
    h->wbox_W = W;
    return OG_OK;
}

void overlay_free(og_overlay* h) {
    og_release(h->d_la, h->d_wbox, h->d_in, h->d_mask, h->d_out, h->d_boxes);
    for (auto& s : h->slots) {
        og_release(s.h_in, s.h_mask, s.h_out, s.h_boxes);
        if (s.ev) (void)hipEventDestroy(s.ev);
    }
}

// one micro-batch of nb resident frames.  la, wbox: the handle's label array and whole-frame windows (placeholders in a dry run).
int overlay_batch(hipStream_t st, int* la, const int32_t* wbox, int ch, const uint8_t* src, const uint8_t* masks, const int32_t* boxes, int nb,
                  int H, int W, int style, uint8_t* out) {
    const long long HW = (long long)H * W, N = (long long)nb * HW * 3;
    const bool outlined = overlay_outlined(style, masks);
    if (outlined) {
        const unsigned tiles = (unsigned)(((W + kBlobTile - 1) / kBlobTile) * (long long)((H + kBlobTile - 1) / kBlobTile));
        const dim3 gt(tiles, (unsigned)nb), gp((unsigned)((HW + 255) / 256), (unsigned)nb);
        plan_need((long long)nb * (HW * 4 + 16), 0);   // the label array and the windows
        OG_LAUNCH(k_tblob_background_mask, gt, dim3(kTileThreads), 0, st, masks, H, W, wbox, la);
        OG_LAUNCH(k_tblob_seams<false>, gt, dim3(kTileThreads), 0, st, H, W, wbox, la, la);
        OG_LAUNCH(k_tblob_flatten, gp, dim3(256), 0, st, H, W, wbox, la);
        OG_LAUNCH(k_tblob_border, gp, dim3(256), 0, st, H, W, wbox, la);
    }
    // a lane per aligned dword of out and one for the ragged ends: at most N / 4 + 1 lanes
    const dim3 go((unsigned)((N / 4 + 1 + 255) / 256));
    const int* labels = outlined ? la : nullptr;
    if (ch == 3)
        OG_LAUNCH(k_overlay<3>, go, dim3(256), 0, st, src, masks, boxes, labels, nb, H, W, style, out);
    else
        OG_LAUNCH(k_overlay<1>, go, dim3(256), 0, st, src, masks, boxes, labels, nb, H, W, style, out);
    if (g_plan) plan_write("out", out, N);
    return OG_OK;
}

int overlay_stream_impl(og_overlay* h, const uint8_t* frames, const uint8_t* const* frame_ptrs, int B, int H, int W, int ch,
                        const uint8_t* masks, const int32_t* boxes, int style, uint8_t* out) {
    int rc = check_overlay(h, B, H, W, ch, style);
    if (rc) return rc;
    OG_ALIGN(frame_ptrs);
    OG_ALIGN(boxes);
    if (B == 0) return OG_OK;
    if (!frames && !frame_ptrs) return fail(OG_EINVAL, "frames is null");
    if (!out) return fail(OG_EINVAL, "out is null");
    if (frame_ptrs)
        for (int i = 0; i < B; ++i)
            if (!frame_ptrs[i]) return fail(OG_EINVAL, "frame_ptrs[" + std::to_string(i) + "] is null");
    if ((rc = og_stream_ready(h))) return rc;
    OG_SCOPE(h);
    const size_t HW = (size_t)H * W, fb = HW * ch;
    const int chunk = overlay_chunk(h->chunk, H, W), cb = chunk < B ? chunk : B;
    const bool outlined = overlay_outlined(style, masks);
    if (outlined && (rc = overlay_ensure_labels(h, cb, H, W))) return rc;
    if ((rc = h->d_in.grow(h, cb * fb, "overlay"))) return rc;
    if ((rc = h->d_out.grow(h, cb * HW * 3, "overlay"))) return rc;
    if (masks && (rc = h->d_mask.grow(h, cb * HW, "overlay"))) return rc;
    if (boxes && (rc = h->d_boxes.grow(h, (size_t)cb * 16, "overlay"))) return rc;
    for (auto& s : h->slots) {
        if ((rc = s.h_in.grow(h, cb * fb, "overlay"))) return rc;
        if ((rc = s.h_out.grow(h, cb * HW * 3, "overlay"))) return rc;
        if (masks && (rc = s.h_mask.grow(h, cb * HW, "overlay"))) return rc;
        if (boxes && (rc = s.h_boxes.grow(h, (size_t)cb * 16, "overlay"))) return rc;
        if (!s.ev) HIPCHK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    }
    const hipStream_t st = h->stream;

    auto retire = [&](og_overlay::Slot& s) -> int {
        if (s.b0 < 0) return OG_OK;
        const int b0 = s.b0, nb = s.nb;
        s.b0 = -1;
        HIPCHK(hipEventSynchronize(s.ev));
        memcpy(out + b0 * HW * 3, s.h_out, nb * HW * 3);
        return OG_OK;
    };
    auto fill = [&](og_overlay::Slot& s, int b0, int nb) -> int {
        if (frame_ptrs)
            for (int j = 0; j < nb; ++j) memcpy(s.h_in + (size_t)j * fb, frame_ptrs[b0 + j], fb);
        else
            memcpy(s.h_in, frames + (size_t)b0 * fb, nb * fb);
        HIPCHK(hipMemcpyAsync(h->d_in, s.h_in, nb * fb, hipMemcpyHostToDevice, st));
        if (masks) {
            memcpy(s.h_mask, masks + (size_t)b0 * HW, nb * HW);
            HIPCHK(hipMemcpyAsync(h->d_mask, s.h_mask, nb * HW, hipMemcpyHostToDevice, st));
        }
        if (boxes) {
            memcpy(s.h_boxes, boxes + 4 * (size_t)b0, (size_t)nb * 16);
            HIPCHK(hipMemcpyAsync(h->d_boxes, s.h_boxes, (size_t)nb * 16, hipMemcpyHostToDevice, st));
        }
        const int rc2 = overlay_batch(st, h->d_la, h->d_wbox, ch, h->d_in, masks ? h->d_mask : nullptr, boxes ? h->d_boxes : nullptr, nb, H, W,
                                      style, h->d_out);
        if (rc2) return rc2;
        HIPCHK(hipMemcpyAsync(s.h_out, h->d_out, nb * HW * 3, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(s.ev, st));
        s.b0 = b0;
        s.nb = nb;
        return OG_OK;
    };

    return og_two_slot(B, chunk, h->slots, retire, fill, [h] { og_stream_drain(h); });
}

// the sequential labelling of the host twins: outside[p] = 1 where p is background of a component that touches the frame's edge
void overlay_outside_host(const uint8_t* mask, int H, int W, std::vector<uint8_t>& outside) {
    const int N = H * W;
    std::vector<int> L(N);
    std::vector<uint8_t> border(N, 0);
    for (int p = 0; p < N; ++p) L[p] = p;
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
    outside.assign(N, 0);
    for (int p = 0; p < N; ++p) outside[p] = !mask[p] && border[host_find(L, p)];
}

template <int C>
void overlay_host_impl(const uint8_t* frame, int H, int W, const uint8_t* mask, const int32_t* box4, int style, uint8_t* out) {
    std::vector<uint8_t> outside;
    if (overlay_outlined(style, mask) && og_overlay_draws(box4)) overlay_outside_host(mask, H, W, outside);
    const uint8_t* o = outside.data();
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            og_overlay_px<C>(frame, mask, box4, style, x, y, H, W, [o](int p) { return o[p] != 0; }, out + ((size_t)y * W + x) * 3);
}

}  // namespace

extern "C" {

long long og_overlay_limit(int which) { return which == 0 ? kTiledMaxPixels : which == 1 ? kOverlayStyles : which == 2 ? kOverlayMaxChunk : -1; }

int og_outline_host(const uint8_t* mask, int H, int W, uint8_t* out) {
    if (!mask || !out || H < 1 || W < 1 || (long long)H * W > kTiledMaxPixels) return fail(OG_EINVAL, "bad argument");
    std::vector<uint8_t> outside;
    overlay_outside_host(mask, H, W, outside);
    const uint8_t* o = outside.data();
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            out[(size_t)y * W + x] = og_outline_at(mask[(size_t)y * W + x] != 0, x, y, H, W, [o](int p) { return o[p] != 0; }) ? 255 : 0;
    return OG_OK;
}

int og_overlay_host(const uint8_t* frame, int H, int W, int channels, const uint8_t* mask_or_null, const int32_t* box4_or_null, int style,
                    uint8_t* out_bgr) {
    if (!frame || !out_bgr || H < 1 || W < 1 || (long long)H * W > kTiledMaxPixels) return fail(OG_EINVAL, "bad argument");
    if (channels != 1 && channels != 3) return fail(OG_EINVAL, "channels must be 1 (gray) or 3 (BGR)");
    if (style < 0 || style >= kOverlayStyles) return fail(OG_EINVAL, "style must be 0 (none), 1 (contour) or 2 (fill)");
    OG_ALIGN(box4_or_null);
    if (channels == 3)
        overlay_host_impl<3>(frame, H, W, mask_or_null, box4_or_null, style, out_bgr);
    else
        overlay_host_impl<1>(frame, H, W, mask_or_null, box4_or_null, style, out_bgr);
    return OG_OK;
}

og_overlay* og_overlay_create(void) { return new og_overlay(); }

void og_overlay_destroy(og_overlay* h) {
    og_stream_destroy(h, [h] { overlay_free(h); });
}

int og_overlay_sync(og_overlay* h) { return og_stream_sync(h); }

int og_overlay_set_chunk(og_overlay* h, int chunk) { return og_stream_set_chunk(h, chunk, kOverlayMaxChunk); }

int og_overlay_u8_dev(og_overlay* h, const uint8_t* frames_dev, int B, int H, int W, int channels, const uint8_t* masks_dev_or_null,
                      const int32_t* boxes_dev_or_null, int style, uint8_t* out_dev) {
    int rc = check_overlay(h, B, H, W, channels, style);
    if (rc) return rc;
    OG_ALIGN(boxes_dev_or_null);
    if (B == 0) return OG_OK;
    if (!frames_dev || !out_dev) return fail(OG_EINVAL, "null buffer");
    if ((rc = og_stream_ready(h))) return rc;
    OG_SCOPE(h);
    const size_t HW = (size_t)H * W;
    const int chunk = overlay_chunk(h->chunk, H, W), cb = chunk < B ? chunk : B;
    if (overlay_outlined(style, masks_dev_or_null) && (rc = overlay_ensure_labels(h, cb, H, W))) return rc;
    for (int b0 = 0; b0 < B && !rc; b0 += chunk) {
        const int nb = (B - b0 < chunk) ? B - b0 : chunk;
        rc = overlay_batch(h->stream, h->d_la, h->d_wbox, channels, frames_dev + b0 * HW * channels,
                           masks_dev_or_null ? masks_dev_or_null + b0 * HW : nullptr, boxes_dev_or_null ? boxes_dev_or_null + 4 * (size_t)b0 : nullptr,
                           nb, H, W, style, out_dev + b0 * HW * 3);
    }
    if (rc) og_stream_drain(h);
    return rc;
}

int og_overlay_stream_u8(og_overlay* h, const uint8_t* frames, int B, int H, int W, int channels, const uint8_t* masks_or_null,
                         const int32_t* boxes_or_null, int style, uint8_t* out) {
    return overlay_stream_impl(h, frames, nullptr, B, H, W, channels, masks_or_null, boxes_or_null, style, out);
}

int og_overlay_stream_frames_u8(og_overlay* h, const uint8_t* const* frame_ptrs, int B, int H, int W, int channels,
                                const uint8_t* masks_or_null, const int32_t* boxes_or_null, int style, uint8_t* out) {
    if (!frame_ptrs && B > 0) return fail(OG_EINVAL, "frame_ptrs is null");
    return overlay_stream_impl(h, nullptr, frame_ptrs, B, H, W, channels, masks_or_null, boxes_or_null, style, out);
}

int og_overlay_plan(int B, int H, int W, int channels, int chunk, int style, char* out, size_t cap, long long* workspace_bytes) {
    if (!out || cap == 0 || B < 1) return fail(OG_EINVAL, "bad argument");
    og_overlay tmp;
    int rc = check_overlay(&tmp, B, H, W, channels, style);
    if (rc) return rc;
    if ((rc = og_check_chunk(chunk, kOverlayMaxChunk))) return rc;
    const int mb = overlay_chunk(chunk, H, W), cb = mb < B ? mb : B;
    if (workspace_bytes) *workspace_bytes = (long long)cb * overlay_frame_bytes(H, W, channels, style);
    const uintptr_t gap = (uintptr_t)1 << 40;   // placeholder bases: nothing dereferences them in a dry run
    uint8_t* dst = (uint8_t*)(1 * gap);
    Plan plan;
    plan.bases = {{"out", dst}};
    g_plan = &plan;
    const size_t HW = (size_t)H * W;
    for (int b0 = 0; b0 < B && !rc; b0 += mb)
        rc = overlay_batch(nullptr, (int*)(2 * gap), (const int32_t*)(3 * gap), channels, (const uint8_t*)(4 * gap), (const uint8_t*)(5 * gap),
                           (const int32_t*)(6 * gap), (B - b0 < mb) ? B - b0 : mb, H, W, style, dst + b0 * HW * 3);
    g_plan = nullptr;
    if (rc) return rc;
    return og_plan_text(plan, kPlanWrites, out, cap);
}

}  // extern "C"
