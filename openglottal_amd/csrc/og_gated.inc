// The detection-gated pipeline in one device pass (include/openglottal_hip_gated.h; detector.py:61-96, features.py:234-245).
// Included by og_api.hip, as og_classic.inc is.  The handle borrows a U-Net and a detector handle and owns: the tracker's state
// words, a copy-in and a copy-out stream, and two slots of one micro-batch each (pinned host and device).  Per micro-batch:
//   s_h2d        frames (and resets) up                                                  -> ev_up
//   yolo stream  waits ev_up; og_yolo_detect_resized_u8_dev, k_track_boxes               -> ev_det
//   unet stream  waits ev_det; og_unet_segment_resized_u8_dev on the same device frames  -> ev_seg
//   s_d2h        waits ev_seg; area / boxes / best / mask down                           -> ev_out
// The tracker's state goes from micro-batch to micro-batch, and from call to call, by the order of the detector's stream alone.
// The *_kept_* entries of og_gate.inc run the same loop with the U-Net step replaced by select / gather / network on the kept frames /
// scatter (gated_stream_impl's `kept` flag; off, the loop below enqueues exactly what it always did).
#include "../../include/openglottal_hip_gated.h"

static_assert(sizeof(og_track_state) == sizeof(OgTrackState) && sizeof(og_track_state) == 24, "og_track_state is OgTrackState");

struct og_gated {
    og_unet* unet = nullptr;
    og_yolo* yolo = nullptr;
    int device = 0;
    bool ready = false;   // streams and state words exist (og_gated_create made them)
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    OgTrackState* d_state = nullptr;
    OgTrackParams params{30.f, 8, 3};
    int stage_kib = 65536;
    size_t cap_in = 0, cap_nb = 0, cap_mask = 0;   // bytes of source frames, frames and mask bytes a slot holds
    struct Slot {
        uint8_t *h_in = nullptr, *d_in = nullptr, *h_mask = nullptr, *d_mask = nullptr, *h_resets = nullptr, *d_resets = nullptr;
        float *h_best = nullptr, *d_best = nullptr;
        int32_t *h_boxes = nullptr, *d_boxes = nullptr, *h_area = nullptr, *d_area = nullptr;
        hipEvent_t ev_up = nullptr, ev_det = nullptr, ev_seg = nullptr, ev_out = nullptr;
        int b0 = -1, nb = 0;
    } slots[2];
    // og_gate.inc (include/openglottal_hip_gate.h): the dense buffers of the kept entries, one set per slot and one for
    // og_gated_segment_kept_dev; nothing of it exists until a kept entry is first used
    struct Gate {
        uint8_t *d_dense = nullptr, *d_mask = nullptr;
        int32_t *d_keep = nullptr, *d_boxes = nullptr, *d_area = nullptr, *d_count = nullptr, *h_count = nullptr;
        hipEvent_t ev_cnt = nullptr;
        size_t cap_n = 0, cap_in = 0, cap_mask = 0;   // frames, bytes of dense frames, bytes of dense masks
    } gate[3];
};
inline bool og_skip_device(const og_gated* g) { return !g || !g->ready; }

namespace {

constexpr int kGatedMaxBatch = 4096;          // most frames per micro-batch, however small the frames
constexpr int kGatedMaxStageKib = 1 << 24;
constexpr long long kGatedRowBytes = 20 + 16 + 4 + 1;   // best, box, area, reset of one frame

// frames a slot holds: a function of the setting and the frame size alone, so that the engine's memory does not depend on B
int gated_cap(int H, int W, int ch, int stage_kib) {
    long long fit = ((long long)stage_kib << 10) / ((long long)H * W * ch);
    if (fit < 1) fit = 1;   // a frame larger than the setting is staged alone
    return (int)(fit > kGatedMaxBatch ? kGatedMaxBatch : fit);
}

long long gated_engine_bytes(int nb, int H, int W, int ch, bool with_mask) {
    return 2 * (long long)nb * ((long long)H * W * (ch + (with_mask ? 1 : 0)) + kGatedRowBytes) + (long long)sizeof(OgTrackState);
}

int check_gated_shape(int B, int H, int W, int ch) {
    if (B < 0 || H <= 0 || W <= 0) return fail(OG_EINVAL, "bad B/H/W");
    if (H > kResizeMaxSide || W > kResizeMaxSide) return fail(OG_EINVAL, "frame side above " + std::to_string(kResizeMaxSide));
    if (ch != 1 && ch != 3) return fail(OG_EINVAL, "channels must be 1 (gray) or 3 (BGR)");
    return OG_OK;
}

// og_gate.inc: the U-Net step of a micro-batch on the kept frames only, and the release of what it allocated
int gate_ensure(og_gated* g, og_gated::Gate& k, int nb, size_t in, size_t mask1);
int gate_select_enqueue(og_gated* g, og_gated::Gate& k, const int32_t* boxes, int B, hipStream_t st);
int gate_segment_enqueue(og_gated* g, og_gated::Gate& k, const uint8_t* src, int B, int H, int W, int ch, int Hn, int Wn, float thr,
                         const int32_t* boxes, uint8_t* mask, int32_t* area, int* n_out);
void gate_free(og_gated* g);

int check_track_params(const og_track_params* p) {
    if (!p) return fail(OG_EINVAL, "params is null");
    if (!(p->max_shift_px >= 0.0f)) return fail(OG_EINVAL, "max_shift_px must be a number >= 0");
    if (p->padding < -(1 << 20) || p->padding > (1 << 20)) return fail(OG_EINVAL, "padding out of range");
    if (p->max_hold_frames < 0) return fail(OG_EINVAL, "max_hold_frames must be >= 0");
    return OG_OK;
}

void gated_free_slots(og_gated* g) {
    for (auto& s : g->slots) {
        void* dev[] = {s.d_in, s.d_mask, s.d_resets, s.d_best, s.d_boxes, s.d_area};
        for (void* p : dev)
            if (p) (void)hipFree(p);
        void* host[] = {s.h_in, s.h_mask, s.h_resets, s.h_best, s.h_boxes, s.h_area};
        for (void* p : host)
            if (p) (void)hipHostFree(p);
        s.h_in = s.d_in = s.h_mask = s.d_mask = s.h_resets = s.d_resets = nullptr;
        s.h_best = s.d_best = nullptr;
        s.h_boxes = s.d_boxes = s.h_area = s.d_area = nullptr;
        s.b0 = -1;
    }
    g->cap_in = g->cap_nb = g->cap_mask = 0;
}

// wait for everything the three handles have in flight on the engine's behalf; the message of a failed call survives the wait
void gated_drain(og_gated* g) {
    const std::string err = g_err;
    (void)hipStreamSynchronize(g->s_h2d);
    (void)hipStreamSynchronize(g->yolo->stream);
    (void)hipStreamSynchronize(g->unet->stream);
    (void)hipStreamSynchronize(g->s_d2h);
    for (auto& s : g->slots) s.b0 = -1;
    g_err = err;
}

// both slots for micro-batches of nb frames of `in` source bytes each; capacities are kept in bytes, as og_classic's
int gated_ensure(og_gated* g, int nb, size_t in, size_t mask1) {
    const size_t inb = (size_t)nb * in, mb = (size_t)nb * mask1;
    if ((size_t)nb <= g->cap_nb && inb <= g->cap_in && mb <= g->cap_mask) return OG_OK;
    gated_drain(g);
    const size_t n = std::max((size_t)nb, g->cap_nb), i = std::max(inb, g->cap_in), m = std::max(mb, g->cap_mask);
    gated_free_slots(g);
    hipError_t e = hipSuccess;
    auto dev = [&](void** q, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc(q, bytes ? bytes : 1);
    };
    auto host = [&](void** q, size_t bytes) {
        if (e == hipSuccess) e = hipHostMalloc(q, bytes ? bytes : 1, hipHostMallocDefault);
    };
    for (auto& s : g->slots) {
        dev((void**)&s.d_in, i);
        host((void**)&s.h_in, i);
        if (m) {
            dev((void**)&s.d_mask, m);
            host((void**)&s.h_mask, m);
        }
        dev((void**)&s.d_resets, n);
        host((void**)&s.h_resets, n);
        dev((void**)&s.d_best, n * 20);
        host((void**)&s.h_best, n * 20);
        dev((void**)&s.d_boxes, n * 16);
        host((void**)&s.h_boxes, n * 16);
        dev((void**)&s.d_area, n * 4);
        host((void**)&s.h_area, n * 4);
    }
    if (e != hipSuccess) {
        gated_free_slots(g);
        return fail(e == hipErrorOutOfMemory ? OG_ENOMEM : OG_EHIP, std::string("gated engine slots: ") + hipGetErrorString(e));
    }
    g->cap_nb = n;
    g->cap_in = i;
    g->cap_mask = m;
    return OG_OK;
}

int gated_track_launch(og_gated* g, const float* best, const uint8_t* resets, int B, int W, int H, int32_t* boxes) {
    OG_LAUNCH(k_track_boxes, dim3(1), dim3(256), 0, g->yolo->stream, best, resets, B, W, H, g->params.max_shift, g->params.padding,
              g->params.max_hold, g->d_state, boxes);
    return OG_OK;
}

int gated_stream_impl(og_gated* g, const uint8_t* frames, const uint8_t* const* frame_ptrs, int B, int H, int W, int ch, int imgsz, int Hn,
                      int Wn, float conf, float thr, const uint8_t* resets, int32_t* area, int32_t* boxes, float* best, uint8_t* mask,
                      bool kept = false, int32_t* n_kept = nullptr) {
    int rc = check_gated_shape(B, H, W, ch);   // (the checks that need no handle come first: they can be tested without a device)
    if (rc) return rc;
    OG_ALIGN(frame_ptrs);
    OG_ALIGN(area);
    OG_ALIGN(boxes);
    OG_ALIGN(best);
    OG_ALIGN(n_kept);
    if (!g) return fail(OG_EINVAL, "null handle");
    if (!g->unet->finalized || !g->yolo->finalized) return fail(OG_ESTATE, "a borrowed handle is not finalized");
    YGeo geo;
    if ((rc = y_check_resized(g->yolo, B, H, W, ch, imgsz, geo))) return rc;
    if ((rc = check_resized(g->unet, B, H, W, ch, Hn, Wn))) return rc;
    if (g->yolo->pend_B) return fail(OG_EINVAL, "a begin / end call is in flight on the detector handle");
    if (B == 0) {
        if (n_kept) *n_kept = 0;
        return OG_OK;
    }
    if (!frames && !frame_ptrs) return fail(OG_EINVAL, "frames is null");
    if (!area) return fail(OG_EINVAL, "area is null");
    if (frame_ptrs)
        for (int i = 0; i < B; ++i)
            if (!frame_ptrs[i]) return fail(OG_EINVAL, "frame_ptrs[" + std::to_string(i) + "] is null");
    OG_SCOPE(g);
    const size_t HW = (size_t)H * W, fb = HW * ch;
    const int chunk = gated_cap(H, W, ch, g->stage_kib);
    if ((rc = gated_ensure(g, chunk, fb, mask ? HW : 0))) return rc;
    if (kept)
        for (int i = 0; i < 2; ++i)
            if ((rc = gate_ensure(g, g->gate[i], chunk, fb, mask ? HW : 0))) return rc;
    long long total_kept = 0;
    const bool pinned = frames != nullptr && is_pinned_host(frames);
    const hipStream_t sy = g->yolo->stream, su = g->unet->stream;

    auto retire = [&](og_gated::Slot& s) -> int {
        if (s.b0 < 0) return OG_OK;
        const int b0 = s.b0, nb = s.nb;
        s.b0 = -1;
        HIPCHK(hipEventSynchronize(s.ev_out));
        memcpy(area + b0, s.h_area, (size_t)nb * 4);
        if (boxes) memcpy(boxes + 4 * (size_t)b0, s.h_boxes, (size_t)nb * 16);
        if (best) memcpy(best + 5 * (size_t)b0, s.h_best, (size_t)nb * 20);
        if (mask) memcpy(mask + b0 * HW, s.h_mask, nb * HW);
        return OG_OK;
    };
    auto fill = [&](og_gated::Slot& s, int b0, int nb) -> int {
        og_gated::Gate& k = g->gate[&s - g->slots];   // the slot's own dense buffers
        const uint8_t* src = frames ? frames + (size_t)b0 * fb : s.h_in;
        if (frame_ptrs) {
            for (int j = 0; j < nb; ++j) memcpy(s.h_in + (size_t)j * fb, frame_ptrs[b0 + j], fb);
        } else if (!pinned) {   // pageable memory: through the slot's pinned buffer, so that the copy up is asynchronous
            memcpy(s.h_in, src, nb * fb);
            src = s.h_in;
        }
        HIPCHK(hipMemcpyAsync(s.d_in, src, nb * fb, hipMemcpyHostToDevice, g->s_h2d));
        if (resets) {
            memcpy(s.h_resets, resets + b0, (size_t)nb);
            HIPCHK(hipMemcpyAsync(s.d_resets, s.h_resets, (size_t)nb, hipMemcpyHostToDevice, g->s_h2d));
        }
        HIPCHK(hipEventRecord(s.ev_up, g->s_h2d));
        HIPCHK(hipStreamWaitEvent(sy, s.ev_up, 0));
        // always the batched kernels, also for a micro-batch of one frame: a frame's `best` row must not depend on where stage_kib
        // cuts the video (the one-frame latency kernels sum in another order; "latency_batch" 0 is the same decision)
        const int lb = g->yolo->latency_batch;
        g->yolo->latency_batch = 0;
        int rc2 = og_yolo_detect_resized_u8_dev(g->yolo, s.d_in, nb, H, W, ch, imgsz, conf, s.d_best);
        g->yolo->latency_batch = lb;
        if (!rc2) rc2 = gated_track_launch(g, s.d_best, resets ? s.d_resets : nullptr, nb, W, H, s.d_boxes);
        if (rc2) return rc2;
        if (kept) {   // select and the count's copy ride the detector's stream; the host waits for the count (the U-Net pass of the
                      // micro-batch before this one is already enqueued), then enqueues gather, network and scatter on the U-Net's
            if ((rc2 = gate_select_enqueue(g, k, s.d_boxes, nb, sy))) return rc2;
            int n = 0;
            if ((rc2 = gate_segment_enqueue(g, k, s.d_in, nb, H, W, ch, Hn, Wn, thr, s.d_boxes, mask ? s.d_mask : nullptr, s.d_area, &n)))
                return rc2;
            total_kept += n;
        } else {
            HIPCHK(hipEventRecord(s.ev_det, sy));
            HIPCHK(hipStreamWaitEvent(su, s.ev_det, 0));
            if ((rc2 = og_unet_segment_resized_u8_dev(g->unet, s.d_in, nb, H, W, ch, Hn, Wn, thr, s.d_boxes, mask ? s.d_mask : nullptr,
                                                      s.d_area, nullptr, nullptr, nullptr)))
                return rc2;
        }
        HIPCHK(hipEventRecord(s.ev_seg, su));
        HIPCHK(hipStreamWaitEvent(g->s_d2h, s.ev_seg, 0));
        HIPCHK(hipMemcpyAsync(s.h_area, s.d_area, (size_t)nb * 4, hipMemcpyDeviceToHost, g->s_d2h));
        if (boxes) HIPCHK(hipMemcpyAsync(s.h_boxes, s.d_boxes, (size_t)nb * 16, hipMemcpyDeviceToHost, g->s_d2h));
        if (best) HIPCHK(hipMemcpyAsync(s.h_best, s.d_best, (size_t)nb * 20, hipMemcpyDeviceToHost, g->s_d2h));
        if (mask) HIPCHK(hipMemcpyAsync(s.h_mask, s.d_mask, nb * HW, hipMemcpyDeviceToHost, g->s_d2h));
        HIPCHK(hipEventRecord(s.ev_out, g->s_d2h));
        s.b0 = b0;
        s.nb = nb;
        return OG_OK;
    };

    rc = og_two_slot(B, chunk, g->slots, retire, fill, [] {});
    gated_drain(g);   // a caller-pinned source may still be read by a copy whose micro-batch failed later; cheap when all is done
    if (rc) return rc;
    if (n_kept) *n_kept = (int32_t)total_kept;
    if ((rc = y_check_range(g->yolo))) return rc;
    return check_range(g->unet);
}

}  // namespace

extern "C" {

int og_track_host(og_track_state* state_inout, const og_track_params* params, const float* best, const uint8_t* resets_or_null, int B,
                  int W, int H, int32_t* boxes_out) {
    if (!state_inout) return fail(OG_EINVAL, "state is null");
    OG_ALIGN(state_inout);
    OG_ALIGN(params);
    OG_ALIGN(best);
    OG_ALIGN(boxes_out);
    int rc = check_track_params(params);
    if (rc) return rc;
    if (B < 0 || W <= 0 || H <= 0) return fail(OG_EINVAL, "bad B/W/H");
    if (B == 0) return OG_OK;
    if (!best || !boxes_out) return fail(OG_EINVAL, "null buffer");
    OgTrackState s;
    memcpy(&s, state_inout, sizeof s);
    const OgTrackParams p{params->max_shift_px, params->padding, params->max_hold_frames};
    for (int i = 0; i < B; ++i) {
        if (resets_or_null && resets_or_null[i]) s = OgTrackState{0.f, 0.f, 0, 0, 0, 0};
        int box[4];
        og_track_step(s, best + 5 * (size_t)i, W, H, p, box);
        for (int k = 0; k < 4; ++k) boxes_out[4 * (size_t)i + k] = box[k];
    }
    memcpy(state_inout, &s, sizeof s);
    return OG_OK;
}

int og_gated_plan(int B, int H, int W, int channels, int stage_kib, char* out, size_t cap, long long* engine_bytes) {
    if (!out || cap == 0 || B < 1) return fail(OG_EINVAL, "bad argument");
    OG_ALIGN(engine_bytes);
    int rc = check_gated_shape(B, H, W, channels);
    if (rc) return rc;
    if (stage_kib < 1 || stage_kib > kGatedMaxStageKib) return fail(OG_EINVAL, "stage_kib must be 1.." + std::to_string(kGatedMaxStageKib));
    const int mb = gated_cap(H, W, channels, stage_kib);
    std::string txt;
    int n = 0;
    for (int b0 = 0; b0 < B; b0 += mb, ++n) txt += std::to_string(b0) + "|" + std::to_string(B - b0 < mb ? B - b0 : mb) + "\n";
    if (txt.size() + 1 > cap) return fail(OG_EINVAL, "plan text does not fit the buffer");
    memcpy(out, txt.c_str(), txt.size() + 1);
    if (engine_bytes) *engine_bytes = gated_engine_bytes(mb, H, W, channels, true);
    return n;
}

og_gated* og_gated_create(og_unet* unet, og_yolo* yolo) {
    if (!unet || !yolo) {
        fail(OG_EINVAL, "null handle");
        return nullptr;
    }
    if (!unet->finalized || !yolo->finalized || unet->host_only || yolo->host_only || !unet->stream || !yolo->stream) {
        fail(OG_ESTATE, "both handles must be finalized");
        return nullptr;
    }
    if (unet->device != yolo->device) {
        fail(OG_EINVAL, "the U-Net and the detector live on different devices");
        return nullptr;
    }
    og_gated* g = new og_gated();
    g->unet = unet;
    g->yolo = yolo;
    g->device = unet->device;
    DeviceGuard dg(g->device, false);
    hipError_t e = dg.err;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&g->s_h2d, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&g->s_d2h, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&g->d_state, sizeof(OgTrackState));
    if (e == hipSuccess) e = hipMemset(g->d_state, 0, sizeof(OgTrackState));
    for (auto& s : g->slots)
        for (hipEvent_t* ev : {&s.ev_up, &s.ev_det, &s.ev_seg, &s.ev_out})
            if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        fail(OG_EHIP, std::string("og_gated_create: ") + hipGetErrorString(e));
        g->ready = true;   // (release whatever exists)
        og_gated_destroy(g);
        return nullptr;
    }
    g->ready = true;
    return g;
}

void og_gated_destroy(og_gated* g) {
    if (!g) return;
    DeviceGuard dg_(g->device, og_skip_device(g));
    const std::string err = g_err;
    if (g->s_h2d) (void)hipStreamSynchronize(g->s_h2d);
    if (g->s_d2h) (void)hipStreamSynchronize(g->s_d2h);
    gated_free_slots(g);
    gate_free(g);
    for (auto& s : g->slots)
        for (hipEvent_t ev : {s.ev_up, s.ev_det, s.ev_seg, s.ev_out})
            if (ev) (void)hipEventDestroy(ev);
    if (g->d_state) (void)hipFree(g->d_state);   // (waits for the device: no launch of the borrowed streams still reads it)
    if (g->s_h2d) (void)hipStreamDestroy(g->s_h2d);
    if (g->s_d2h) (void)hipStreamDestroy(g->s_d2h);
    g_err = err;
    delete g;
}

int og_gated_sync(og_gated* g) {
    if (!g) return fail(OG_EINVAL, "null handle");
    OG_SCOPE(g);
    HIPCHK(hipStreamSynchronize(g->s_h2d));
    HIPCHK(hipStreamSynchronize(g->yolo->stream));
    HIPCHK(hipStreamSynchronize(g->unet->stream));
    HIPCHK(hipStreamSynchronize(g->s_d2h));
    const int rc = y_check_range(g->yolo);
    return rc ? rc : check_range(g->unet);
}

int og_gated_set_option(og_gated* g, const char* name, int value) {
    if (!g || !name) return fail(OG_EINVAL, "null argument");
    if (std::string(name) == "stage_kib" && value >= 1 && value <= kGatedMaxStageKib) {
        g->stage_kib = value;
        return OG_OK;
    }
    return fail(OG_EINVAL, std::string("og_gated_set_option: unknown option or value out of range: ") + name);
}

int og_gated_reset(og_gated* g) {
    if (!g) return fail(OG_EINVAL, "null handle");
    OG_SCOPE(g);
    HIPCHK(hipMemsetAsync(g->d_state, 0, sizeof(OgTrackState), g->yolo->stream));
    return OG_OK;
}

int og_gated_set_params(og_gated* g, const og_track_params* params) {
    if (!g) return fail(OG_EINVAL, "null handle");
    OG_ALIGN(params);
    const int rc = check_track_params(params);
    if (rc) return rc;
    g->params = OgTrackParams{params->max_shift_px, params->padding, params->max_hold_frames};
    return OG_OK;
}

int og_gated_get_state(og_gated* g, og_track_state* state) {
    if (!g || !state) return fail(OG_EINVAL, "null argument");
    OG_ALIGN(state);
    OG_SCOPE(g);
    HIPCHK(hipStreamSynchronize(g->yolo->stream));
    HIPCHK(hipMemcpy(state, g->d_state, sizeof(OgTrackState), hipMemcpyDeviceToHost));
    return OG_OK;
}

int og_gated_set_state(og_gated* g, const og_track_state* state) {
    if (!g || !state) return fail(OG_EINVAL, "null argument");
    OG_ALIGN(state);
    OgTrackState s;
    memcpy(&s, state, sizeof s);
    if (!s.has) s = OgTrackState{0.f, 0.f, 0, 0, 0, 0};
    s.has = s.has ? 1 : 0;
    OG_SCOPE(g);
    HIPCHK(hipStreamSynchronize(g->yolo->stream));   // ordered after the work enqueued; the copy below reads host memory of this call
    HIPCHK(hipMemcpy(g->d_state, &s, sizeof s, hipMemcpyHostToDevice));
    return OG_OK;
}

int og_track_boxes_dev(og_gated* g, const float* best_dev, const uint8_t* resets_dev_or_null, int B, int W, int H, int32_t* boxes_dev) {
    if (!g) return fail(OG_EINVAL, "null handle");
    if (B < 0 || W <= 0 || H <= 0) return fail(OG_EINVAL, "bad B/W/H");
    OG_ALIGN(best_dev);
    OG_ALIGN(boxes_dev);
    if (B == 0) return OG_OK;
    if (!best_dev || !boxes_dev) return fail(OG_EINVAL, "null buffer");
    OG_SCOPE(g);
    return gated_track_launch(g, best_dev, resets_dev_or_null, B, W, H, boxes_dev);
}

int og_gated_stream_u8(og_gated* g, const uint8_t* frames, int B, int H, int W, int channels, int imgsz, int net_h, int net_w, float conf,
                       float threshold, const uint8_t* resets_or_null, int32_t* area, int32_t* boxes_or_null, float* best_or_null,
                       uint8_t* mask_or_null) {
    return gated_stream_impl(g, frames, nullptr, B, H, W, channels, imgsz, net_h, net_w, conf, threshold, resets_or_null, area, boxes_or_null,
                             best_or_null, mask_or_null);
}

int og_gated_stream_frames_u8(og_gated* g, const uint8_t* const* frame_ptrs, int B, int H, int W, int channels, int imgsz, int net_h,
                              int net_w, float conf, float threshold, const uint8_t* resets_or_null, int32_t* area,
                              int32_t* boxes_or_null, float* best_or_null, uint8_t* mask_or_null) {
    if (!frame_ptrs && B > 0) return fail(OG_EINVAL, "frame_ptrs is null");
    return gated_stream_impl(g, nullptr, frame_ptrs, B, H, W, channels, imgsz, net_h, net_w, conf, threshold, resets_or_null, area,
                             boxes_or_null, best_or_null, mask_or_null);
}

}  // extern "C"
