// Host plumbing shared by the streaming families (og_classic, og_overlay, og_sweep, og_mjpeg, og_mjpd) and by every plan entry.
// Included by og_api.hip after fail, HIPCHK, OG_SCOPE and Plan, before the first family.  No kernels, no extern "C" entry.
// A family keeps what is its own: its checks, its batch function (the launches of one micro-batch), and the retire / fill lambdas
// of its streamed entry.  DESIGN.md, "Shared host plumbing of the streaming families", says what a new family reuses.

// what every streaming handle begins with: one stream on one device, made by the first call that needs it
struct OgStreamHandle {
    int device = -1;
    bool ready = false;   // the stream exists
    hipStream_t stream = nullptr;
    int chunk = 128;
};
inline bool og_skip_device(const OgStreamHandle* h) { return !h || !h->ready; }

namespace {

int og_stream_ready(OgStreamHandle* h) {
    if (h->ready) return OG_OK;
    HIPCHK(hipGetDevice(&h->device));
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->ready = true;
    return OG_OK;
}

// after a failed call: wait for everything in flight, keep the message
void og_stream_drain(OgStreamHandle* h) {
    const std::string err = g_err;
    if (h->ready) (void)hipStreamSynchronize(h->stream);
    g_err = err;
}

int og_stream_sync(OgStreamHandle* h) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (!h->ready) return OG_OK;
    OG_SCOPE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    return OG_OK;
}

// free_all: the family's buffers and events; it runs on the handle's device, after the stream has drained
template <class H, class F>
void og_stream_destroy(H* h, F free_all) {
    if (!h) return;
    DeviceGuard dg_(h->device, og_skip_device(h));
    if (h->ready) {
        (void)hipStreamSynchronize(h->stream);
        free_all();
        (void)hipStreamDestroy(h->stream);
    }
    delete h;
}

int og_check_chunk(int chunk, int max, bool zero_is_default = false) {
    if (chunk < (zero_is_default ? 0 : 1) || chunk > max)
        return fail(OG_EINVAL, "chunk must be 1.." + std::to_string(max) + (zero_is_default ? ", or 0 for the default" : ""));
    return OG_OK;
}

int og_stream_set_chunk(OgStreamHandle* h, int chunk, int max, bool zero_is_default = false) {
    if (!h) return fail(OG_EINVAL, "null handle");
    const int rc = og_check_chunk(chunk, max, zero_is_default);
    if (rc) return rc;
    h->chunk = chunk;
    return OG_OK;
}

// One buffer of a handle, device or pinned host memory, with its capacity in bytes.  Reads as the pointer it holds.  Freed by
// release() only, never by a destructor: the family's free function runs under the handle's DeviceGuard (og_stream_destroy).
template <class T>
struct OgBuf {
    T* p = nullptr;
    size_t cap = 0;
    bool pinned = false;
    explicit OgBuf(bool pinned_host = false) : pinned(pinned_host) {}
    operator T*() const { return p; }

    // grow to `need` bytes (never shrink); what it held is dropped, so the stream is drained first
    int grow(OgStreamHandle* h, size_t need, const char* family) {
        if (need <= cap && p) return OG_OK;
        HIPCHK(hipStreamSynchronize(h->stream));
        release();
        const size_t bytes = need ? need : 1;
        const hipError_t e = pinned ? hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) : hipMalloc((void**)&p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(e == hipErrorOutOfMemory ? OG_ENOMEM : OG_EHIP, std::string(family) + " workspace: " + hipGetErrorString(e));
        }
        cap = bytes;
        return OG_OK;
    }
    void release() {
        if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
};

template <class... Bufs>
void og_release(Bufs&... bufs) {
    (bufs.release(), ...);
}

// The streamed entries' pipeline: micro-batch k goes through slot k & 1, whose previous micro-batch (k - 2) is retired first, so
// the host fills one slot while the device works on the other.  retire(slot) delivers a slot's results (nothing if it is free,
// b0 < 0); fill(slot, b0, nb) stages, enqueues and records the slot's event `ev`; drain() runs after an error.
template <class Slot, class Retire, class Fill, class Drain>
int og_two_slot(int B, int chunk, Slot (&slots)[2], Retire retire, Fill fill, Drain drain) {
    int rc = OG_OK, k = 0;
    for (int b0 = 0; b0 < B && !rc; b0 += chunk, ++k) {
        Slot& s = slots[k & 1];
        if ((rc = retire(s))) break;   // micro-batch k - 2 is complete and delivered: its pinned buffers are free
        rc = fill(s, b0, (B - b0 < chunk) ? B - b0 : chunk);
    }
    for (int i = 0; i < 2; ++i) {   // in age order; on an error still wait for what is in flight
        const int rc2 = retire(slots[(k + i) & 1]);
        if (!rc) rc = rc2;
    }
    if (rc) {
        for (Slot& s : slots) s.b0 = -1;
        drain();
    }
    return rc;
}

// The text of a dry run, one line per recorded launch: kernel|gx|gy|gz|block|lds|partial|counters and a last column.
enum OgPlanLast {
    kPlanNoLast,   // og_unet_plan: eight columns
    kPlanWrites,   // "buffer=end;..." of the caller-owned buffers the launch writes, "-" if none
    kPlanMod,      // og_yolo_plan: the module path the launch serves
};
int og_plan_text(const Plan& plan, OgPlanLast last, char* out, size_t cap) {
    std::string txt;
    txt.reserve(plan.recs.size() * 96);
    for (const PlanRec& r : plan.recs) {
        txt += r.kernel + "|" + std::to_string(r.gx) + "|" + std::to_string(r.gy) + "|" + std::to_string(r.gz) + "|" + std::to_string(r.block) + "|" +
               std::to_string(r.lds) + "|" + std::to_string(r.partial_bytes) + "|" + std::to_string(r.counters);
        if (last == kPlanWrites) txt += "|" + (r.writes.empty() ? std::string("-") : r.writes);
        if (last == kPlanMod) txt += "|" + r.mod;
        txt += "\n";
    }
    if (txt.size() + 1 > cap) return fail(OG_EINVAL, "plan text does not fit the buffer");
    memcpy(out, txt.c_str(), txt.size() + 1);
    return (int)plan.recs.size();
}

}  // namespace
