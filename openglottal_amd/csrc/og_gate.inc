// The gated pipeline with the U-Net run only on the frames the tracker kept (include/openglottal_hip_gate.h, DESIGN.md section
// 21).  Included by og_api.hip after og_gated.inc, whose handle and stream loop it extends.  Three kernels, all plain C++:
//   k_gate_select    one workgroup: the kept frames' indices, ascending, and their number
//   k_gate_gather    dst row j = src row keep[j]
//   k_gate_scatter   dst row keep[j] = src row j, every other row zero
// and the step that puts them around the unchanged og_unet_segment_resized_u8_dev (gate_segment_enqueue).
#include "../../include/openglottal_hip_gate.h"

// ONE workgroup, as k_track_boxes.  Per block of 256 frames: a lane per frame takes its flag (og_gate_keeps), an inclusive
// Hillis-Steele scan over LDS gives every kept frame its rank inside the block, and `base` -- the same value in every lane, advanced
// by the block's total -- its place in keep.  Stable: ranks grow with the frame index, blocks come in order.
__global__ __launch_bounds__(256) void k_gate_select(const int32_t* __restrict__ boxes, int B, int32_t* __restrict__ keep,
                                                     int32_t* __restrict__ count) {
    __shared__ int s_scan[256];
    const int tid = threadIdx.x;
    int base = 0;
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int i = b0 + tid;
        const int flag = (i < B && og_gate_keeps(boxes + 4 * (long long)i)) ? 1 : 0;
        s_scan[tid] = flag;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int v = tid >= o ? s_scan[tid - o] : 0;
            __syncthreads();
            s_scan[tid] += v;
            __syncthreads();
        }
        if (flag) keep[base + s_scan[tid] - 1] = i;
        base += s_scan[255];
        __syncthreads();   // (the next block's flags overwrite what every lane has just read)
    }
    if (tid == 0) *count = base;
}

// grid (x, y): block y takes rows y, y + gridDim.y, ...; within a row the x blocks stride over 16-byte units (vec16: row_bytes
// and both bases are multiples of 16) or over bytes.  All offsets are 64-bit.
__device__ inline void og_gate_copy_row(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, long long row_bytes, int vec16) {
    const long long step = (long long)gridDim.x * 256, first = (long long)blockIdx.x * 256 + threadIdx.x;
    if (vec16) {
        const long long units = row_bytes >> 4;
        const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(s);
        uint4* __restrict__ d4 = reinterpret_cast<uint4*>(d);
        for (long long u = first; u < units; u += step) d4[u] = s4[u];
    } else {
        for (long long u = first; u < row_bytes; u += step) d[u] = s[u];
    }
}

__global__ __launch_bounds__(256) void k_gate_gather(const uint8_t* __restrict__ src, long long row_bytes, const int32_t* __restrict__ keep,
                                                     int n, int vec16, uint8_t* __restrict__ dst) {
    for (long long j = blockIdx.y; j < n; j += gridDim.y) og_gate_copy_row(src + (long long)keep[j] * row_bytes, dst + j * row_bytes, row_bytes, vec16);
}

// Block y owns destination rows y, y + gridDim.y, ... of all B: a binary search of the ascending keep list says whether row r is
// keep[j] for some j -- then it is src row j -- or a row that nobody kept, which is zero-filled here.  Every destination byte is
// written exactly once, by this launch.
__global__ __launch_bounds__(256) void k_gate_scatter(const uint8_t* __restrict__ src, long long row_bytes, const int32_t* __restrict__ keep,
                                                      int n, int B, int vec16, uint8_t* __restrict__ dst) {
    for (long long r = blockIdx.y; r < B; r += gridDim.y) {
        int lo = 0, hi = n;   // first j with keep[j] >= r
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (keep[mid] < r) lo = mid + 1;
            else hi = mid;
        }
        uint8_t* __restrict__ d = dst + r * row_bytes;
        if (lo < n && keep[lo] == r) {
            og_gate_copy_row(src + (long long)lo * row_bytes, d, row_bytes, vec16);
        } else {
            const long long step = (long long)gridDim.x * 256, first = (long long)blockIdx.x * 256 + threadIdx.x;
            if (vec16) {
                uint4* __restrict__ d4 = reinterpret_cast<uint4*>(d);
                for (long long u = first; u < (row_bytes >> 4); u += step) d4[u] = make_uint4(0u, 0u, 0u, 0u);
            } else {
                for (long long u = first; u < row_bytes; u += step) d[u] = 0;
            }
        }
    }
}

namespace {

constexpr int kGateMaxRows = 1 << 20;
constexpr long long kGateMaxRowBytes = (long long)kResizeMaxSide * kResizeMaxSide * 3;
constexpr int kGateGridBlocks = 2048;   // of 256 lanes per launch; the rest is grid-strided

// the header's MEMORY formula: what the kept entries add per slot, on the device
long long gate_slot_bytes(int nb, int H, int W, int ch, bool with_mask) {
    return (long long)nb * ((long long)H * W * (ch + (with_mask ? 1 : 0)) + 24) + 4;
}

int check_gate_rows(size_t row_bytes, int n, int B) {
    if (row_bytes < 1 || row_bytes > (size_t)kGateMaxRowBytes) return fail(OG_EINVAL, "row_bytes must be 1.." + std::to_string(kGateMaxRowBytes));
    if (B < 0 || B > kGateMaxRows) return fail(OG_EINVAL, "B must be 0.." + std::to_string(kGateMaxRows));
    if (n < 0 || n > B) return fail(OG_EINVAL, "n must be 0..B");
    return OG_OK;
}

// y: a block per row, x: what is left of kGateGridBlocks, at most what the row needs
dim3 gate_grid(long long rows, long long row_bytes, int vec16) {
    const long long gy = rows < kGateGridBlocks ? rows : kGateGridBlocks;
    const long long units = vec16 ? row_bytes >> 4 : row_bytes, need = (units + 255) / 256, room = kGateGridBlocks / gy;
    const long long gx = need < room ? need : room;
    return dim3((unsigned)(gx < 1 ? 1 : gx), (unsigned)gy);
}

inline int gate_vec16(const void* a, const void* b, size_t row_bytes) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)row_bytes) & 15) == 0 ? 1 : 0;
}

int gate_gather_launch(hipStream_t st, const uint8_t* src, size_t row_bytes, const int32_t* keep, int n, uint8_t* dst) {
    if (n == 0) return OG_OK;
    const int v = gate_vec16(src, dst, row_bytes);
    OG_LAUNCH(k_gate_gather, gate_grid(n, (long long)row_bytes, v), dim3(256), 0, st, src, (long long)row_bytes, keep, n, v, dst);
    return OG_OK;
}

int gate_scatter_launch(hipStream_t st, const uint8_t* src, size_t row_bytes, const int32_t* keep, int n, int B, uint8_t* dst) {
    if (B == 0) return OG_OK;
    const int v = gate_vec16(src, dst, row_bytes);
    OG_LAUNCH(k_gate_scatter, gate_grid(B, (long long)row_bytes, v), dim3(256), 0, st, src, (long long)row_bytes, keep, n, B, v, dst);
    return OG_OK;
}

void gate_release(og_gated::Gate& k) {
    void* dev[] = {k.d_dense, k.d_mask, k.d_keep, k.d_boxes, k.d_area, k.d_count};
    for (void* p : dev)
        if (p) (void)hipFree(p);
    if (k.h_count) (void)hipHostFree(k.h_count);
    k.d_dense = k.d_mask = nullptr;
    k.d_keep = k.d_boxes = k.d_area = k.d_count = k.h_count = nullptr;
    k.cap_n = k.cap_in = k.cap_mask = 0;
}

void gate_free(og_gated* g) {
    for (auto& k : g->gate) {
        gate_release(k);
        if (k.ev_cnt) (void)hipEventDestroy(k.ev_cnt);
        k.ev_cnt = nullptr;
    }
}

// one set of dense buffers for nb frames of `in` source bytes (and mask1 mask bytes) each; never shrinks
int gate_ensure(og_gated* g, og_gated::Gate& k, int nb, size_t in, size_t mask1) {
    const size_t inb = (size_t)nb * in, mb = (size_t)nb * mask1;
    if (k.ev_cnt && (size_t)nb <= k.cap_n && inb <= k.cap_in && mb <= k.cap_mask) return OG_OK;
    gated_drain(g);
    const size_t n = std::max((size_t)nb, k.cap_n), i = std::max(inb, k.cap_in), m = std::max(mb, k.cap_mask);
    gate_release(k);
    hipError_t e = hipSuccess;
    if (!k.ev_cnt) e = hipEventCreateWithFlags(&k.ev_cnt, hipEventDisableTiming);
    auto dev = [&](void** q, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc(q, bytes ? bytes : 1);
    };
    dev((void**)&k.d_dense, i);
    if (m) dev((void**)&k.d_mask, m);
    dev((void**)&k.d_keep, n * 4);
    dev((void**)&k.d_boxes, n * 16);
    dev((void**)&k.d_area, n * 4);
    dev((void**)&k.d_count, 4);
    if (e == hipSuccess) e = hipHostMalloc((void**)&k.h_count, 4, hipHostMallocDefault);
    if (e != hipSuccess) {
        gate_release(k);
        return fail(e == hipErrorOutOfMemory ? OG_ENOMEM : OG_EHIP, std::string("gate buffers: ") + hipGetErrorString(e));
    }
    k.cap_n = n;
    k.cap_in = i;
    k.cap_mask = m;
    return OG_OK;
}

// on `st`: select, the count to the pinned word, the event the host will wait for
int gate_select_enqueue(og_gated* g, og_gated::Gate& k, const int32_t* boxes, int B, hipStream_t st) {
    (void)g;
    OG_LAUNCH(k_gate_select, dim3(1), dim3(256), 0, st, boxes, B, k.d_keep, k.d_count);
    HIPCHK(hipMemcpyAsync(k.h_count, k.d_count, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(k.ev_cnt, st));
    return OG_OK;
}

// the host's one wait (the count), then on the U-Net's stream, ordered after the select: the network on the kept frames only
int gate_segment_enqueue(og_gated* g, og_gated::Gate& k, const uint8_t* src, int B, int H, int W, int ch, int Hn, int Wn, float thr,
                         const int32_t* boxes, uint8_t* mask, int32_t* area, int* n_out) {
    const hipStream_t su = g->unet->stream;
    HIPCHK(hipEventSynchronize(k.ev_cnt));
    const int n = *k.h_count;
    if (n < 0 || n > B) return fail(OG_EHIP, "k_gate_select left a count outside 0..B");
    HIPCHK(hipStreamWaitEvent(su, k.ev_cnt, 0));
    const size_t HW = (size_t)H * W, fb = HW * ch;
    int rc = OG_OK;
    if (n == B) {
        rc = og_unet_segment_resized_u8_dev(g->unet, src, B, H, W, ch, Hn, Wn, thr, boxes, mask, area, nullptr, nullptr, nullptr);
    } else if (n == 0) {
        HIPCHK(hipMemsetAsync(area, 0, (size_t)B * 4, su));
        if (mask) HIPCHK(hipMemsetAsync(mask, 0, B * HW, su));
    } else {
        if ((rc = gate_gather_launch(su, src, fb, k.d_keep, n, k.d_dense))) return rc;
        if ((rc = gate_gather_launch(su, (const uint8_t*)boxes, 16, k.d_keep, n, (uint8_t*)k.d_boxes))) return rc;
        if ((rc = og_unet_segment_resized_u8_dev(g->unet, k.d_dense, n, H, W, ch, Hn, Wn, thr, k.d_boxes, mask ? k.d_mask : nullptr, k.d_area,
                                                 nullptr, nullptr, nullptr)))
            return rc;
        if ((rc = gate_scatter_launch(su, (const uint8_t*)k.d_area, 4, k.d_keep, n, B, (uint8_t*)area))) return rc;
        if (mask) rc = gate_scatter_launch(su, k.d_mask, HW, k.d_keep, n, B, mask);
    }
    if (!rc && n_out) *n_out = n;
    return rc;
}

}  // namespace

extern "C" {

int og_gate_select_host(const int32_t* boxes, int B, int32_t* keep_out) {
    if (B < 0 || B > kGateMaxRows) return fail(OG_EINVAL, "B must be 0.." + std::to_string(kGateMaxRows));
    OG_ALIGN(boxes);
    OG_ALIGN(keep_out);
    if (B == 0) return 0;
    if (!boxes || !keep_out) return fail(OG_EINVAL, "null buffer");
    int n = 0;
    for (int i = 0; i < B; ++i)
        if (og_gate_keeps(boxes + 4 * (size_t)i)) keep_out[n++] = i;
    return n;
}

int og_gate_select_dev(og_gated* g, const int32_t* boxes_dev, int B, int32_t* keep_dev, int32_t* count_dev) {
    if (B < 0 || B > kGateMaxRows) return fail(OG_EINVAL, "B must be 0.." + std::to_string(kGateMaxRows));
    OG_ALIGN(boxes_dev);
    OG_ALIGN(keep_dev);
    OG_ALIGN(count_dev);
    if (!count_dev || (B > 0 && (!boxes_dev || !keep_dev))) return fail(OG_EINVAL, "null buffer");
    if (!g) return fail(OG_EINVAL, "null handle");
    OG_SCOPE(g);
    OG_LAUNCH(k_gate_select, dim3(1), dim3(256), 0, g->yolo->stream, boxes_dev, B, keep_dev, count_dev);
    return OG_OK;
}

int og_gate_gather_dev(og_gated* g, const uint8_t* src_dev, size_t row_bytes, const int32_t* keep_dev, int n, uint8_t* dst_dev) {
    int rc = check_gate_rows(row_bytes, n, kGateMaxRows);
    if (rc) return rc;
    OG_ALIGN(keep_dev);
    if (n > 0 && (!src_dev || !keep_dev || !dst_dev)) return fail(OG_EINVAL, "null buffer");
    if (!g) return fail(OG_EINVAL, "null handle");
    OG_SCOPE(g);
    return gate_gather_launch(g->unet->stream, src_dev, row_bytes, keep_dev, n, dst_dev);
}

int og_gate_scatter_dev(og_gated* g, const uint8_t* src_dev, size_t row_bytes, const int32_t* keep_dev, int n, int B, uint8_t* dst_dev) {
    int rc = check_gate_rows(row_bytes, n, B);
    if (rc) return rc;
    OG_ALIGN(keep_dev);
    if ((n > 0 && (!src_dev || !keep_dev)) || (B > 0 && !dst_dev)) return fail(OG_EINVAL, "null buffer");
    if (!g) return fail(OG_EINVAL, "null handle");
    OG_SCOPE(g);
    return gate_scatter_launch(g->unet->stream, src_dev, row_bytes, keep_dev, n, B, dst_dev);
}

int og_gated_segment_kept_dev(og_gated* g, const uint8_t* src_dev, int B, int H, int W, int channels, int net_h, int net_w, float threshold,
                              const int32_t* boxes_dev, uint8_t* mask_dev_or_null, int32_t* area_dev, int32_t* n_kept_out) {
    int rc = check_gated_shape(B, H, W, channels);
    if (rc) return rc;
    if (B > kGateMaxRows) return fail(OG_EINVAL, "B must be 0.." + std::to_string(kGateMaxRows));
    OG_ALIGN(boxes_dev);
    OG_ALIGN(area_dev);
    OG_ALIGN(n_kept_out);
    if (!g) return fail(OG_EINVAL, "null handle");
    if (!g->unet->finalized) return fail(OG_ESTATE, "a borrowed handle is not finalized");
    if ((rc = check_resized(g->unet, B, H, W, channels, net_h, net_w))) return rc;
    if (B == 0) {
        if (n_kept_out) *n_kept_out = 0;
        return OG_OK;
    }
    if (!src_dev || !boxes_dev || !area_dev) return fail(OG_EINVAL, "null buffer");
    OG_SCOPE(g);
    og_gated::Gate& k = g->gate[2];
    const size_t HW = (size_t)H * W;
    if ((rc = gate_ensure(g, k, B, HW * channels, mask_dev_or_null ? HW : 0))) return rc;
    int n = 0;
    rc = gate_select_enqueue(g, k, boxes_dev, B, g->unet->stream);
    if (!rc) rc = gate_segment_enqueue(g, k, src_dev, B, H, W, channels, net_h, net_w, threshold, boxes_dev, mask_dev_or_null, area_dev, &n);
    if (rc) {
        gated_drain(g);   // error path only: nothing of this call is in flight when the error is reported
        return rc;
    }
    if (n_kept_out) *n_kept_out = n;
    return OG_OK;
}

int og_gated_stream_kept_u8(og_gated* g, const uint8_t* frames, int B, int H, int W, int channels, int imgsz, int net_h, int net_w,
                            float conf, float threshold, const uint8_t* resets_or_null, int32_t* area, int32_t* boxes_or_null,
                            float* best_or_null, uint8_t* mask_or_null, int32_t* n_kept_or_null) {
    return gated_stream_impl(g, frames, nullptr, B, H, W, channels, imgsz, net_h, net_w, conf, threshold, resets_or_null, area, boxes_or_null,
                             best_or_null, mask_or_null, true, n_kept_or_null);
}

int og_gated_stream_kept_frames_u8(og_gated* g, const uint8_t* const* frame_ptrs, int B, int H, int W, int channels, int imgsz, int net_h,
                                   int net_w, float conf, float threshold, const uint8_t* resets_or_null, int32_t* area,
                                   int32_t* boxes_or_null, float* best_or_null, uint8_t* mask_or_null, int32_t* n_kept_or_null) {
    if (!frame_ptrs && B > 0) return fail(OG_EINVAL, "frame_ptrs is null");
    return gated_stream_impl(g, nullptr, frame_ptrs, B, H, W, channels, imgsz, net_h, net_w, conf, threshold, resets_or_null, area,
                             boxes_or_null, best_or_null, mask_or_null, true, n_kept_or_null);
}

int og_gate_plan(int B, int H, int W, int channels, int stage_kib, int with_mask, char* out, size_t cap, long long* engine_bytes) {
    if (with_mask != 0 && with_mask != 1) return fail(OG_EINVAL, "with_mask must be 0 or 1");
    OG_ALIGN(engine_bytes);
    const int n = og_gated_plan(B, H, W, channels, stage_kib, out, cap, nullptr);
    if (n < 0) return n;
    if (engine_bytes) {
        const int mb = gated_cap(H, W, channels, stage_kib);
        *engine_bytes = gated_engine_bytes(mb, H, W, channels, with_mask != 0) + 2 * gate_slot_bytes(mb, H, W, channels, with_mask != 0);
    }
    return n;
}

}  // extern "C"
