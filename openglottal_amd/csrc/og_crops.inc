// The YOLO-Crop+UNet video pipeline (include/openglottal_hip_crops.h; scripts/infer.py:222-248): the crop leg of the streaming
// engine.  Included by og_api.hip, as og_yolo.inc is.  Shaped like the resized mode of stream_impl: per micro-batch the source
// frames go up into a ring slot, k_crop_tiles writes the size x size tiles (geometry computed on the device, BGR2GRAY per tap), the
// chain runs at size x size and leaves its tile masks in the slot, and k_crop_project counts the area inside the box (and writes
// the full-frame mask when one is asked for).  The two crop kernels are launched eagerly on the lane's stream around run_chunk, as
// k_resize_in / k_resize_out are; run_chunk's own graphs for size x size stay as they are, and there is no zero-copy variant.
#include "../../include/openglottal_hip_crops.h"

namespace {

int check_crops(og_unet* h, int B, int H, int W, int ch, int size) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (!h->finalized) return fail(OG_ESTATE, "og_unet_finalize() has not been called");
    if (B < 0 || H <= 0 || W <= 0) return fail(OG_EINVAL, "bad B/H/W");
    if (size <= 0) return fail(OG_EINVAL, "size must be positive");
    if (H > kResizeMaxSide || W > kResizeMaxSide || size > kResizeMaxSide)
        return fail(OG_EINVAL, "frame or tile side above " + std::to_string(kResizeMaxSide));
    if (ch != 1 && ch != 3) return fail(OG_EINVAL, "channels must be 1 (gray) or 3 (BGR)");
    return check_shape(h, B, size, size);   // the tile side must be a multiple of 2^n_levels
}

// source u8 [nb,H,W,ch] + boxes [nb,4] -> tiles u8 [nb,size,size] (the input k_conv_first<u8> reads)
int enqueue_crop_in(hipStream_t st, int ch, const uint8_t* src, int nb, int H, int W, const int32_t* boxes, int size, uint8_t* tiles) {
    const dim3 grid((unsigned)((size * size + 255) / 256), (unsigned)nb);
    if (ch == 3)
        OG_LAUNCH(k_crop_tiles<3>, grid, dim3(256), 0, st, src, H, W, boxes, size, tiles);
    else
        OG_LAUNCH(k_crop_tiles<1>, grid, dim3(256), 0, st, src, H, W, boxes, size, tiles);
    return OG_OK;
}

// tile masks u8 [nb,size,size] -> area [nb] (zero on entry) and, when asked for, the full-frame mask [nb,H,W]
int enqueue_crop_out(hipStream_t st, const uint8_t* tile_masks, int nb, int size, const int32_t* boxes, int H, int W, uint8_t* mask,
                     int32_t* area) {
    if (!mask && !area) return OG_OK;
    if (mask) {
        const dim3 grid((unsigned)((H * W + 255) / 256), (unsigned)nb);
        OG_LAUNCH(k_crop_project<true>, grid, dim3(256), 0, st, tile_masks, size, boxes, H, W, mask, area);
    } else {
        const dim3 grid((unsigned)kCropProjectBlocks, (unsigned)nb);
        OG_LAUNCH(k_crop_project<false>, grid, dim3(256), 0, st, tile_masks, size, boxes, H, W, mask, area);
    }
    if (g_plan) {   // extents from the launch's own geometry: nb frames from each pointer
        plan_write("mask", mask, (long long)nb * H * W);
        plan_write("area", area, (long long)nb * 4);
    }
    return OG_OK;
}

// one micro-batch of nb resident frames on `lane`; area (may be null) must be zero on entry
int crops_micro_batch(og_unet* lane, int ch, const uint8_t* src, int nb, int H, int W, const int32_t* boxes, int size, float thr,
                      uint8_t* tiles, uint8_t* tile_masks, uint8_t* mask, int32_t* area) {
    int rc = enqueue_crop_in(lane->stream, ch, src, nb, H, W, boxes, size, tiles);
    if (!rc) rc = run_chunk(lane, KIND_U8, tiles, nb, size, size, thr, nullptr, tile_masks, nullptr, nullptr);
    if (!rc) rc = enqueue_crop_out(lane->stream, tile_masks, nb, size, boxes, H, W, mask, area);
    return rc;
}

// frame indices with a usable box, in order: the compaction list of the host entries and of the dry run
std::vector<int> usable_frames(const int32_t* boxes, int B, int H, int W, int size) {
    std::vector<int> idx;
    int geom[4];
    for (int b = 0; b < B; ++b)
        if (og_crop_usable(boxes[4 * b], boxes[4 * b + 1], boxes[4 * b + 2], boxes[4 * b + 3], H, W, size, geom)) idx.push_back(b);
    return idx;
}

int crops_stream_impl(og_unet* h, const uint8_t* frames, const uint8_t* const* frame_ptrs, int B, int H, int W, int ch,
                      const int32_t* boxes, int size, float thr, uint8_t* mask, int32_t* area) {
    OG_SCOPE(h);
    int rc = check_crops(h, B, H, W, ch, size);
    if (rc) return rc;
    OG_ALIGN(frame_ptrs);
    OG_ALIGN(boxes);
    OG_ALIGN(area);
    if (B == 0) return OG_OK;
    if (!frames && !frame_ptrs) return fail(OG_EINVAL, "frames is null");
    if (!boxes) return fail(OG_EINVAL, "boxes is null");
    if (frame_ptrs)
        for (int i = 0; i < B; ++i)
            if (!frame_ptrs[i]) return fail(OG_EINVAL, "frame_ptrs[" + std::to_string(i) + "] is null");
    const size_t HW = (size_t)H * W, fb = HW * ch;
    const std::vector<int> idx = usable_frames(boxes, B, H, W, size);
    const int n = (int)idx.size();
    // frames without a usable box: area 0 and a zeroed mask from the host; they never reach the device
    if (area) memset(area, 0, (size_t)B * 4);
    if (mask)
        for (int b = 0, j = 0; b < B; ++b) {
            if (j < n && idx[j] == b) ++j;
            else memset(mask + b * HW, 0, HW);
        }
    if (n == 0) return OG_OK;
    const int chunk = resized_chunk(h, H, W, ch);   // the handle's chunk, lowered to 64 MiB of source frames per slot
    const int cb = chunk < n ? chunk : n;
    const int n_chunks = (n + chunk - 1) / chunk;
    og_unet* lanes[kMaxLanes] = {h};
    int n_lanes = 1;
    const int want = h->n_lanes ? h->n_lanes : (chunk <= 16 ? 3 : 2);
    if (h->dual)
        for (og_unet* t = h->twin; t && n_lanes < want && n_lanes < n_chunks; t = t->twin) lanes[n_lanes++] = t;
    for (int l = 0; l < n_lanes; ++l)
        if ((rc = ensure_arena(lanes[l], cb, size, size))) return rc;
    for (int l = 0; l < n_lanes; ++l) lanes[l]->active_lanes = n_lanes;
    const int n_slots = (n_chunks < n_lanes + 2) ? n_chunks : n_lanes + 2;
    // the slot buffers of the resized mode at network size size x size: d_gray holds the tiles, d_net the tile masks
    if ((rc = ensure_ring(h, n_slots, cb, H, W, ch, mask != nullptr, false, size, size))) return rc;
    auto& R = h->ring;
    const bool single = n_chunks == 1;

    auto retire = [&](og_unet::Slot& s) -> int {   // wait for the slot's outputs and scatter them to their frame indices
        if (s.b0 < 0) return OG_OK;
        const int k0 = s.b0, nb = s.nb;
        s.b0 = -1;
        HIPCHK(hipEventSynchronize(s.ev_out));
        for (int j = 0; j < nb; ++j) {
            if (area) area[idx[k0 + j]] = s.h_area[j];
            if (mask) memcpy(mask + idx[k0 + j] * HW, s.h_mask + j * HW, HW);
        }
        return OG_OK;
    };
    auto fill = [&](og_unet::Slot& s, og_unet* lane, int k0, int nb) -> int {   // usable frames idx[k0 .. k0 + nb)
        for (int j = 0; j < nb; ++j) {
            const int b = idx[k0 + j];
            memcpy(s.h_in + (size_t)j * fb, frame_ptrs ? frame_ptrs[b] : frames + (size_t)b * fb, fb);
            memcpy(s.h_boxes + 4 * j, boxes + 4 * (size_t)b, 16);
        }
        const hipStream_t s_in = single ? lane->stream : R.s_h2d, s_out = single ? lane->stream : R.s_d2h;
        HIPCHK(hipMemcpyAsync(s.d_in, s.h_in, nb * fb, hipMemcpyHostToDevice, s_in));
        HIPCHK(hipMemcpyAsync(s.d_boxes, s.h_boxes, (size_t)nb * 16, hipMemcpyHostToDevice, s_in));
        if (!single) {
            HIPCHK(hipEventRecord(s.ev_h2d, R.s_h2d));
            HIPCHK(hipStreamWaitEvent(lane->stream, s.ev_h2d, 0));
        }
        if (area) HIPCHK(hipMemsetAsync(s.d_area, 0, (size_t)nb * 4, lane->stream));
        const int rc2 = crops_micro_batch(lane, ch, s.d_in, nb, H, W, s.d_boxes, size, thr, s.d_gray, (uint8_t*)s.d_net,
                                          mask ? s.d_mask : nullptr, area ? s.d_area : nullptr);
        if (rc2) return rc2;
        if (!single) {
            HIPCHK(hipEventRecord(s.ev_done, lane->stream));
            HIPCHK(hipStreamWaitEvent(R.s_d2h, s.ev_done, 0));
        }
        if (area) HIPCHK(hipMemcpyAsync(s.h_area, s.d_area, (size_t)nb * 4, hipMemcpyDeviceToHost, s_out));
        if (mask) HIPCHK(hipMemcpyAsync(s.h_mask, s.d_mask, nb * HW, hipMemcpyDeviceToHost, s_out));
        HIPCHK(hipEventRecord(s.ev_out, s_out));
        s.b0 = k0;
        s.nb = nb;
        return OG_OK;
    };

    int k = 0;
    for (int k0 = 0; k0 < n && !rc; k0 += chunk, ++k) {
        og_unet::Slot& s = R.slots[k % n_slots];
        if ((rc = retire(s))) break;   // frees the slot: its previous micro-batch (k - n_slots) is complete and delivered
        rc = fill(s, lanes[k % n_lanes], k0, (n - k0 < chunk) ? n - k0 : chunk);
    }
    for (int i = 0; i < n_slots; ++i) {   // drain in age order; on error still wait for everything in flight
        const int rc2 = retire(R.slots[(k + i) % n_slots]);
        if (!rc) rc = rc2;
    }
    if (rc) {
        const std::string err = g_err;
        (void)hipStreamSynchronize(R.s_h2d);
        for (int l = 0; l < n_lanes; ++l) {
            reset_counters(lanes[l]);
            (void)hipStreamSynchronize(lanes[l]->stream);
        }
        (void)hipStreamSynchronize(R.s_d2h);
        for (auto& s : R.slots) s.b0 = -1;
        g_err = err;
    }
    return rc ? rc : check_range(h);
}

}  // namespace

extern "C" {

int og_crop_geometry_host(int h, int w, int size, int32_t* geom4) {
    if (h < 1 || w < 1 || size < 1 || !geom4) return fail(OG_EINVAL, "bad argument");
    OG_ALIGN(geom4);
    int g[4];
    og_crop_geometry(h, w, size, g);
    for (int i = 0; i < 4; ++i) geom4[i] = g[i];
    return OG_OK;
}

int og_crop_tile_host(const uint8_t* frame, int H, int W, int channels, const int32_t* box4, int size, uint8_t* tile) {
    if (!frame || !box4 || !tile || H < 1 || W < 1 || size < 1 || (channels != 1 && channels != 3)) return fail(OG_EINVAL, "bad argument");
    OG_ALIGN(box4);
    const int x1 = box4[0], y1 = box4[1], x2 = box4[2], y2 = box4[3];
    int g[4];
    if (!og_crop_usable(x1, y1, x2, y2, H, W, size, g)) {
        memset(tile, 0, (size_t)size * size);
        return OG_OK;
    }
    for (int ty = 0; ty < size; ++ty)
        for (int tx = 0; tx < size; ++tx)
            tile[(size_t)ty * size + tx] = channels == 3 ? og_crop_tile_px<3>(frame, W, x1, y1, x2, y2, g, ty, tx)
                                                         : og_crop_tile_px<1>(frame, W, x1, y1, x2, y2, g, ty, tx);
    return OG_OK;
}

int og_crop_project_host(const uint8_t* tile_mask, int size, const int32_t* box4, int H, int W, uint8_t* mask_or_null, int32_t* area) {
    if (!tile_mask || !box4 || !area || H < 1 || W < 1 || size < 1) return fail(OG_EINVAL, "bad argument");
    OG_ALIGN(box4);
    OG_ALIGN(area);
    const int x1 = box4[0], y1 = box4[1], x2 = box4[2], y2 = box4[3];
    int g[4];
    const bool ok = og_crop_usable(x1, y1, x2, y2, H, W, size, g);
    if (mask_or_null) memset(mask_or_null, 0, (size_t)H * W);
    int cnt = 0;
    if (ok)
        for (int y = y1; y < y2; ++y)
            for (int x = x1; x < x2; ++x) {
                const uint8_t v = og_crop_project_px(tile_mask, size, x1, y1, x2, y2, g, y, x);
                if (mask_or_null) mask_or_null[(size_t)y * W + x] = v;
                cnt += v > 0 ? 1 : 0;
            }
    *area = cnt;
    return OG_OK;
}

int og_unet_stream_crops_u8(og_unet* h, const uint8_t* frames, int B, int H, int W, int channels, const int32_t* boxes, int size,
                            float thr, uint8_t* mask, int32_t* area) {
    return crops_stream_impl(h, frames, nullptr, B, H, W, channels, boxes, size, thr, mask, area);
}

int og_unet_stream_frames_crops_u8(og_unet* h, const uint8_t* const* frame_ptrs, int B, int H, int W, int channels,
                                   const int32_t* boxes, int size, float thr, uint8_t* mask, int32_t* area) {
    if (!frame_ptrs && B > 0) return fail(OG_EINVAL, "frame_ptrs is null");
    return crops_stream_impl(h, nullptr, frame_ptrs, B, H, W, channels, boxes, size, thr, mask, area);
}

int og_unet_segment_crops_area_u8_dev(og_unet* h, const uint8_t* src, int B, int H, int W, int channels, const int32_t* boxes, int size,
                                      float thr, uint8_t* tiles_scratch, uint8_t* tile_masks_scratch, uint8_t* mask, int32_t* area) {
    OG_SCOPE(h);
    int rc = check_crops(h, B, H, W, channels, size);
    if (rc) return rc;
    OG_ALIGN(boxes);
    OG_ALIGN(area);
    if (B == 0) return OG_OK;
    if (!src || !boxes || !tiles_scratch || !tile_masks_scratch) return fail(OG_EINVAL, "null buffer");
    const int chunk = resized_chunk(h, H, W, channels), cb = chunk < B ? chunk : B;
    if ((rc = ensure_arena(h, cb, size, size))) return rc;
    h->active_lanes = 1;
    if (area) HIPCHK(hipMemsetAsync(area, 0, (size_t)B * sizeof(int32_t), h->stream));
    const size_t HW = (size_t)H * W, SS = (size_t)size * size;
    for (int b0 = 0; b0 < B && !rc; b0 += chunk) {
        const int nb = (B - b0 < chunk) ? B - b0 : chunk;
        rc = crops_micro_batch(h, channels, src + b0 * HW * channels, nb, H, W, boxes + 4 * (size_t)b0, size, thr, tiles_scratch + b0 * SS,
                               tile_masks_scratch + b0 * SS, mask ? mask + b0 * HW : nullptr, area ? area + b0 : nullptr);
    }
    if (rc) {
        const std::string err = g_err;
        reset_counters(h);
        (void)hipStreamSynchronize(h->stream);   // error path only: nothing of this call is in flight when the error is reported
        g_err = err;
    }
    return rc;
}

int og_unet_plan_crops(const int* features, int n_levels, int B, int H, int W, int channels, const int32_t* boxes, int size, int lanes,
                       const char* options, char* out, size_t cap, long long* arena_bytes) {
    if (!out || cap == 0 || B < 1 || !boxes) return fail(OG_EINVAL, "bad argument");
    OG_ALIGN(boxes);
    og_unet* h = og_unet_create(features, n_levels, 1, 1);
    if (!h) return OG_EINVAL;
    h->host_only = true;
    int rc = og_unet_finalize(h);
    if (!rc) rc = check_crops(h, B, H, W, channels, size);
    std::string opt = options ? options : "";
    for (size_t p0 = 0; !rc && p0 < opt.size();) {   // "name=value,name=value"
        size_t p1 = opt.find(',', p0);
        if (p1 == std::string::npos) p1 = opt.size();
        const std::string kv = opt.substr(p0, p1 - p0);
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) rc = fail(OG_EINVAL, "option without '=': " + kv);
        else if (kv.substr(0, eq) == "chunk") rc = og_unet_set_chunk(h, atoi(kv.c_str() + eq + 1));
        else rc = og_unet_set_option(h, kv.substr(0, eq).c_str(), atoi(kv.c_str() + eq + 1));
        p0 = p1 + 1;
    }
    Plan plan;
    if (!rc) {
        const std::vector<int> idx = usable_frames(boxes, B, H, W, size);
        const int n = (int)idx.size();
        const int chunk = resized_chunk(h, H, W, channels), cb = n == 0 ? 1 : (chunk < n ? chunk : n);
        ArenaPlan ap = arena_layout(h, cb, size, size);
        if (arena_bytes) *arena_bytes = (long long)ap.total;
        adopt_arena(h, ap, (void*)4096, cb, size, size);   // placeholder bases: nothing dereferences them in a dry run
        h->active_lanes = lanes < 1 ? 1 : lanes;
        // the micro-batches of og_unet_stream_crops_u8 with mask and area asked for; every micro-batch writes the buffers of a ring slot
        const uintptr_t gap = (uintptr_t)1 << 40;
        uint8_t* mask = (uint8_t*)(1 * gap);
        int32_t* area = (int32_t*)(2 * gap);
        plan.bases = {{"mask", mask}, {"area", area}};
        g_plan = &plan;
        for (int k0 = 0; k0 < n && !rc; k0 += chunk)
            rc = crops_micro_batch(h, channels, (const uint8_t*)(3 * gap), (n - k0 < chunk) ? n - k0 : chunk, H, W, (const int32_t*)(4 * gap),
                                   size, 0.5f, (uint8_t*)(5 * gap), (uint8_t*)(6 * gap), mask, area);
        g_plan = nullptr;
    }
    og_unet_destroy(h);
    if (rc) return rc;
    return og_plan_text(plan, kPlanWrites, out, cap);
}

}  // extern "C"
