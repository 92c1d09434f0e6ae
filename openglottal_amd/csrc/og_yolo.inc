// YOLOv8 detector host side (included by og_api.hip; shares its helpers).
//
// Replaces the `self.model(frame_bgr, conf=..., verbose=False)` call of
// openglottal/models/detector.py:58 — i.e. ultralytics' predictor: BGR->RGB, /255, YOLOv8n
// forward, Detect decode, top-confidence box.  ultralytics is a third-party dependency of the
// reference (`pyproject.toml:25`, `ultralytics>=8.0`, no pin, not vendored, not installed here):
// the architecture below restates its published yolov8.yaml (scale n/s: depth .33) and
// nn/modules {Conv, C2f, Bottleneck, SPPF, Detect, DFL}.  PARITY UNPINNED against ultralytics.
//
// Weights arrive under ultralytics' own state_dict keys ("model.0.conv.weight",
// "model.2.m.0.cv1.bn.running_var", "model.22.cv2.0.2.bias", ...), either with BatchNorm tensors
// (eps 1e-3) or already fused (conv.weight + conv.bias).  Channel widths and C2f depths are
// inferred from the tensor shapes.

namespace {

struct YView {  // one logical tensor = a channel segment of an NHWC buffer
    float* base = nullptr;
    int Ctot = 0;     // pixel stride of the buffer (floats)
    int off = 0;      // first channel of the segment
    int C = 0;        // logical channels
    int H = 0, W = 0;
    int es = 1;       // elements per 4-byte unit: 1 = f32, 2 = f16 ("precision" 2; Ctot, off and C keep counting CHANNELS)
    long long frame_stride() const { return (long long)H * W * Ctot; }
    // what the kernels take: strides and channel offsets in 4-byte units (every physical width and offset is a multiple of 32 channels)
    long long fs4() const { return frame_stride() / es; }
    int ps4() const { return Ctot / es; }
    int off4() const { return off / es; }
};

struct YSeg {
    int off, C;
};

struct YConv {
    std::string name;
    int kind = 0;  // 0 MFMA 3x3 s1, 2 MFMA 1x1, 3 direct (VALU), 4 MFMA 3x3 stride 2 (space-to-depth view)
    int Cin = 0, Cout = 0, Cin_p = 0, Cout_p = 0, ks = 1, stride = 1, act = 2, NT = 1;
    float *d_w = nullptr, *d_scale = nullptr, *d_shift = nullptr;
    float* d_w1 = nullptr;   // NT == 2 layers: the same weights packed for 32-column tiles (latency path: twice the workgroups)
    float* d_wf = nullptr;   // MFMA convs: the f16 image of the same weights ("precision" 2, k_conv_mfma_fy), rounded once at finalize
    bool f32out = false;     // Detect's last Conv2d layers: their logits stay f32 in f16 mode
};

struct YAct {  // a named tensor: channel segments of one buffer, concatenated in order
    YView v;
    std::vector<YSeg> segs;   // (first channel in the buffer, logical width)
};

}  // namespace

struct og_yolo {
    std::map<std::string, HostTensor> host;
    std::map<std::string, int> couts;   // weight key -> output channels (kept after the host copies are dropped)
    bool finalized = false;
    int device = 0;   // as og_unet::device
    int nc = 1, reg_max = 16;
    bool host_only = false;             // og_yolo_plan's copy: layer shapes and launch decisions only -- no device, no stream, placeholder pointers
    int trace_launches = 0;             // DIAGNOSTIC ("trace_launches" 1): keep the (label, module) of every launch of the last chain (og_yolo_last_launches)
    std::vector<std::pair<std::string, std::string>> last_launches;
    og_yolo* plan_copy = nullptr;       // og_yolo_plan: the finalized host-only copy of this (unfinalized) handle, kept between calls; a new tensor drops it
    int n_c2f[8] = {0};                 // bottleneck counts of the eight C2f blocks (2,4,6,8,12,15,18,21)
    std::map<std::string, YConv> convs; // by module path, e.g. "model.4.m.1.cv2"
    hipStream_t stream = nullptr;
    int n_cu = 256;
    float* d_zero = nullptr;
    // arena
    int capB = 0, aH = 0, aW = 0;
    void* arena = nullptr;
    std::map<std::string, YAct> acts;   // named logical tensors (for parity tests)
    int precision = 0;           // 0: f32 (default); 2: opt-in f16 mode (f16 weights and activations, f32 accumulation, f32 logits)
    int* h_range = nullptr;      // f16 mode: host-mapped word the kernels raise when an activation leaves the f16 range
    int* d_range = nullptr;
    void* stage = nullptr;
    size_t stage_bytes = 0;
    int lastB = 0;
    // latency path (calls of at most `latency_batch` frames: the reference's one-frame-per-call pattern): convs that
    // would leave most of the chip idle split K over workgroups (fused reduce, as in the U-Net's batch-1 chain)
    int latency_batch = 1;
    int zero_copy = 1;           // latency path: the first kernel reads the frame from, the decode writes the best box to, pinned host memory
    int splitk_slots = 1, splitk_div = 2;
    int splitk_max = 8;          // most K parts per tile (the last part to arrive sums them all)
    int splitk_min_steps = 3;    // smallest K part of a 3x3 conv, in (chunk, tap) steps
    int latency_nt1 = 1;         // 32-column tiles on the latency path (twice the workgroups per layer)
    static constexpr int kDecBlocks = 512;   // most decode workgroups per frame (64 anchors each)
    float* d_cand = nullptr;     // [64 frames][kDecBlocks][8]: per-workgroup best candidates of k_yolo_decode_mb
    int* d_dec_counter = nullptr;
    bool head_synth = false;     // model.22.hd.{l}.{0,1,2} built (see y_synth_head)
    int head_fused = 1;          // latency path: a level's box and class branches as ONE chain of three convs
    float* d_partial = nullptr;      // split-K workspace + arrival counters of the latency path
    int* d_tile_counter = nullptr;
    // pinned host staging of the latency path (frame in, boxes out): async copies, one wait per call
    void* pin = nullptr;
    size_t pin_bytes = 0;
    int pend_B = 0;              // og_yolo_detect_u8_begin: frames of the call in flight (0: none)
    size_t pend_off = 0;         // ... offset of its `best` rows in the pinned buffer
    bool pend_sync = false;      // ... the call ran synchronously; its results wait in pend_best
    std::vector<float> pend_best;
    // frames of any size (og_yolo_detect_resized_u8*): source frames staged in chunks, letterboxed on the device (k_letterbox_bgr)
    int source_stage_kib = 65536;   // most KiB of source frames staged per upload (64 MiB, as the U-Net's kResizeSlotBytes); a larger frame is staged alone
    int source_mapped = 1;          // latency path: k_letterbox_bgr reads the source frame from the mapped pinned buffer (1, measured 12-15 us faster per call) or after an async copy (0)
    long long n_letterbox = 0, n_scale_boxes = 0;   // launches so far (og_yolo_launch_count)
    bool pend_resized = false;      // the call in flight came through og_yolo_detect_resized_u8_begin: end maps its boxes to source pixels
    int pend_H = 0, pend_W = 0, pend_left = 0, pend_top = 0;
    float pend_gain = 1.f;
    bool pend_scale = false;
};

inline bool og_skip_device(const og_yolo* h) { return !h || h->host_only || !h->finalized; }

namespace {

bool yhas(const og_yolo* h, const std::string& k) { return h->host.count(k) != 0; }

// Conv module -> folded scale/shift (BN eps 1e-3, ultralytics' initialize_weights) or fused bias.
int y_affine(const og_yolo* h, const std::string& mod, int Cout, std::vector<float>& sc, std::vector<float>& sh, bool plain_conv2d) {
    sc.assign(Cout, 1.f);
    sh.assign(Cout, 0.f);
    if (plain_conv2d) {  // nn.Conv2d with bias (Detect's last layers)
        if (yhas(h, mod + ".bias")) {
            const auto& b = h->host.at(mod + ".bias").data;
            for (int c = 0; c < Cout; ++c) sh[c] = b[c];
        }
        return OG_OK;
    }
    if (yhas(h, mod + ".bn.weight")) {
        for (const char* f : {".bn.bias", ".bn.running_mean", ".bn.running_var"})
            if (!yhas(h, mod + f)) return fail(OG_EINVAL, "missing key " + mod + f);
        const auto& g = h->host.at(mod + ".bn.weight").data;
        const auto& b = h->host.at(mod + ".bn.bias").data;
        const auto& mu = h->host.at(mod + ".bn.running_mean").data;
        const auto& var = h->host.at(mod + ".bn.running_var").data;
        for (int c = 0; c < Cout; ++c) {
            const double s = (double)g[c] / std::sqrt((double)var[c] + 1e-3);
            sc[c] = (float)s;
            sh[c] = (float)((double)b[c] - (double)mu[c] * s);
        }
    } else if (yhas(h, mod + ".conv.bias")) {  // exported after model.fuse()
        const auto& b = h->host.at(mod + ".conv.bias").data;
        for (int c = 0; c < Cout; ++c) sh[c] = b[c];
    } else {
        return fail(OG_EINVAL, "module " + mod + " has neither bn.* nor conv.bias");
    }
    return OG_OK;
}

// Latency path: the two branches of a Detect level (box: cv2.l, class: cv3.l; three convs each) as ONE chain of three
// convs -- 9 launches instead of 18 on a path whose launches sit on their latency floors.  Conv 0 of both branches reads
// the same map: the weights stack along the output channels.  Convs 1 and 2 read their own branch: block-diagonal weights
// over the stacked channels; the zero blocks add exact zeros to every sum.  Synthesised host tensors model.22.hd.{l}.{j}.
bool y_synth_head(og_yolo* h) {
    auto get = [&](const std::string& k) -> const HostTensor* {
        auto it = h->host.find(k);
        return it == h->host.end() ? nullptr : &it->second;
    };
    std::map<std::string, HostTensor> add;
    for (int l = 0; l < 3; ++l) {
        const std::string pb = "model.22.cv2." + std::to_string(l), pc = "model.22.cv3." + std::to_string(l),
                          ph = "model.22.hd." + std::to_string(l);
        for (int j = 0; j < 3; ++j) {
            const std::string sj = "." + std::to_string(j), wk = (j == 2) ? ".weight" : ".conv.weight";
            const HostTensor *wb = get(pb + sj + wk), *wc = get(pc + sj + wk);
            if (!wb || !wc || wb->shape.size() != 4 || wc->shape.size() != 4) return false;
            const int ob = (int)wb->shape[0], oc = (int)wc->shape[0], ib = (int)wb->shape[1], ic = (int)wc->shape[1];
            const int kk = (int)(wb->shape[2] * wb->shape[3]);
            if (wc->shape[2] != wb->shape[2] || wc->shape[3] != wb->shape[3] || (j == 0 && ib != ic)) return false;
            const int cin = (j == 0) ? ib : ib + ic;
            HostTensor w;
            w.shape = {ob + oc, cin, wb->shape[2], wb->shape[3]};
            if (!h->host_only) w.data.assign((size_t)(ob + oc) * cin * kk, 0.f);
            for (int o = 0; !h->host_only && o < ob; ++o)
                for (int i = 0; i < ib; ++i)
                    for (int t = 0; t < kk; ++t) w.data[((size_t)o * cin + i) * kk + t] = wb->data[((size_t)o * ib + i) * kk + t];
            const int ioff = (j == 0) ? 0 : ib;
            for (int o = 0; !h->host_only && o < oc; ++o)
                for (int i = 0; i < ic; ++i)
                    for (int t = 0; t < kk; ++t) w.data[((size_t)(ob + o) * cin + ioff + i) * kk + t] = wc->data[((size_t)o * ic + i) * kk + t];
            add[ph + sj + wk] = std::move(w);
            std::vector<std::string> fs;
            if (j == 2) fs = {".bias"};
            else fs = {".bn.weight", ".bn.bias", ".bn.running_mean", ".bn.running_var", ".conv.bias"};
            for (const auto& f : fs) {
                const HostTensor *vb = get(pb + sj + f), *vc = get(pc + sj + f);
                if (!vb && !vc) continue;
                if (j != 2 && (!vb || !vc)) return false;   // one branch folded, the other not: keep the per-branch chain
                auto numel = [](const HostTensor* t) { long long n = 1; for (auto d : t->shape) n *= d; return n; };
                if ((vb && numel(vb) != ob) || (vc && numel(vc) != oc)) return false;
                HostTensor v;
                v.shape = {ob + oc};
                if (!h->host_only) {
                    v.data.assign(ob + oc, 0.f);
                    if (vb) std::copy(vb->data.begin(), vb->data.end(), v.data.begin());
                    if (vc) std::copy(vc->data.begin(), vc->data.end(), v.data.begin() + ob);
                }
                add[ph + sj + f] = std::move(v);
            }
        }
    }
    for (auto& kv : add) h->host[kv.first] = std::move(kv.second);
    return true;
}

// in_segs / out_segs: physical channel segments (offset relative to the view's first segment, logical width)
int y_build_conv(og_yolo* h, const std::string& mod, bool plain_conv2d, int kind, int stride, int act,
                 const std::vector<YSeg>& in_segs, const std::vector<YSeg>& out_segs) {
    const std::string wkey = plain_conv2d ? mod + ".weight" : mod + ".conv.weight";
    if (!yhas(h, wkey)) return fail(OG_EINVAL, "missing key " + wkey);
    const HostTensor& wt = h->host.at(wkey);
    if (wt.shape.size() != 4) return fail(OG_EINVAL, "bad weight rank for " + wkey);
    YConv L;
    L.name = mod;
    L.kind = kind;
    L.Cout = (int)wt.shape[0];
    L.Cin = (int)wt.shape[1];
    L.ks = (int)wt.shape[2];
    L.stride = stride;
    L.act = act;
    int cin_sum = 0, cout_sum = 0;
    for (auto& s_ : in_segs) cin_sum += s_.C;
    for (auto& s_ : out_segs) cout_sum += s_.C;
    if (cin_sum != L.Cin || cout_sum != L.Cout)
        return fail(OG_EINVAL, "channel mismatch at " + mod + ": weight [" + std::to_string(L.Cout) + "," + std::to_string(L.Cin) +
                                   "] vs graph [" + std::to_string(cout_sum) + "," + std::to_string(cin_sum) + "]");
    // physical <-> logical channel maps
    const int in_base = in_segs.front().off, out_base = out_segs.front().off;
    L.Cin_p = in_segs.back().off + cp32(in_segs.back().C) - in_base;
    L.Cout_p = out_segs.back().off + cp32(out_segs.back().C) - out_base;
    if (h->host_only) {   // shapes only: every image a launch decision asks for "exists"
        if (kind == 3 && in_segs.size() != 1) return fail(OG_EINVAL, "direct conv with concatenated input");
        if (kind == 4 && (L.ks != 3 || stride != 2)) return fail(OG_EINVAL, "kind 4 is the 3x3 stride-2 conv: " + mod);
        if ((kind == 0 && L.ks != 3) || (kind == 2 && L.ks != 1)) return fail(OG_EINVAL, "kernel size mismatch at " + mod);
        if (kind != 3) L.NT = (L.Cout_p % 64 == 0) ? 2 : 1;
        L.d_w = L.d_scale = L.d_shift = (float*)8;
        L.d_w1 = (L.NT == 2) ? (float*)8 : nullptr;
        L.d_wf = (kind != 3) ? (float*)8 : nullptr;
        L.f32out = plain_conv2d;
        h->convs[mod] = L;
        return OG_OK;
    }
    std::vector<int> cin_map(L.Cin_p, -1), cout_map(L.Cout_p, -1);
    int lc = 0;
    for (auto& s_ : in_segs)
        for (int c = 0; c < s_.C; ++c) cin_map[s_.off - in_base + c] = lc++;
    lc = 0;
    for (auto& s_ : out_segs)
        for (int c = 0; c < s_.C; ++c) cout_map[s_.off - out_base + c] = lc++;
    std::vector<float> sc_l, sh_l, sc(L.Cout_p, 0.f), sh(L.Cout_p, 0.f);
    int rc = y_affine(h, mod, L.Cout, sc_l, sh_l, plain_conv2d);
    if (rc) return rc;
    for (int n = 0; n < L.Cout_p; ++n)
        if (cout_map[n] >= 0) {
            sc[n] = sc_l[cout_map[n]];
            sh[n] = sh_l[cout_map[n]];
        }
    const auto& w = wt.data;  // [Cout][Cin][k][k]
    const int kk = L.ks * L.ks, Cin = L.Cin;
    std::vector<float> pk, pk1;
    if (kind == 3) {  // direct: [k*k][Cin_phys][Cout_p]; input is always a single plain segment here
        if (in_segs.size() != 1) return fail(OG_EINVAL, "direct conv with concatenated input");
        pk.assign((size_t)kk * Cin * L.Cout_p, 0.f);
        for (int t = 0; t < kk; ++t)
            for (int ci = 0; ci < Cin; ++ci)
                for (int n = 0; n < L.Cout_p; ++n)
                    if (cout_map[n] >= 0) pk[((size_t)t * Cin + ci) * L.Cout_p + n] = w[((size_t)cout_map[n] * Cin + ci) * kk + t];
    } else if (kind == 4) {
        // k_conv_mfma_o MODE 3: dense sequence of the 9 non-zero (parity, 2x2 tap) pairs per 32-channel chunk, in the
        // kernel's execution order: parity-major (py,px), channel chunk, tap (ty,tx).  (ty,py) -> ky: (0,1) 0, (1,0) 1, (1,1) 2.
        if (L.ks != 3 || stride != 2) return fail(OG_EINVAL, "kind 4 is the 3x3 stride-2 conv: " + mod);
        L.NT = (L.Cout_p % 64 == 0) ? 2 : 1;
        auto pack4 = [&](int NT) {
            std::vector<float> out;
            const int rows = 32 * NT, n_tiles = L.Cout_p / rows, cpc = L.Cin_p / 32;
            out.assign((size_t)L.Cout_p * L.Cin_p * 9, 0.f);
            size_t o = 0;
            for (int nt = 0; nt < n_tiles; ++nt)
                for (int par = 0; par < 4; ++par)
                    for (int cc = 0; cc < cpc; ++cc)
                        for (int t = 0; t < 4; ++t) {
                            const int ty = t >> 1, tx = t & 1, py = par >> 1, px = par & 1;
                            if ((ty == 0 && py == 0) || (tx == 0 && px == 0)) continue;
                            const int ky = (ty == 0) ? 0 : 1 + py, kx = (tx == 0) ? 0 : 1 + px;
                            for (int r = 0; r < rows; ++r)
                                for (int ps = 0; ps < 8; ++ps) {
                                    const int sl = ps ^ ((r >> 1) & 7);
                                    for (int e = 0; e < 4; ++e) {
                                        const int co = cout_map[nt * rows + r], ci = cin_map[cc * 32 + sl * 4 + e];
                                        out[o + (size_t)r * 32 + ps * 4 + e] = (co < 0 || ci < 0) ? 0.f : w[((size_t)co * Cin + ci) * 9 + ky * 3 + kx];
                                    }
                                }
                            o += (size_t)rows * 32;
                        }
            return out;
        };
        pk = pack4(L.NT);
        if (L.NT == 2) pk1 = pack4(1);
    } else {
        if ((kind == 0 && L.ks != 3) || (kind == 2 && L.ks != 1)) return fail(OG_EINVAL, "kernel size mismatch at " + mod);
        L.NT = (L.Cout_p % 64 == 0) ? 2 : 1;
        auto at = [&](int n, int k, int t) -> float {
            const int co = cout_map[n], ci = cin_map[k];
            if (co < 0 || ci < 0) return 0.f;
            return w[((size_t)co * Cin + ci) * kk + t];
        };
        pk = pack_gemm_b(L.Cout_p, L.Cin_p, kk, L.NT, at);
        if (L.NT == 2) pk1 = pack_gemm_b(L.Cout_p, L.Cin_p, kk, 1, at);
        if ((rc = upload(pack_gemm_b_f(L.Cout_p, L.Cin_p, kk, L.NT, at), &L.d_wf))) return rc;
    }
    if (kind == 4) {
        // k_conv_mfma_fy MODE 3: the same 9 (parity, tap) pairs over 64-channel chunks (F layout: eight 16-byte slots of 8 f16),
        // in the kernel's execution order: parity-major, chunk, tap.  A padded Cin that is an odd multiple of 32 leaves the upper
        // half of each parity's last chunk zero (the kernel skips it: ConvArgs::k_half).
        const int rows = 32 * L.NT, n_tiles = L.Cout_p / rows, cpc = (L.Cin_p + 63) / 64;
        std::vector<float> pf((size_t)L.Cout_p * cpc * 32 * 9, 0.f);
        _Float16* o16 = (_Float16*)pf.data();
        size_t o = 0;   // in halves
        for (int nt = 0; nt < n_tiles; ++nt)
            for (int par = 0; par < 4; ++par)
                for (int cc = 0; cc < cpc; ++cc)
                    for (int t = 0; t < 4; ++t) {
                        const int ty = t >> 1, tx = t & 1, py = par >> 1, px = par & 1;
                        if ((ty == 0 && py == 0) || (tx == 0 && px == 0)) continue;
                        const int ky = (ty == 0) ? 0 : 1 + py, kx = (tx == 0) ? 0 : 1 + px;
                        for (int r = 0; r < rows; ++r)
                            for (int ps = 0; ps < 8; ++ps) {
                                const int sl = ps ^ ((r >> 1) & 7);
                                for (int e = 0; e < 8; ++e) {
                                    const int k = cc * 64 + sl * 8 + e;
                                    const int co = cout_map[nt * rows + r], ci = (k < L.Cin_p) ? cin_map[k] : -1;
                                    o16[o + (size_t)r * 64 + ps * 8 + e] = (_Float16)((co < 0 || ci < 0) ? 0.f : w[((size_t)co * Cin + ci) * 9 + ky * 3 + kx]);
                                }
                            }
                        o += (size_t)rows * 64;
                    }
        if ((rc = upload(pf, &L.d_wf))) return rc;
    }
    L.f32out = plain_conv2d;
    if ((rc = upload(pk, &L.d_w))) return rc;
    if (!pk1.empty() && (rc = upload(pk1, &L.d_w1))) return rc;
    if ((rc = upload(sc, &L.d_scale))) return rc;
    if ((rc = upload(sh, &L.d_shift))) return rc;
    h->convs[mod] = L;
    return OG_OK;
}

// k_conv_mfma_fy: the occupancy-shaped grid of launch_conv_f (tile column, tile row, frame group x column tile x frame in group)
template <int NT, int MODE, bool F32OUT = false>
int launch_conv_fy(const LaunchCtx& c, const ConvArgs& a_in, int n_ntiles) {
    constexpr int lds = ConvTile<NT, MODE, 8>::lds_bytes;
    static_assert(lds <= 160 * 1024, "one workgroup of this tile must fit a CU's LDS");
    ConvArgs a = a_in;
    const int gz = grid_z(c, a, n_ntiles, a.tiles_x * a.tiles_y);
    if (gz < 0) return gz;
    OG_LAUNCH_LDS((k_conv_mfma_fy<NT, MODE, 3, F32OUT>), dim3(a.tiles_x, a.tiles_y, gz), dim3(256), lds, c.stream, a);
    plan_inst("k_conv_mfma_fy<%d, %d, 3, %s> chunks=%d k_half=%d", NT, MODE, F32OUT ? "true" : "false", a.n_chunks, a.k_half);
    return OG_OK;
}

// What both precisions pass for an MFMA conv of the detector: the views in the kernels' 4-byte units (f32 views: es 1, the plain
// strides), the weight image of the precision, the layer's affine and activation, the optional residual.  The K walk is the caller's.
ConvArgs y_conv_args(const og_yolo* h, const YConv& L, const float* wpk, const YView& in, const YView& out, const YView* res) {
    return conv_args({in.base, in.fs4(), in.ps4(), in.off4()}, {out.base, out.fs4(), out.ps4(), out.off4()}, ConvView{},
                     res ? ConvView{res->base, res->fs4(), res->ps4(), res->off4()} : ConvView{}, wpk, L.d_scale, L.d_shift, L.Cout_p,
                     h->d_zero, L.act);
}

// f16 mode ("precision" 2): every MFMA conv on k_conv_mfma_fy, the whole K range in ONE workgroup in ONE order at every B -- no
// split-K, no virtual split, no workspace, never k_conv_mfma_p -- so a frame's bits cannot depend on the launch it rides in.
int y_launch_f(og_yolo* h, const YConv& L, int B, const void* in_u8, const YView& in, const YView& out, const YView* res) {
    if (L.kind == 3) {   // model.0: f32 weights, f32 fma chain, rounded output
        if (!in_u8) return fail(OG_ESTATE, "f16 mode runs the stride-2 convs on the MFMA kernel: " + L.name);
        const int Hout = out.H, Wout = out.W, total = B * Hout * ((Wout + 3) / 4);
        // all eight channel quads of a 32-channel group, padded ones included (zero weights: they store 0).  The f32 path leaves the
        // padded slots at whatever the arena holds (finite f32, times a zero weight); here stale bytes of another batch size's
        // layout -- f32 logits -- can read as f16 NaN, and 0 x NaN would poison the next conv
        const int cq_shift = 3;
        const unsigned gx = (unsigned)(((long long)total * (1 << cq_shift) + 255) / 256);
        OG_LAUNCH(k_conv_direct_u8h, dim3(gx, L.Cout_p / 32), dim3(256), 0, h->stream, (const uint8_t*)in_u8, in.H, in.W, L.d_w,
                  L.d_scale, L.d_shift, L.Cout_p, out.base, out.fs4(), out.ps4(), out.off4(), Hout, Wout, L.ks, L.stride, L.ks / 2,
                  L.act, total, cq_shift, h->d_range);
        plan_inst("k_conv_direct_u8h cq_shift=%d", cq_shift);
        return OG_OK;
    }
    if (!L.d_wf) return fail(OG_ESTATE, "no f16 weight image for " + L.name);
    if (L.f32out != (out.es == 1) || in.es != 2) return fail(OG_ESTATE, "f16 mode: buffer format mismatch at " + L.name);
    ConvArgs a = y_conv_args(h, L, L.d_wf, in, out, res);
    const int cpc = (L.Cin_p + 63) / 64;
    a.n_chunks = (L.kind == 4) ? 4 * cpc : cpc;
    a.k_half = (L.Cin_p % 64) ? 1 : 0;
    if (L.kind == 4 && (in.H != 2 * out.H || in.W != 2 * out.W)) return fail(OG_EINVAL, "stride-2 conv needs even input sizes: " + L.name);
    a.H = out.H;   // (kind 4: the kernel addresses the (2H x 2W) input through the space-to-depth view)
    a.W = out.W;
    a.tiles_x = (a.W + 15) / 16;
    a.tiles_y = (a.H + 7) / 8;
    a.n_spatial = B * a.tiles_x * a.tiles_y;
    a.range_flag = h->d_range;
    const LaunchCtx ctx{h->stream, h->n_cu, 2};
    const int n_ntiles = L.Cout_p / (32 * L.NT);
    if (L.f32out) {
        if (L.kind != 2 || L.act != 0 || res) return fail(OG_ESTATE, "f32 logits come from the plain 1x1 Conv2d layers only: " + L.name);
        return og_pick<2, 1>(L.NT, [&](auto nt) { return launch_conv_fy<decltype(nt)::value, 2, true>(ctx, a, n_ntiles); });
    }
    return og_pick<2, 1>(L.NT, [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        if (L.kind == 4) return launch_conv_fy<NT, 3>(ctx, a, n_ntiles);
        if (L.kind == 0) return launch_conv_fy<NT, 0>(ctx, a, n_ntiles);
        return launch_conv_fy<NT, 2>(ctx, a, n_ntiles);
    });
}

int y_launch(og_yolo* h, const std::string& mod, int B, const void* in_u8, const YView& in, const YView& out, const YView* res) {
    auto it = h->convs.find(mod);
    if (it == h->convs.end()) return fail(OG_ESTATE, "conv not built: " + mod);
    const YConv& L = it->second;
    if (h->precision == 2) return y_launch_f(h, L, B, in_u8, in, out, res);
    if (L.kind == 3) {
        const bool px1 = B <= h->latency_batch;   // one-frame calls: one output pixel per thread
        const int Hout = out.H, Wout = out.W, total = px1 ? B * Hout * Wout : B * Hout * ((Wout + 3) / 4);
        const int pad = L.ks / 2;
        // channel quads that hold real channels in a 32-channel group (single-segment outputs only): 16 real -> 4 quads
        int cq_shift = 3;
        if (L.Cout_p == 32 && L.Cout <= 16) cq_shift = (L.Cout <= 4) ? 0 : (L.Cout <= 8) ? 1 : 2;
        const unsigned gx = (unsigned)(((long long)total * (1 << cq_shift) + 255) / 256);
        // (the stride-2 convs behind model.0 run on the MFMA kernel, MODE 3: the only direct conv reads the u8 frame)
        if (!in_u8) return fail(OG_ESTATE, "the direct conv reads the u8 frame only: " + L.name);
        if (px1)
            OG_LAUNCH((k_conv_direct<true, 1>), dim3(gx, L.Cout_p / 32), dim3(256), 0, h->stream, in_u8, 0LL, 0, 0, in.H, in.W, 3,
                      L.d_w, L.d_scale, L.d_shift, L.Cout_p, out.base, out.frame_stride(), out.Ctot, out.off, Hout, Wout,
                      L.ks, L.stride, pad, L.act, total, cq_shift);
        else
            OG_LAUNCH(k_conv_direct<true>, dim3(gx, L.Cout_p / 32), dim3(256), 0, h->stream, in_u8, 0LL, 0, 0, in.H, in.W, 3,
                      L.d_w, L.d_scale, L.d_shift, L.Cout_p, out.base, out.frame_stride(), out.Ctot, out.off, Hout, Wout,
                      L.ks, L.stride, pad, L.act, total, cq_shift);
        plan_inst(px1 ? "k_conv_direct<true, 1> cq_shift=%d" : "k_conv_direct<true, 4> cq_shift=%d", cq_shift);
        return OG_OK;
    }
    ConvArgs a = y_conv_args(h, L, L.d_w, in, out, res);
    a.n_chunks = L.Cin_p / 32;
    a.H = in.H;
    a.W = in.W;
    a.tiles_x = (in.W + 15) / 16;
    a.tiles_y = (in.H + 7) / 8;
    a.n_spatial = B * a.tiles_x * a.tiles_y;
    const LaunchCtx ctx{h->stream, h->n_cu, 2};
    // THE DETECTOR'S CANONICAL ARITHMETIC (a property of the handle, as the U-Net's is): a conv whose ONE-FRAME launch would leave
    // most of the chip idle sums its K range as `ks` parts, combined in split order -- decided from the layer's shape, the frame
    // size and the handle's options alone, never from B.  One-frame calls (TemporalDetector.detect, detector.py:58) run the parts
    // on separate workgroups (split-K with the fused reduce: the latency path); batched calls (area_waveform) run the whole K range
    // in one workgroup and keep the parts apart in registers (k_conv_mfma_o<..., VS>): the same bits, so `detect(frame)` and
    // `detect_frames(video)[i]` return the same five floats and the truncations of detector.py:68-69,94-95 see the same numbers.
    const bool can_split = h->d_partial && h->d_tile_counter;
    const int NTc = (h->latency_nt1 && L.d_w1) ? 1 : L.NT;   // tile width the one-frame launch would take (same sums either way)
    const int tiles1 = (L.kind == 4) ? ((out.W + 15) / 16) * ((out.H + 7) / 8) : a.tiles_x * a.tiles_y;   // one frame's spatial tiles
    const int chunks = (L.kind == 4) ? 4 * (L.Cin_p / 32) : L.Cin_p / 32;
    const int k_units = (L.kind == 0) ? (chunks * 9) / h->splitk_min_steps : chunks;
    int ks = 1;
    if (can_split) {
        ks = pick_ksplit(tiles1 * (L.Cout_p / (32 * NTc)), k_units, h->n_cu * h->splitk_slots, (NTc == 2) ? 2 : 1, true, h->splitk_div);
        if (ks > h->splitk_max) ks = h->splitk_max;
    }
    const bool latency = can_split && B <= h->latency_batch;   // ("latency_batch" 0: every call takes the batched kernels -- the same bits, later)
    // a real split of this launch must fit the workspace and the counters; otherwise (and for every batched call) the virtual one
    const int NTr = latency ? NTc : L.NT;
    bool real = latency && ks > 1;
    if (real) {
        const long long items = (long long)B * tiles1 * (L.Cout_p / (32 * NTr));
        real = items <= kTileCounters && items * ks * 4 * (((NTr == 2) ? 2 : 1) * 16 * 64) * 4 <= (long long)kPartialBytes;
    }
    const int NTu = (real || (latency && ks == 1)) ? NTc : L.NT;
    if (NTu != L.NT) a.wpk = L.d_w1;
    const int n_ntiles = L.Cout_p / (32 * NTu);
    a.partial = h->d_partial;
    a.tile_counter = h->d_tile_counter;
    if (L.kind == 4) {  // a.H, a.W = output grid; the kernel addresses the (2H x 2W) input through the space-to-depth view
        if (in.H != 2 * out.H || in.W != 2 * out.W) return fail(OG_EINVAL, "stride-2 conv needs even input sizes: " + mod);
        a.H = out.H;
        a.W = out.W;
        a.tiles_x = (out.W + 15) / 16;
        a.tiles_y = (out.H + 7) / 8;
        a.n_spatial = B * a.tiles_x * a.tiles_y;
        a.n_chunks = chunks;
    }
    if (ks > 1 && !real) a.vsplit = ks;   // virtual split: any B, no workspace
    else a.ksplit = real ? ks : 1;
    // launches that fill the chip (3 workgroups per CU) take the occupancy kernel, as in the U-Net chain, and so does every split and
    // every stride-2 conv (MODE 3 exists on that kernel only); the rest run on the persistent one
    const bool occ = a.ksplit > 1 || a.n_spatial * n_ntiles >= h->n_cu;
    return og_pick<2, 1>(NTu, [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        if (a.vsplit > 1) {
            if (L.kind == 4) return launch_conv_o<NT, 3, 8, 3, true>(ctx, a, n_ntiles);
            if (L.kind == 0) return launch_conv_o<NT, 0, 8, 3, true>(ctx, a, n_ntiles);
            return launch_conv_o<NT, 2, 8, 3, true>(ctx, a, n_ntiles);
        }
        if (L.kind == 4) return launch_conv_o<NT, 3, 8, 3>(ctx, a, n_ntiles);
        if (L.kind == 0) return occ ? launch_conv_o<NT, 0, 8, 3>(ctx, a, n_ntiles) : launch_conv_p<NT, 0, 8, (NT == 2) ? 1 : 3>(ctx, a, n_ntiles);
        // 1x1 convs: the occupancy kernel's MODE 2 (no halo border, one tap)
        return occ ? launch_conv_o<NT, 2, 8, 3>(ctx, a, n_ntiles) : launch_conv_p<NT, 2, 8, 1>(ctx, a, n_ntiles);
    });
}

// Channel width of a Conv module's output from its weight shape.
int y_cout(const og_yolo* h, const std::string& wkey) {
    auto it = h->couts.find(wkey);
    return it == h->couts.end() ? -1 : it->second;
}

struct YPlan {  // everything derived from (B,H,W): buffers + named views
    size_t total = 0;
    std::vector<std::pair<std::string, YView>> named;
};

const int kC2fIdx[8] = {2, 4, 6, 8, 12, 15, 18, 21};

}  // namespace

// The forward pass is written once as a template over an "executor" so that the very same
// topology code (a) builds and packs the layers at finalize time and (b) enqueues the launches.
namespace {

struct YNet {
    og_yolo* h;
    int B, H, W;
    int mode;              // 0 BUILD (pack weights, no device work) | 1 PLAN (size the arena) | 2 RUN (launch)
    const uint8_t* in_u8;  // device BGR frames (launch mode)
    size_t bump = 0;       // arena offset (bytes)
    int rc = OG_OK;
    float conf = 0.25f;
    float* pred = nullptr;  // device, optional
    float* best = nullptr;  // device
    int n_anchors = 0;

    // INVARIANT (both modes, vital in f16): the arena is zeroed only when it is (re)allocated, and a buffer's place moves with B.
    // So every byte a conv reads must have been written in THIS run: each producer stores all Cout_p padded channels of every
    // segment (padded columns have zero weights, scale and shift: they store act(0) = 0), pools and up-sampling copy whole padded
    // segments, model.0 in f16 mode stores its padded quads too.  A slot left to stale bytes is multiplied by a zero weight, which
    // is harmless for finite f32 (the f32 model.0) but not for f16: stale f32 logits can read as NaN, and 0 x NaN = NaN in the MFMA.
    YView alloc(int segsC, int Hh, int Ww, bool f32 = false) {  // buffer of `segsC` physical channels (f32: also in f16 mode)
        YView v;
        v.es = (h->precision == 2 && !f32) ? 2 : 1;
        v.Ctot = segsC;
        v.off = 0;
        v.C = segsC;
        v.H = Hh;
        v.W = Ww;
        v.base = (float*)((char*)h->arena + bump);
        bump += ((size_t)B * Hh * Ww * segsC * (sizeof(float) / v.es) + 255) / 256 * 256;
        return v;
    }
    static YView seg(const YView& buf, int off, int C) {
        YView v = buf;
        v.off = off;
        v.C = C;
        return v;
    }
    void conv(const std::string& mod, bool plain, int kind, int stride, int act, const YView& in, const std::vector<YSeg>& in_segs,
              const YView& out, const std::vector<YSeg>& out_segs, const YView* res = nullptr, bool first = false) {
        if (rc || mode == 1) return;
        if (mode == 0) {
            rc = y_build_conv(h, mod, plain, kind, stride, act, in_segs, out_segs);
        } else {
            YView i2 = in;
            i2.off = in_segs.front().off;
            YView o2 = out;
            o2.off = out_segs.front().off;
            g_launch_mod = mod.c_str();
            rc = y_launch(h, mod, B, first ? in_u8 : nullptr, i2, o2, res);
            g_launch_mod = nullptr;
            if (!h->host_only && mod.compare(0, 12, "model.22.hd.") != 0) h->acts[mod] = YAct{out, out_segs};   // every Conv's output by its module path
        }
    }
    void name(const std::string& n, const YView& v) {
        if (mode == 2 && !h->host_only) h->acts[n] = YAct{v, {{v.off, v.C}}};
    }

    // C2f (ultralytics nn/modules/block.py): cv1 1x1 -> split in two -> n Bottlenecks(3x3,3x3) chained on the
    // last piece -> concat all -> cv2 1x1.  `out`/`out_seg`: where the block's result goes.
    void c2f(int idx, int n, bool shortcut, const YView& in, const std::vector<YSeg>& in_segs, int c2, const YView& out, int out_off) {
        const std::string p = "model." + std::to_string(idx);
        const int c = c2 / 2, cp = cp32(c);
        YView cat = alloc((2 + n) * cp, in.H, in.W);
        conv(p + ".cv1", false, 2, 1, 2, in, in_segs, cat, {{0, c}, {cp, c}});
        for (int j = 0; j < n; ++j) {
            const std::string m = p + ".m." + std::to_string(j);
            YView tmp = alloc(cp, in.H, in.W);   // one per bottleneck: every stored tensor stays readable (og_yolo_get_activation)
            YView src = seg(cat, (1 + j) * cp, c);
            conv(m + ".cv1", false, 0, 1, 2, cat, {{(1 + j) * cp, c}}, tmp, {{0, c}});
            conv(m + ".cv2", false, 0, 1, 2, tmp, {{0, c}}, cat, {{(2 + j) * cp, c}}, shortcut ? &src : nullptr);
        }
        std::vector<YSeg> all;
        for (int j = 0; j < 2 + n; ++j) all.push_back({j * cp, c});
        conv(p + ".cv2", false, 2, 1, 2, cat, all, out, {{out_off, c2}});
        name(p, seg(out, out_off, c2));
    }

    void upsample(const char* mod, const YView& in, const YView& out, int out_off) {
        if (rc || mode != 2) return;
        const int C4 = cp32(in.C) / (4 * in.es);   // 16-byte pieces per pixel: 4 f32 or 8 f16 channels
        const long long total = (long long)B * out.H * out.W * C4;
        g_launch_mod = mod;
        rc = [&]() -> int {
            OG_LAUNCH(k_upsample2, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, in.base, in.fs4(),
                      in.ps4(), in.off4(), out.base, out.fs4(), out.ps4(), out_off / out.es, C4, out.H, out.W, total);
            return OG_OK;
        }();
        g_launch_mod = nullptr;
    }

    // the three chained 5x5 max-pools of the SPPF, in place in its concat buffer
    int pools(const YView& sp, int csp, int H5, int W5) {
        if (h->precision == 2) {   // packed f16 max, 8 channels per thread; one-frame calls take it too
            const long long total = (long long)B * H5 * W5 * (csp / 8);
            for (int j = 0; j < 3; ++j) {
                const std::string m = "model.9.m." + std::to_string(j + 1);
                g_launch_mod = m.c_str();
                OG_LAUNCH(k_maxpool5_h, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, sp.base, sp.base,
                          sp.fs4(), sp.ps4(), j * csp / 2, (j + 1) * csp / 2, csp / 8, H5, W5, total);
            }
        } else if (B <= h->latency_batch && H5 * W5 <= 224) {   // one launch: the map's 32-channel slabs pooled in LDS
            g_launch_mod = "model.9.m.1-3";
            OG_LAUNCH(k_sppf_pools, dim3(csp / 32, B), dim3(256), (size_t)H5 * W5 * 256, h->stream, sp.base, sp.frame_stride(), sp.Ctot, csp, H5, W5);
        } else {
            const long long total = (long long)B * H5 * W5 * (csp / 4);
            for (int j = 0; j < 3; ++j) {
                const std::string m = "model.9.m." + std::to_string(j + 1);
                g_launch_mod = m.c_str();
                OG_LAUNCH(k_maxpool5, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, sp.base, sp.base,
                          sp.frame_stride(), sp.Ctot, j * csp, (j + 1) * csp, csp / 4, H5, W5, total);
            }
        }
        return OG_OK;
    }

    int decode(const YoloDecodeArgs& da) {
        g_launch_mod = "model.22";
        if (B <= h->latency_batch && h->d_cand && (da.n_anchors + 63) / 64 <= og_yolo::kDecBlocks)
            OG_LAUNCH(k_yolo_decode_mb, dim3((da.n_anchors + 63) / 64, B), dim3(256), 0, h->stream, da, h->d_cand, h->d_dec_counter);
        else
            OG_LAUNCH(k_yolo_decode, dim3(B), dim3(256), 0, h->stream, da);
        return OG_OK;
    }

    void run() {
        auto ch = [&](const std::string& k) { return y_cout(h, k); };
        const int c0 = ch("model.0.conv.weight"), c1 = ch("model.1.conv.weight"), c3 = ch("model.3.conv.weight"),
                  c5 = ch("model.5.conv.weight"), c7 = ch("model.7.conv.weight");
        const int c12 = ch("model.12.cv2.conv.weight"), c15 = ch("model.15.cv2.conv.weight"), c18 = ch("model.18.cv2.conv.weight"),
                  c21 = ch("model.21.cv2.conv.weight"), c16 = ch("model.16.conv.weight"), c19 = ch("model.19.conv.weight");
        if (c0 < 0 || c1 < 0 || c3 < 0 || c5 < 0 || c7 < 0 || c12 < 0 || c15 < 0 || c18 < 0 || c21 < 0 || c16 != c15 || c19 != c18) {
            rc = fail(OG_EINVAL, "incomplete YOLOv8 state_dict (backbone/neck conv weights missing)");
            return;
        }
        const int H1 = H / 2, W1 = W / 2, H2 = H / 4, W2 = W / 4, H3 = H / 8, W3 = W / 8, H4 = H / 16, W4 = W / 16, H5 = H / 32, W5 = W / 32;
        YView in0;  // the u8 frame (only H, W used)
        in0.H = H;
        in0.W = W;
        // ---- backbone ----
        YView t0 = alloc(cp32(c0), H1, W1);
        conv("model.0", false, 3, 2, 2, in0, {{0, 3}}, t0, {{0, c0}}, nullptr, true);
        name("model.0", seg(t0, 0, c0));
        YView t1 = alloc(cp32(c1), H2, W2);
        conv("model.1", false, 4, 2, 2, t0, {{0, c0}}, t1, {{0, c1}});
        name("model.1", seg(t1, 0, c1));
        YView t2 = alloc(cp32(c1), H2, W2);
        c2f(2, h->n_c2f[0], true, t1, {{0, c1}}, c1, t2, 0);
        YView t3 = alloc(cp32(c3), H3, W3);
        conv("model.3", false, 4, 2, 2, t2, {{0, c1}}, t3, {{0, c3}});
        name("model.3", seg(t3, 0, c3));
        // concat buffers of the neck, laid out [upsampled | lateral] (Concat([up, backbone]) order)
        YView cat14 = alloc(cp32(c12) + cp32(c3), H3, W3);   // [up(12) , 4]
        c2f(4, h->n_c2f[1], true, t3, {{0, c3}}, c3, cat14, cp32(c12));
        YView t4 = seg(cat14, cp32(c12), c3);
        YView t5 = alloc(cp32(c5), H4, W4);
        conv("model.5", false, 4, 2, 2, t4, {{t4.off, c3}}, t5, {{0, c5}});
        name("model.5", seg(t5, 0, c5));
        YView cat11 = alloc(cp32(c7) + cp32(c5), H4, W4);     // [up(9), 6]
        c2f(6, h->n_c2f[2], true, t5, {{0, c5}}, c5, cat11, cp32(c7));
        YView t6 = seg(cat11, cp32(c7), c5);
        YView t7 = alloc(cp32(c7), H5, W5);
        conv("model.7", false, 4, 2, 2, t6, {{t6.off, c5}}, t7, {{0, c7}});
        name("model.7", seg(t7, 0, c7));
        YView t8 = alloc(cp32(c7), H5, W5);
        c2f(8, h->n_c2f[3], true, t7, {{0, c7}}, c7, t8, 0);
        // ---- SPPF (model.9): cv1 1x1 -> 3 chained 5x5 max-pools -> concat 4 -> cv2 1x1 ----
        const int cs = c7 / 2, csp = cp32(cs);
        YView sp = alloc(4 * csp, H5, W5);
        conv("model.9.cv1", false, 2, 1, 2, t8, {{0, c7}}, sp, {{0, cs}});
        if (!rc && mode == 2) {
            rc = pools(sp, csp, H5, W5);
            g_launch_mod = nullptr;
        }
        for (int j = 1; j <= 3; ++j) name("model.9.m." + std::to_string(j), seg(sp, j * csp, cs));   // the three chained pools
        YView cat20 = alloc(cp32(c18) + cp32(c7), H5, W5);    // [19, 9]
        conv("model.9.cv2", false, 2, 1, 2, sp, {{0, cs}, {csp, cs}, {2 * csp, cs}, {3 * csp, cs}}, cat20, {{cp32(c18), c7}});
        YView t9 = seg(cat20, cp32(c18), c7);
        name("model.9", t9);
        // ---- neck ----
        upsample("model.10", t9, cat11, 0);
        name("model.10", seg(cat11, 0, c7));
        YView cat17 = alloc(cp32(c15) + cp32(c12), H4, W4);   // [16, 12]
        c2f(12, h->n_c2f[4], false, cat11, {{0, c7}, {cp32(c7), c5}}, c12, cat17, cp32(c15));
        YView t12 = seg(cat17, cp32(c15), c12);
        upsample("model.13", t12, cat14, 0);
        name("model.13", seg(cat14, 0, c12));
        // ---- Detect (model.22): per level a box branch (-> 4*reg_max DFL logits) and a class branch, three convs each;
        //      one-frame calls run the two branches as one chain of three (y_synth_head)
        const bool fused = h->head_fused;   // every B: the stacked chain has other K-part boundaries than the two branch chains (canonical form)
        YoloDecodeArgs da;
        da.n_anchors = 0;
        auto head = [&](int l, const YView& x, int cx) {
            if (rc) return;
            const std::string pb = "model.22.cv2." + std::to_string(l), pc = "model.22.cv3." + std::to_string(l);
            const int cb = ch(pb + ".0.conv.weight"), cc = ch(pc + ".0.conv.weight");
            const int nb = ch(pb + ".2.weight"), ncls = ch(pc + ".2.weight");
            if (cb < 0 || cc < 0 || nb != 4 * h->reg_max || ncls != h->nc) {
                rc = fail(OG_EINVAL, "Detect head tensors missing or of unexpected shape (need reg_max 16, nc " + std::to_string(h->nc) + ")");
                return;
            }
            da.lv[l].h = x.H;
            da.lv[l].w = x.W;
            da.lv[l].stride = (float)(H / x.H);
            da.n_anchors += x.H * x.W;
            if (h->head_synth && (mode == 0 || (fused && mode == 2))) {   // BUILD packs both forms
                const std::string ph = "model.22.hd." + std::to_string(l);
                const int cbp = cp32(cb), nbp = cp32(nb);
                YView h1 = alloc(cbp + cp32(cc), x.H, x.W), h2 = alloc(cbp + cp32(cc), x.H, x.W), ho = alloc(nbp + cp32(ncls), x.H, x.W, true);
                conv(ph + ".0", false, 0, 1, 2, x, {{0, cx}}, h1, {{0, cb}, {cbp, cc}});
                conv(ph + ".1", false, 0, 1, 2, h1, {{0, cb}, {cbp, cc}}, h2, {{0, cb}, {cbp, cc}});
                conv(ph + ".2", true, 2, 1, 0, h2, {{0, cb}, {cbp, cc}}, ho, {{0, nb}, {nbp, ncls}});
                if (mode == 2) {   // the stacked chain's two channel segments, by their branch paths
                    name(pb + ".0", seg(h1, 0, cb));
                    name(pc + ".0", seg(h1, cbp, cc));
                    name(pb + ".1", seg(h2, 0, cb));
                    name(pc + ".1", seg(h2, cbp, cc));
                    name(pb + ".2", seg(ho, 0, nb));
                    name(pc + ".2", seg(ho, nbp, ncls));
                }
                name("box" + std::to_string(l), seg(ho, 0, nb));
                name("cls" + std::to_string(l), seg(ho, nbp, ncls));
                da.lv[l].box = ho.base;
                da.lv[l].cls = ho.base + nbp;
                da.lv[l].box_frame_stride = da.lv[l].cls_frame_stride = ho.frame_stride();
                da.lv[l].box_pix_stride = da.lv[l].cls_pix_stride = ho.Ctot;
                if (mode == 2) return;
            }
            YView b1 = alloc(cp32(cb), x.H, x.W), b2 = alloc(cp32(cb), x.H, x.W), bo = alloc(cp32(nb), x.H, x.W, true);
            YView k1 = alloc(cp32(cc), x.H, x.W), k2 = alloc(cp32(cc), x.H, x.W), ko = alloc(cp32(ncls), x.H, x.W, true);
            conv(pb + ".0", false, 0, 1, 2, x, {{0, cx}}, b1, {{0, cb}});
            conv(pb + ".1", false, 0, 1, 2, b1, {{0, cb}}, b2, {{0, cb}});
            conv(pb + ".2", true, 2, 1, 0, b2, {{0, cb}}, bo, {{0, nb}});
            conv(pc + ".0", false, 0, 1, 2, x, {{0, cx}}, k1, {{0, cc}});
            conv(pc + ".1", false, 0, 1, 2, k1, {{0, cc}}, k2, {{0, cc}});
            conv(pc + ".2", true, 2, 1, 0, k2, {{0, cc}}, ko, {{0, ncls}});
            name("box" + std::to_string(l), seg(bo, 0, nb));
            name("cls" + std::to_string(l), seg(ko, 0, ncls));
            da.lv[l].box = bo.base;
            da.lv[l].cls = ko.base;
            da.lv[l].box_frame_stride = bo.frame_stride();
            da.lv[l].cls_frame_stride = ko.frame_stride();
            da.lv[l].box_pix_stride = bo.Ctot;
            da.lv[l].cls_pix_stride = ko.Ctot;
        };
        YView t15 = alloc(cp32(c15), H3, W3);
        c2f(15, h->n_c2f[5], false, cat14, {{0, c12}, {cp32(c12), c3}}, c15, t15, 0);
        head(0, t15, c15);
        conv("model.16", false, 4, 2, 2, t15, {{0, c15}}, cat17, {{0, c16}});
        name("model.16", seg(cat17, 0, c16));
        YView t18 = alloc(cp32(c18), H4, W4);
        c2f(18, h->n_c2f[6], false, cat17, {{0, c16}, {cp32(c15), c12}}, c18, t18, 0);
        head(1, t18, c18);
        conv("model.19", false, 4, 2, 2, t18, {{0, c18}}, cat20, {{0, c19}});
        name("model.19", seg(cat20, 0, c19));
        YView t21 = alloc(cp32(c21), H5, W5);
        c2f(21, h->n_c2f[7], false, cat20, {{0, c19}, {cp32(c18), c7}}, c21, t21, 0);
        head(2, t21, c21);
        n_anchors = da.n_anchors;
        if (rc || mode != 2) return;
        da.conf_thres = conf;
        da.img_w = (float)W;
        da.img_h = (float)H;
        da.pred = pred;
        da.best = best;
        rc = decode(da);
        g_launch_mod = nullptr;
    }
};

}  // namespace

namespace {

int y_ensure_arena(og_yolo* h, int B, int H, int W) {
    if (h->arena && B <= h->capB && H == h->aH && W == h->aW) return OG_OK;
    if (h->arena) {
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipFree(h->arena));
        h->arena = nullptr;
        h->acts.clear();
    }
    YNet plan{h, B, H, W, 1, nullptr};
    plan.run();
    if (plan.rc) return plan.rc;
    HIPCHK(hipMalloc(&h->arena, plan.bump + 256));
    HIPCHK(hipMemsetAsync(h->arena, 0, plan.bump + 256, h->stream));  // padded channels must stay finite (x0 weights)
    h->capB = B;
    h->aH = H;
    h->aW = W;
    return OG_OK;
}

int y_check(og_yolo* h, int B, int H, int W) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (!h->finalized) return fail(OG_ESTATE, "og_yolo_finalize() has not been called");
    if (B < 0 || H <= 0 || W <= 0 || H % 32 || W % 32)
        return fail(OG_EINVAL, "H and W must be positive multiples of 32 (letterbox on the host first)");
    return OG_OK;
}

// f16 mode: did any activation leave the f16 range since the last check?  Call after the work has completed.
int y_check_range(og_yolo* h) {
    if (h->h_range && *(volatile int*)h->h_range) {
        *(volatile int*)h->h_range = 0;
        return fail(OG_ERANGE, "detector f16 mode: an activation exceeded the f16 range (|v| > 60000); the result of this call is not "
                               "valid.  Use \"precision\" 0 for these weights");
    }
    return OG_OK;
}

int y_stage(og_yolo* h, size_t bytes) {
    if (bytes <= h->stage_bytes) return OG_OK;
    if (h->stage) {
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipFree(h->stage));
        h->stage = nullptr;
    }
    HIPCHK(hipMalloc(&h->stage, bytes));
    h->stage_bytes = bytes;
    return OG_OK;
}

}  // namespace

extern "C" {

og_yolo* og_yolo_create(int nc) {
    if (nc < 1 || nc > 80) {
        fail(OG_EINVAL, "nc out of range");
        return nullptr;
    }
    og_yolo* h = new og_yolo();
    h->nc = nc;
    return h;
}

void og_yolo_destroy(og_yolo* h) {
    if (!h) return;
    if (h->plan_copy) og_yolo_destroy(h->plan_copy);
    if (h->host_only) {   // placeholders only: nothing to release on any device
        delete h;
        return;
    }
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& kv : h->convs)
        for (float* p : {kv.second.d_w, kv.second.d_w1, kv.second.d_wf, kv.second.d_scale, kv.second.d_shift})
            if (p) (void)hipFree(p);
    if (h->arena) (void)hipFree(h->arena);
    if (h->stage) (void)hipFree(h->stage);
    if (h->d_zero) (void)hipFree(h->d_zero);
    if (h->d_partial) (void)hipFree(h->d_partial);
    if (h->d_tile_counter) (void)hipFree(h->d_tile_counter);
    if (h->d_cand) (void)hipFree(h->d_cand);
    if (h->d_dec_counter) (void)hipFree(h->d_dec_counter);
    if (h->pin) (void)hipHostFree(h->pin);
    if (h->h_range) (void)hipHostFree(h->h_range);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int og_yolo_set_tensor(og_yolo* h, const char* key, const void* host, const int64_t* shape, int ndim, int dtype) {
    if (!h || !key || !host) return fail(OG_EINVAL, "null argument");
    if (h->finalized) return fail(OG_ESTATE, "handle already finalized");
    const std::string k(key);
    if (k.rfind("model.", 0) != 0) return fail(OG_EINVAL, "unexpected key " + k + " (ultralytics keys start with 'model.')");
    if (dtype == OG_DTYPE_I64) return OG_OK;  // num_batches_tracked: accepted, ignored
    if (dtype != OG_DTYPE_F32) return fail(OG_EINVAL, "tensor " + k + " must be float32");
    if (ndim < 0 || ndim > 4 || (ndim > 0 && !shape)) return fail(OG_EINVAL, "bad shape for " + k);
    HostTensor t;
    t.shape.assign(shape, shape + ndim);
    size_t n = 1;
    for (auto v : t.shape) {
        if (v <= 0) return fail(OG_EINVAL, "bad shape for " + k);
        n *= (size_t)v;
    }
    t.data.assign((const float*)host, (const float*)host + n);
    h->host[k] = std::move(t);
    if (h->plan_copy) {
        og_yolo_destroy(h->plan_copy);
        h->plan_copy = nullptr;
    }
    return OG_OK;
}

int og_yolo_finalize(og_yolo* h) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (h->finalized) return OG_OK;
    for (int i = 0; i < 8; ++i) {  // C2f depth = number of m.{j} bottlenecks present
        int n = 0;
        while (yhas(h, "model." + std::to_string(kC2fIdx[i]) + ".m." + std::to_string(n) + ".cv1.conv.weight")) ++n;
        if (n < 1) return fail(OG_EINVAL, "C2f block model." + std::to_string(kC2fIdx[i]) + " has no bottleneck weights");
        h->n_c2f[i] = n;
    }
    if (yhas(h, "model.22.dfl.conv.weight")) {  // fixed arange(reg_max) in ultralytics; verify rather than trust
        const auto& d = h->host.at("model.22.dfl.conv.weight");
        if ((int)d.data.size() != h->reg_max) return fail(OG_EINVAL, "only reg_max = 16 is implemented");
        for (int i = 0; i < h->reg_max; ++i)
            if (d.data[i] != (float)i) return fail(OG_EINVAL, "model.22.dfl.conv.weight is not arange(16)");
    }
    int rc;
    if (h->host_only) {   // og_yolo_plan: no device -- every workspace "exists", upload() hands out placeholders (y_build_conv packs nothing)
        h->d_zero = (float*)8;
        h->d_partial = (float*)8;
        h->d_tile_counter = (int*)8;
        h->d_cand = (float*)8;
        h->d_dec_counter = (int*)8;
        h->d_range = (int*)8;
        h->head_synth = y_synth_head(h);
        for (auto& kv : h->host)
            if (!kv.second.shape.empty()) h->couts[kv.first] = (int)kv.second.shape[0];
        YNet b{h, 1, 32, 32, 0, nullptr};
        b.run();
        if (b.rc) return b.rc;
        h->host.clear();
        h->finalized = true;
        return OG_OK;
    }
    if ((rc = init_kernel_attrs())) return rc;
    {
        int dev = 0;
        hipDeviceProp_t prop;
        HIPCHK(hipGetDevice(&dev));
        HIPCHK(hipGetDeviceProperties(&prop, dev));
        h->device = dev;
        h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HIPCHK(hipMalloc((void**)&h->d_zero, 4096));
    HIPCHK(hipMemset(h->d_zero, 0, 4096));
    HIPCHK(hipMalloc((void**)&h->d_partial, kPartialBytes));
    HIPCHK(hipMalloc((void**)&h->d_tile_counter, 4096 * sizeof(int)));
    HIPCHK(hipMemset(h->d_tile_counter, 0, 4096 * sizeof(int)));
    HIPCHK(hipMalloc((void**)&h->d_cand, (size_t)64 * og_yolo::kDecBlocks * 8 * sizeof(float)));
    HIPCHK(hipMalloc((void**)&h->d_dec_counter, 64 * sizeof(int)));
    HIPCHK(hipMemset(h->d_dec_counter, 0, 64 * sizeof(int)));
    HIPCHK(hipHostMalloc((void**)&h->h_range, sizeof(int), hipHostMallocMapped));
    *h->h_range = 0;
    HIPCHK(hipHostGetDevicePointer((void**)&h->d_range, h->h_range, 0));
    h->head_synth = y_synth_head(h);
    for (auto& kv : h->host)
        if (!kv.second.shape.empty()) h->couts[kv.first] = (int)kv.second.shape[0];
    YNet b{h, 1, 32, 32, 0, nullptr};
    b.run();
    if (b.rc) return b.rc;
    h->host.clear();
    h->finalized = true;
    return OG_OK;
}

int og_yolo_set_option(og_yolo* h, const char* name, int value) {
    if (!h || !name) return fail(OG_EINVAL, "null argument");
    const std::string n(name);
    int* slot = nullptr;
    if (n == "latency_batch" && value >= 0 && value <= 64) slot = &h->latency_batch;
    else if (n == "zero_copy" && (value == 0 || value == 1)) slot = &h->zero_copy;
    else if (n == "head_fused" && (value == 0 || value == 1)) slot = &h->head_fused;
    else if (n == "latency_nt1" && (value == 0 || value == 1)) slot = &h->latency_nt1;
    else if (n == "splitk_max" && value >= 1 && value <= 64) slot = &h->splitk_max;
    else if (n == "splitk_min_steps" && (value == 1 || value == 3 || value == 9)) slot = &h->splitk_min_steps;
    else if (n == "splitk_slots" && value >= 1 && value <= 4) slot = &h->splitk_slots;
    else if (n == "splitk_div" && value >= 1 && value <= 8) slot = &h->splitk_div;
    else if (n == "precision" && (value == 0 || value == 2)) slot = &h->precision;   // (no split precision, 1, for the detector)
    else if (n == "source_stage_kib" && value >= 1 && value <= (1 << 24)) slot = &h->source_stage_kib;
    else if (n == "source_mapped" && (value == 0 || value == 1)) slot = &h->source_mapped;
    else if (n == "trace_launches" && (value == 0 || value == 1)) slot = &h->trace_launches;
    if (!slot) return fail(OG_EINVAL, "unknown detector option or value out of range: " + n);
    if (h->stream) HIPCHK(hipStreamSynchronize(h->stream));
    if (slot == &h->precision && value != h->precision && h->arena) {   // other buffer sizes: the next call plans the arena anew
        HIPCHK(hipFree(h->arena));
        h->arena = nullptr;
        h->capB = 0;
        h->acts.clear();
    }
    *slot = value;
    return OG_OK;
}

int og_yolo_plan(og_yolo* h, int B, int H, int W, int n_cu, const char* options, char* out, size_t cap, long long* arena_bytes) {
    if (!h || !out || cap == 0 || B < 1 || n_cu < 0) return fail(OG_EINVAL, "bad argument");
    if (h->finalized) return fail(OG_ESTATE, "og_yolo_plan takes a handle that has its tensors and is not finalized");
    if (H <= 0 || W <= 0 || H % 32 || W % 32) return fail(OG_EINVAL, "H and W must be positive multiples of 32 (letterbox on the host first)");
    // a host-only copy: the options and the tensors' SHAPES (no launch decision reads a weight)
    int rc = OG_OK;
    if (!h->plan_copy) {
        og_yolo* c0 = new og_yolo();
        c0->host_only = true;
        c0->nc = h->nc;
        c0->reg_max = h->reg_max;
        for (auto& kv : h->host) {
            if (kv.first == "model.22.dfl.conv.weight") continue;   // (values, checked by the real finalize)
            c0->host[kv.first].shape = kv.second.shape;
        }
        if ((rc = og_yolo_finalize(c0))) {
            og_yolo_destroy(c0);
            return rc;
        }
        h->plan_copy = c0;
    }
    og_yolo* c = h->plan_copy;
    c->latency_batch = h->latency_batch;
    c->zero_copy = h->zero_copy;
    c->splitk_slots = h->splitk_slots;
    c->splitk_div = h->splitk_div;
    c->splitk_max = h->splitk_max;
    c->splitk_min_steps = h->splitk_min_steps;
    c->latency_nt1 = h->latency_nt1;
    c->head_fused = h->head_fused;
    c->precision = h->precision;
    c->arena = nullptr;
    c->acts.clear();
    c->n_cu = n_cu > 0 ? n_cu : 256;
    std::string opt = options ? options : "";
    for (size_t p0 = 0; !rc && p0 < opt.size();) {   // "name=value,name=value"
        size_t p1 = opt.find(',', p0);
        if (p1 == std::string::npos) p1 = opt.size();
        const std::string kv = opt.substr(p0, p1 - p0);
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) rc = fail(OG_EINVAL, "option without '=': " + kv);
        else rc = og_yolo_set_option(c, kv.substr(0, eq).c_str(), atoi(kv.c_str() + eq + 1));
        p0 = p1 + 1;
    }
    Plan plan;
    if (!rc) {
        constexpr int kMaxLaunch = 512;   // og_yolo_detect_u8_dev's: the first chain of a larger call
        const int nb = B < kMaxLaunch ? B : kMaxLaunch;
        if (arena_bytes) {   // (the sizing pass of y_ensure_arena; the chain below makes the same checks)
            YNet size{c, nb, H, W, 1, nullptr};
            size.run();
            rc = size.rc;
            *arena_bytes = (long long)size.bump + 256;
        }
        if (!rc) {
            c->arena = (void*)4096;   // a placeholder base: nothing dereferences it in a dry run
            g_plan = &plan;
            YNet run{c, nb, H, W, 2, (const uint8_t*)4096};
            run.best = (float*)4096;
            run.pred = (float*)4096;
            run.run();
            g_plan = nullptr;
            g_launch_mod = nullptr;
            rc = run.rc;
        }
    }
    c->arena = nullptr;
    if (rc) return rc;
    return og_plan_text(plan, kPlanMod, out, cap);
}

int og_yolo_last_launches(og_yolo* h, char* out, size_t cap) {
    if (!h || !out || cap == 0) return fail(OG_EINVAL, "bad argument");
    std::string txt;
    for (auto& r : h->last_launches) txt += r.first + "|" + r.second + "\n";
    if (txt.size() + 1 > cap) return fail(OG_EINVAL, "launch list does not fit the buffer");
    memcpy(out, txt.c_str(), txt.size() + 1);
    return (int)h->last_launches.size();
}

int og_yolo_num_anchors(og_yolo* h, int H, int W) {
    if (!h || H % 32 || W % 32 || H <= 0 || W <= 0) return fail(OG_EINVAL, "bad argument");
    return (H / 8) * (W / 8) + (H / 16) * (W / 16) + (H / 32) * (W / 32);
}

int og_yolo_detect_u8_dev(og_yolo* h, const uint8_t* bgr_dev, int B, int H, int W, float conf, float* best_dev, float* pred_dev) {
    OG_SCOPE(h);
    int rc = y_check(h, B, H, W);
    if (rc) return rc;
    if (B == 0) return OG_OK;
    if (!bgr_dev || !best_dev) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(best_dev);
    OG_ALIGN(pred_dev);
    // at most kMaxLaunch frames per kernel chain: bounds the arena and keeps the conv kernels' grid.z (frame x column
    // tile) inside 16 bits; callers may pass any B
    constexpr int kMaxLaunch = 512;
    const int cap = B < kMaxLaunch ? B : kMaxLaunch;
    if ((rc = y_ensure_arena(h, cap > h->capB ? cap : h->capB, H, W))) return rc;
    const int A = og_yolo_num_anchors(h, H, W);
    for (int b0 = 0; b0 < B; b0 += kMaxLaunch) {
        const int nb = B - b0 < kMaxLaunch ? B - b0 : kMaxLaunch;
        YNet run{h, nb, H, W, 2, bgr_dev + (size_t)b0 * H * W * 3};
        run.conf = conf;
        run.best = best_dev + (size_t)b0 * 5;
        run.pred = pred_dev ? pred_dev + (size_t)b0 * A * 5 : nullptr;
        if (h->trace_launches) {
            h->last_launches.clear();
            g_trace = &h->last_launches;
        }
        run.run();
        g_trace = nullptr;
        h->lastB = nb;
        if (run.rc) return run.rc;
    }
    return OG_OK;
}

// The asynchronous form of the one-frame call (detector.py:58): begin stages the frame in the handle's pinned buffer and enqueues the
// chain on the handle's stream, end waits for it and delivers the best boxes.  Between the two the caller is free to run something
// else -- in the reference's frame loop (features.py:235-245) the U-Net pass of the SAME frame, which does not depend on the box.
int og_yolo_detect_u8_begin(og_yolo* h, const uint8_t* bgr, int B, int H, int W, float conf) {
    OG_SCOPE(h);
    int rc = y_check(h, B, H, W);
    if (rc) return rc;
    if (h->pend_B) return fail(OG_EINVAL, "og_yolo_detect_u8_begin: a call is already in flight on this handle");
    if (B == 0) return OG_OK;
    if (!bgr) return fail(OG_EINVAL, "null buffer");
    h->pend_resized = false;
    const size_t n_in = (size_t)B * H * W * 3, o_best = al256(n_in), tot = o_best + al256((size_t)B * 5 * 4);
    if (B <= h->latency_batch && h->zero_copy) {
        if (tot > h->pin_bytes) {
            if (h->pin) {
                HIPCHK(hipStreamSynchronize(h->stream));
                HIPCHK(hipHostFree(h->pin));
                h->pin = nullptr;
                h->pin_bytes = 0;
            }
            HIPCHK(hipHostMalloc(&h->pin, tot, hipHostMallocDefault));
            h->pin_bytes = tot;
        }
        char* ps = (char*)h->pin;
        memcpy(ps, bgr, n_in);
        char* zp = nullptr;
        HIPCHK(hipHostGetDevicePointer((void**)&zp, ps, 0));
        rc = og_yolo_detect_u8_dev(h, (const uint8_t*)zp, B, H, W, conf, (float*)(zp + o_best), nullptr);
        if (rc) return rc;
        h->pend_sync = false;
    } else {   // larger calls / "zero_copy" 0: nothing to overlap with -- run now, deliver at end
        h->pend_best.resize((size_t)B * 5);
        rc = og_yolo_detect_u8(h, bgr, B, H, W, conf, h->pend_best.data(), nullptr);
        if (rc) return rc;
        h->pend_sync = true;
    }
    h->pend_B = B;
    h->pend_off = o_best;
    return OG_OK;
}

int og_yolo_detect_u8_end(og_yolo* h, float* best) {
    OG_SCOPE(h);
    if (!h || !h->pend_B) return fail(OG_EINVAL, "og_yolo_detect_u8_end: no call in flight");
    OG_ALIGN(best);   // (refused with the call still in flight: a second og_yolo_detect_u8_end with a good pointer delivers it)
    const int B = h->pend_B;
    h->pend_B = 0;
    if (!best) return fail(OG_EINVAL, "null buffer");
    if (h->pend_sync) {
        memcpy(best, h->pend_best.data(), (size_t)B * 5 * 4);
        return OG_OK;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(best, (char*)h->pin + h->pend_off, (size_t)B * 5 * 4);
    if (h->pend_resized)   // og_yolo_detect_resized_u8_begin: network pixels -> source pixels
        for (int b = 0; b < B; ++b) og_scale_box(best + (size_t)b * 5, h->pend_scale, h->pend_gain, h->pend_left, h->pend_top, h->pend_H, h->pend_W);
    return y_check_range(h);
}

int og_yolo_detect_u8(og_yolo* h, const uint8_t* bgr, int B, int H, int W, float conf, float* best, float* pred) {
    OG_SCOPE(h);
    int rc = y_check(h, B, H, W);
    if (rc) return rc;
    if (B == 0) return OG_OK;
    if (!bgr || !best) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(best);
    OG_ALIGN(pred);
    if (h->pend_B) return fail(OG_EINVAL, "og_yolo_detect_u8: a begin / end call is in flight on this handle");
    const int A = og_yolo_num_anchors(h, H, W);
    const size_t n_in = (size_t)B * H * W * 3, o_best = al256(n_in), o_pred = o_best + al256((size_t)B * 5 * 4),
                 tot = o_pred + (pred ? al256((size_t)B * A * 5 * 4) : 0);
    if ((rc = y_stage(h, tot))) return rc;
    char* s = (char*)h->stage;
    if (B <= h->latency_batch) {
        // latency path: the frame goes through a pinned buffer so that both copies are truly asynchronous and the host
        // waits exactly once (a pageable hipMemcpyAsync blocks until its staging copy is done: two more host wake-ups)
        if (tot > h->pin_bytes) {
            if (h->pin) {
                HIPCHK(hipStreamSynchronize(h->stream));
                HIPCHK(hipHostFree(h->pin));
                h->pin = nullptr;
                h->pin_bytes = 0;
            }
            HIPCHK(hipHostMalloc(&h->pin, tot, hipHostMallocDefault));
            h->pin_bytes = tot;
        }
        char* ps = (char*)h->pin;
        memcpy(ps, bgr, n_in);
        if (h->zero_copy && !pred) {
            // each copy command costs a launch floor (~5 us) on the one stream of a 58-launch chain: the first conv reads the frame
            // from, and the decode writes the 5 floats per frame to, the pinned buffer itself (mapped into the device's address space)
            char* zp = nullptr;
            HIPCHK(hipHostGetDevicePointer((void**)&zp, ps, 0));
            rc = og_yolo_detect_u8_dev(h, (const uint8_t*)zp, B, H, W, conf, (float*)(zp + o_best), nullptr);
            if (rc) return rc;
            HIPCHK(hipStreamSynchronize(h->stream));
            memcpy(best, ps + o_best, (size_t)B * 5 * 4);
            return y_check_range(h);
        }
        HIPCHK(hipMemcpyAsync(s, ps, n_in, hipMemcpyHostToDevice, h->stream));
        rc = og_yolo_detect_u8_dev(h, (const uint8_t*)s, B, H, W, conf, (float*)(s + o_best), pred ? (float*)(s + o_pred) : nullptr);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(ps + o_best, s + o_best, tot - o_best, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        memcpy(best, ps + o_best, (size_t)B * 5 * 4);
        if (pred) memcpy(pred, ps + o_pred, (size_t)B * A * 5 * 4);
        return y_check_range(h);
    }
    const int chunk = 256;  // the detector's maps are tiny (8x8 at the deepest level): big micro-batches fill the chip (18k -> 35k fps)
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = B - b0 < chunk ? B - b0 : chunk;
        HIPCHK(hipMemcpyAsync(s + (size_t)b0 * H * W * 3, bgr + (size_t)b0 * H * W * 3, (size_t)nb * H * W * 3, hipMemcpyHostToDevice, h->stream));
        rc = og_yolo_detect_u8_dev(h, (const uint8_t*)s + (size_t)b0 * H * W * 3, nb, H, W, conf, (float*)(s + o_best) + (size_t)b0 * 5,
                                   pred ? (float*)(s + o_pred) + (size_t)b0 * A * 5 : nullptr);
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(best, s + o_best, (size_t)B * 5 * 4, hipMemcpyDeviceToHost, h->stream));
    if (pred) HIPCHK(hipMemcpyAsync(pred, s + o_pred, (size_t)B * A * 5 * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return y_check_range(h);
}

}  // extern "C"

// ---- frames of any size: letterbox on the device (DESIGN section 12) ----
namespace {

struct YGeo {
    int net_h = 0, net_w = 0, new_h = 0, new_w = 0, top = 0, left = 0;
    double gain = 1.0;
    bool scale() const { return !(gain == 1.0 && left == 0 && top == 0); }   // detect_frames_host's `(gain, px, py) != (1.0, 0, 0)`
};

// argument checks of every resized entry, before the handle's state is looked at (so they can be tested without a device)
int y_check_resized(og_yolo* h, int B, int H, int W, int channels, int imgsz, YGeo& g) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (B < 0) return fail(OG_EINVAL, "negative batch size");
    if (channels != 1 && channels != 3) return fail(OG_EINVAL, "channels must be 1 (gray) or 3 (BGR)");
    int rc = og_yolo_letterbox_geometry(H, W, imgsz, &g.net_h, &g.net_w, &g.new_h, &g.new_w, &g.top, &g.left, &g.gain);
    if (rc) return rc;
    if (!h->finalized) return fail(OG_ESTATE, "og_yolo_finalize() has not been called");
    return OG_OK;
}

// nb <= 32768 frames src [nb,H,W,C] -> out [nb,net_h,net_w,3], on the handle's stream
int y_letterbox(og_yolo* h, const uint8_t* src, int nb, int H, int W, int channels, const YGeo& g, uint8_t* out) {
    const dim3 grid((unsigned)((g.net_h * g.net_w + 255) / 256), (unsigned)nb);
    if (channels == 3)
        OG_LAUNCH(k_letterbox_bgr<3>, grid, dim3(256), 0, h->stream, src, H, W, g.net_h, g.net_w, g.new_h, g.new_w, g.top, g.left, out);
    else
        OG_LAUNCH(k_letterbox_bgr<1>, grid, dim3(256), 0, h->stream, src, H, W, g.net_h, g.net_w, g.new_h, g.new_w, g.top, g.left, out);
    ++h->n_letterbox;
    return OG_OK;
}

int y_pin(og_yolo* h, size_t bytes) {
    if (bytes <= h->pin_bytes) return OG_OK;
    if (h->pin) {
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipHostFree(h->pin));
        h->pin = nullptr;
        h->pin_bytes = 0;
    }
    HIPCHK(hipHostMalloc(&h->pin, bytes, hipHostMallocDefault));
    h->pin_bytes = bytes;
    return OG_OK;
}

// an error inside a resized call: nothing of it stays in flight when the code is returned (the message survives the wait)
int y_fail_sync(og_yolo* h, int rc) {
    const std::string err = g_err;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    g_err = err;
    return rc;
}

constexpr int kNetLaunch = 256;   // network frames per launch of a resized call, whatever the source size (og_yolo_detect_u8's chunk)
constexpr int kBestRows = 65536;  // `best` rows kept on the device before they go back to the host (a multiple of kNetLaunch; 1.25 MiB)

// One-frame calls (B <= latency_batch) of the resized entries: the source frames go through the pinned buffer, k_letterbox_bgr
// writes the network input on the device, the unchanged latency chain follows, and the host waits once (by the caller: `wait`
// false = og_yolo_detect_resized_u8_begin).  Returns the offset of the `best` rows in the pinned buffer.
int y_resized_latency(og_yolo* h, const uint8_t* frames, int B, int H, int W, int channels, const YGeo& g, float conf, size_t* o_best_pin) {
    const size_t n_src = (size_t)B * H * W * channels, n_net = (size_t)B * g.net_h * g.net_w * 3;
    const size_t p_best = al256(n_src), p_tot = p_best + al256((size_t)B * 5 * 4);
    const size_t o_net = al256(n_src), o_best = o_net + al256(n_net), tot = o_best + al256((size_t)B * 5 * 4);
    int rc;
    if ((rc = y_pin(h, p_tot)) || (rc = y_stage(h, tot))) return rc;
    char *ps = (char*)h->pin, *s = (char*)h->stage, *zp = nullptr;
    memcpy(ps, frames, n_src);
    HIPCHK(hipHostGetDevicePointer((void**)&zp, ps, 0));
    const uint8_t* src = (const uint8_t*)zp;
    if (!h->source_mapped) {
        HIPCHK(hipMemcpyAsync(s, ps, n_src, hipMemcpyHostToDevice, h->stream));
        src = (const uint8_t*)s;
    }
    if ((rc = y_letterbox(h, src, B, H, W, channels, g, (uint8_t*)(s + o_net)))) return rc;
    float* best_dev = h->zero_copy ? (float*)(zp + p_best) : (float*)(s + o_best);
    if ((rc = og_yolo_detect_u8_dev(h, (const uint8_t*)(s + o_net), B, g.net_h, g.net_w, conf, best_dev, nullptr))) return rc;
    if (!h->zero_copy) HIPCHK(hipMemcpyAsync(ps + p_best, s + o_best, (size_t)B * 5 * 4, hipMemcpyDeviceToHost, h->stream));
    *o_best_pin = p_best;
    return OG_OK;
}

}  // namespace

extern "C" {

int og_yolo_letterbox_geometry(int H, int W, int imgsz, int* net_h, int* net_w, int* new_h, int* new_w, int* pad_top, int* pad_left,
                               double* gain) {
#pragma clang fp contract(off)
    if (!net_h || !net_w || !new_h || !new_w || !pad_top || !pad_left || !gain) return fail(OG_EINVAL, "null argument");
    OG_ALIGN(net_h);
    OG_ALIGN(net_w);
    OG_ALIGN(new_h);
    OG_ALIGN(new_w);
    OG_ALIGN(pad_top);
    OG_ALIGN(pad_left);
    OG_ALIGN(gain);
    if (H < 1 || W < 1 || H > 8192 || W > 8192) return fail(OG_EINVAL, "frame sides must be in 1..8192");
    if (imgsz < 32 || imgsz > 8192 || imgsz % 32) return fail(OG_EINVAL, "imgsz must be a positive multiple of 32 (at most 8192)");
    const double rh = (double)imgsz / (double)H, rw = (double)imgsz / (double)W, r = rh < rw ? rh : rw;
    const int nw = (int)std::rint((double)W * r), nh = (int)std::rint((double)H * r);   // Python's round(): half to even
    if (nw < 1 || nh < 1) return fail(OG_EINVAL, "the letterboxed frame would have a side of 0 pixels");
    const int dw = (imgsz - nw) % 32, dh = (imgsz - nh) % 32;   // (nw, nh <= imgsz: non-negative)
    const int top = (int)std::rint((double)dh / 2 - 0.1), bottom = (int)std::rint((double)dh / 2 + 0.1);
    const int left = (int)std::rint((double)dw / 2 - 0.1), right = (int)std::rint((double)dw / 2 + 0.1);
    *net_h = nh + top + bottom;
    *net_w = nw + left + right;
    *new_h = nh;
    *new_w = nw;
    *pad_top = top;
    *pad_left = left;
    *gain = r;
    return OG_OK;
}

int og_yolo_letterbox_host(const uint8_t* src, int H, int W, int channels, int imgsz, uint8_t* out) {
    if (!src || !out) return fail(OG_EINVAL, "null buffer");
    if (channels != 1 && channels != 3) return fail(OG_EINVAL, "channels must be 1 (gray) or 3 (BGR)");
    YGeo g;
    int rc = og_yolo_letterbox_geometry(H, W, imgsz, &g.net_h, &g.net_w, &g.new_h, &g.new_w, &g.top, &g.left, &g.gain);
    if (rc) return rc;
    for (int y = 0; y < g.net_h; ++y)
        for (int x = 0; x < g.net_w; ++x) {
            uint8_t* o = out + ((size_t)y * g.net_w + x) * 3;
            if (channels == 3) og_letterbox_px<3>(src, H, W, g.new_h, g.new_w, g.top, g.left, y, x, o);
            else og_letterbox_px<1>(src, H, W, g.new_h, g.new_w, g.top, g.left, y, x, o);
        }
    return OG_OK;
}

int og_yolo_letterbox_u8_dev(og_yolo* h, const uint8_t* src_dev, int B, int H, int W, int channels, int imgsz, uint8_t* out_dev) {
    OG_SCOPE(h);
    YGeo g;
    int rc = y_check_resized(h, B, H, W, channels, imgsz, g);
    if (rc) return rc;
    if (B == 0) return OG_OK;
    if (!src_dev || !out_dev) return fail(OG_EINVAL, "null buffer");
    constexpr int kMaxY = 32768;   // grid.y
    for (int b0 = 0; b0 < B; b0 += kMaxY) {
        const int nb = B - b0 < kMaxY ? B - b0 : kMaxY;
        if ((rc = y_letterbox(h, src_dev + (size_t)b0 * H * W * channels, nb, H, W, channels, g, out_dev + (size_t)b0 * g.net_h * g.net_w * 3)))
            return rc;
    }
    return OG_OK;
}

int og_yolo_detect_resized_u8_dev(og_yolo* h, const uint8_t* src_dev, int B, int H, int W, int channels, int imgsz, float conf,
                                  float* best_dev) {
    OG_SCOPE(h);
    YGeo g;
    int rc = y_check_resized(h, B, H, W, channels, imgsz, g);
    if (rc) return rc;
    if (B == 0) return OG_OK;
    if (!src_dev || !best_dev) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(best_dev);
    if (h->pend_B) return fail(OG_EINVAL, "og_yolo_detect_resized_u8_dev: a begin / end call is in flight on this handle");
    const size_t net1 = (size_t)g.net_h * g.net_w * 3, src1 = (size_t)H * W * channels;
    if ((rc = y_stage(h, al256((size_t)(B < kNetLaunch ? B : kNetLaunch) * net1)))) return rc;
    uint8_t* net = (uint8_t*)h->stage;   // reused by every launch: the stream orders its writers after its readers
    for (int b0 = 0; b0 < B; b0 += kNetLaunch) {
        const int nb = B - b0 < kNetLaunch ? B - b0 : kNetLaunch;
        if ((rc = y_letterbox(h, src_dev + (size_t)b0 * src1, nb, H, W, channels, g, net)) ||
            (rc = og_yolo_detect_u8_dev(h, net, nb, g.net_h, g.net_w, conf, best_dev + (size_t)b0 * 5, nullptr)))
            return y_fail_sync(h, rc);
        OG_LAUNCH(k_scale_boxes, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, h->stream, best_dev + (size_t)b0 * 5, nb, g.scale() ? 1 : 0,
                  (float)g.gain, g.left, g.top, H, W);
        ++h->n_scale_boxes;
    }
    return OG_OK;
}

int og_yolo_detect_resized_u8(og_yolo* h, const uint8_t* frames, int B, int H, int W, int channels, int imgsz, float conf, float* best) {
    OG_SCOPE(h);
    YGeo g;
    int rc = y_check_resized(h, B, H, W, channels, imgsz, g);
    if (rc) return rc;
    if (B == 0) return OG_OK;
    if (!frames || !best) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(best);
    if (h->pend_B) return fail(OG_EINVAL, "og_yolo_detect_resized_u8: a begin / end call is in flight on this handle");
    const size_t net1 = (size_t)g.net_h * g.net_w * 3, src1 = (size_t)H * W * channels;
    if (B <= h->latency_batch) {
        size_t o_best = 0;
        if ((rc = y_resized_latency(h, frames, B, H, W, channels, g, conf, &o_best))) return y_fail_sync(h, rc);
        HIPCHK(hipStreamSynchronize(h->stream));
        memcpy(best, (char*)h->pin + o_best, (size_t)B * 5 * 4);
    } else {
        // the stage: [source chunk | network input of one launch | up to kBestRows best rows] -- bounded by the options, independent of B
        size_t fit = ((size_t)h->source_stage_kib << 10) / src1;
        if (fit < 1) fit = 1;   // a frame larger than the setting is staged alone
        if (fit > (size_t)kNetLaunch) fit = kNetLaunch;
        if (fit > (size_t)B) fit = B;
        const int nl = B < kNetLaunch ? B : kNetLaunch;
        const int nr = B < kBestRows ? B : kBestRows;
        const size_t o_net = al256(fit * src1), o_best = o_net + al256((size_t)nl * net1), tot = o_best + al256((size_t)nr * 5 * 4);
        if ((rc = y_stage(h, tot))) return rc;
        char* s = (char*)h->stage;
        for (int b0 = 0; b0 < B; b0 += kNetLaunch) {
            const int nb = B - b0 < kNetLaunch ? B - b0 : kNetLaunch;
            for (int c0 = 0; c0 < nb; c0 += (int)fit) {
                const int nc = nb - c0 < (int)fit ? nb - c0 : (int)fit;
                hipError_t e = hipMemcpyAsync(s, frames + (size_t)(b0 + c0) * src1, (size_t)nc * src1, hipMemcpyHostToDevice, h->stream);
                if (e != hipSuccess) return y_fail_sync(h, fail(OG_EHIP, std::string("hipMemcpyAsync (source frames): ") + hipGetErrorString(e)));
                if ((rc = y_letterbox(h, (const uint8_t*)s, nc, H, W, channels, g, (uint8_t*)(s + o_net) + (size_t)c0 * net1))) return y_fail_sync(h, rc);
            }
            const int r0 = b0 % kBestRows, end = b0 + nb;
            if ((rc = og_yolo_detect_u8_dev(h, (const uint8_t*)(s + o_net), nb, g.net_h, g.net_w, conf, (float*)(s + o_best) + (size_t)r0 * 5, nullptr)))
                return y_fail_sync(h, rc);
            if (end % kBestRows == 0 || end == B) {   // (a copy to pageable memory waits for the stream: once per kBestRows frames)
                const int first = end - (r0 + nb);
                hipError_t e = hipMemcpyAsync(best + (size_t)first * 5, s + o_best, (size_t)(r0 + nb) * 5 * 4, hipMemcpyDeviceToHost, h->stream);
                if (e != hipSuccess) return y_fail_sync(h, fail(OG_EHIP, std::string("hipMemcpyAsync (best): ") + hipGetErrorString(e)));
            }
        }
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if ((rc = y_check_range(h))) return rc;
    for (int b = 0; b < B; ++b) og_scale_box(best + (size_t)b * 5, g.scale(), (float)g.gain, g.left, g.top, H, W);
    return OG_OK;
}

int og_yolo_detect_resized_u8_begin(og_yolo* h, const uint8_t* frames, int B, int H, int W, int channels, int imgsz, float conf) {
    OG_SCOPE(h);
    YGeo g;
    int rc = y_check_resized(h, B, H, W, channels, imgsz, g);
    if (rc) return rc;
    if (h->pend_B) return fail(OG_EINVAL, "og_yolo_detect_resized_u8_begin: a call is already in flight on this handle");
    if (B == 0) return OG_OK;
    if (!frames) return fail(OG_EINVAL, "null buffer");
    if (B <= h->latency_batch && h->zero_copy) {
        size_t o_best = 0;
        if ((rc = y_resized_latency(h, frames, B, H, W, channels, g, conf, &o_best))) return y_fail_sync(h, rc);
        h->pend_sync = false;
        h->pend_off = o_best;
        h->pend_resized = true;
        h->pend_scale = g.scale();
        h->pend_gain = (float)g.gain;
        h->pend_left = g.left;
        h->pend_top = g.top;
        h->pend_H = H;
        h->pend_W = W;
    } else {   // larger calls / "zero_copy" 0: run now, deliver at end (as og_yolo_detect_u8_begin)
        h->pend_best.resize((size_t)B * 5);
        if ((rc = og_yolo_detect_resized_u8(h, frames, B, H, W, channels, imgsz, conf, h->pend_best.data()))) return rc;
        h->pend_sync = true;
        h->pend_resized = true;
    }
    h->pend_B = B;
    return OG_OK;
}

long long og_yolo_launch_count(og_yolo* h, const char* kernel) {
    if (!h || !kernel) return fail(OG_EINVAL, "null argument");
    const std::string k(kernel);
    if (k == "k_letterbox_bgr") return h->n_letterbox;
    if (k == "k_scale_boxes") return h->n_scale_boxes;
    return fail(OG_EINVAL, "og_yolo_launch_count: no counter for " + k);
}

}  // extern "C"

extern "C" {

int og_yolo_sync(og_yolo* h) {
    if (!h || !h->stream) return fail(OG_ESTATE, "handle not finalized");
    OG_SCOPE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    return y_check_range(h);
}

int og_yolo_get_activation(og_yolo* h, const char* name, int B, float* out, size_t cap, int* dims) {
    if (!h || !h->finalized || !h->arena) return fail(OG_ESTATE, "no detect call has run yet");
    if (!name || !out || !dims || B < 1 || B > h->lastB) return fail(OG_EINVAL, "bad argument");
    OG_ALIGN(out);
    OG_ALIGN(dims);
    auto it = h->acts.find(name);
    if (it == h->acts.end()) return fail(OG_EINVAL, std::string("unknown activation ") + name);
    const YView& v = it->second.v;
    int Cn = 0;
    for (const auto& s_ : it->second.segs) Cn += s_.C;
    dims[0] = Cn;
    dims[1] = v.H;
    dims[2] = v.W;
    const size_t HW = (size_t)v.H * v.W;
    if (cap < (size_t)B * Cn * HW) return fail(OG_EINVAL, "capacity too small");
    std::vector<float> tmp((size_t)B * v.fs4());
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(tmp.data(), v.base, tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
    const _Float16* t16 = (const _Float16*)tmp.data();   // f16 mode: widened here, f32 out in both modes
    for (int b = 0; b < B; ++b) {
        int c = 0;
        for (const auto& s_ : it->second.segs)
            for (int k = 0; k < s_.C; ++k, ++c)
                for (size_t p = 0; p < HW; ++p) {
                    const size_t i = ((size_t)b * HW + p) * v.Ctot + s_.off + k;
                    out[((size_t)b * Cn + c) * HW + p] = (v.es == 2) ? (float)t16[i] : tmp[i];
                }
    }
    return OG_OK;
}

}  // extern "C"
