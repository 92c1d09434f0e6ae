// C-ABI host side of libopenglottal_hip.so: state_dict intake, BN fold, weight
// repack into the MFMA fragment/LDS image, activation arena, kernel chain,
// hipGraph replay.  See include/openglottal_hip.h for the contract.
#include "../../include/openglottal_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "og_kernels.hpp"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// The header's alignment rule for caller-owned buffers: the natural alignment of the element type (u8: none).  Checked by every
// entry point before anything is launched or copied; NULL (an optional buffer left out) passes.
bool og_misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
#define OG_ALIGN(ptr)                                                                                                              \
    do {                                                                                                                           \
        if (og_misaligned((ptr), alignof(decltype(*(ptr)))))                                                                       \
            return fail(OG_EINVAL, std::string(#ptr) + " must be aligned to " + std::to_string(alignof(decltype(*(ptr)))) + " bytes"); \
    } while (0)

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            return fail(OG_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
        }                                                                                     \
    } while (0)

inline int cp32(int c) { return (c + 31) / 32 * 32; }

constexpr int kMaxLanes = 3;   // a fourth lane measured slower than three at every micro-batch size
constexpr size_t kPartialBytes = 64u << 20;  // split-K / position-split workspace per lane (only small launches ever use it)
constexpr int kTileCounters = 4096;          // arrival counters of the fused reduces per lane (one per tile of a split launch)

// A handle lives on one HIP device; HIP's current device is per host thread.  Every entry point selects the handle's device for
// the duration of the call and RESTORES the caller's on every exit path (a process that also drives torch on another device must not
// find its current device changed by a call into this library).
struct DeviceGuard {
    int prev = -1;
    bool restore = false;
    hipError_t err = hipSuccess;
    DeviceGuard(int dev, bool skip) {
        if (skip || dev < 0) return;
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            restore = (err == hipSuccess);
        }
    }
    ~DeviceGuard() {
        if (restore) (void)hipSetDevice(prev);
    }
};
#define OG_SCOPE(h)                                                                                       \
    DeviceGuard dg_((h) ? (h)->device : -1, og_skip_device(h));                                           \
    if (dg_.err != hipSuccess) return fail(OG_EHIP, std::string("selecting the handle's device: ") + hipGetErrorString(dg_.err))

// Dry run of a kernel chain ("plan"): while a recorder is installed on the calling thread, every launch site of the U-Net chain
// records (kernel, grid, block, LDS bytes, split-K workspace bytes, arrival counters) instead of launching, and no HIP call is made.
// og_unet_plan() runs the product's own launch decisions this way on a host-only handle, so that their bounds -- grid.z <= 65535,
// LDS <= 160 KB, workspace <= kPartialBytes, counters <= kTileCounters -- can be walked over every micro-batch size, layer shape and
// forced option on a machine without a GPU (tests/test_launch_plan.py).
struct PlanRec {
    std::string kernel;
    unsigned gx, gy, gz, block, lds;
    long long partial_bytes;
    long long counters;
    std::string writes;   // og_unet_plan_resized: "buffer=end" per caller-owned buffer the launch writes (end = bytes from its base)
    std::string mod;      // og_yolo_plan: the module path the launch serves
};
struct Plan {
    std::vector<PlanRec> recs;
    long long need_partial = 0, need_counters = 0;
    std::map<std::string, const void*> bases;   // og_unet_plan_resized: placeholder base of each caller-owned buffer
};
thread_local Plan* g_plan = nullptr;
// the detector's chain: the module path the launches being enqueued serve (og_yolo_plan records, "trace_launches" 1 traces)
thread_local const char* g_launch_mod = nullptr;
// og_yolo option "trace_launches" 1: while a real chain is enqueued, the labels og_yolo_plan would give its launches, with their modules
thread_local std::vector<std::pair<std::string, std::string>>* g_trace = nullptr;
// og_yolo_plan: upload() hands out placeholder pointers (no device)
thread_local bool g_upload_placeholder = false;
inline void plan_need(long long partial_bytes, long long counters) {
    if (g_plan) {
        g_plan->need_partial = partial_bytes;
        g_plan->need_counters = counters;
    }
}
inline void plan_record(const char* kernel, dim3 grid, dim3 block, size_t lds) {
    g_plan->recs.push_back({kernel, grid.x, grid.y, grid.z, block.x, (unsigned)lds, g_plan->need_partial, g_plan->need_counters, "",
                            g_launch_mod ? g_launch_mod : ""});
    g_plan->need_partial = g_plan->need_counters = 0;
}
// the last recorded launch writes `bytes` into caller-owned buffer `name` starting at `p`: note where that ends, from the buffer's base
inline void plan_write(const char* name, const void* p, long long bytes) {
    if (!g_plan || !p || g_plan->recs.empty()) return;
    auto it = g_plan->bases.find(name);
    if (it == g_plan->bases.end()) return;
    const long long end = (long long)((const char*)p - (const char*)it->second) + bytes;
    std::string& w = g_plan->recs.back().writes;
    w += (w.empty() ? "" : ";") + std::string(name) + "=" + std::to_string(end);
}
// og_unet_plan only: name the launch just recorded by the instantiation that would run, every template argument resolved (the
// launch site's text has template parameters in it), with what is decided at run time behind it (" ksplit=3", " nt=2")
inline void plan_inst(const char* fmt, ...) {
    std::string* slot = nullptr;
    if (g_plan && !g_plan->recs.empty()) slot = &g_plan->recs.back().kernel;
    else if (g_trace && !g_trace->empty()) slot = &g_trace->back().first;
    if (!slot) return;
    char inst[96];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(inst, sizeof inst, fmt, ap);
    va_end(ap);
    *slot = inst;
}
// every launch of the chain goes through here: a failed launch is reported as OG_EHIP by THIS call (not by a later one)
#define OG_LAUNCH(kern, grid, block, lds, stream, ...)                                                    \
    do {                                                                                                  \
        if (g_plan) {                                                                                     \
            plan_record(#kern, grid, block, lds);                                                         \
        } else {                                                                                          \
            hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);                              \
            hipError_t le_ = hipGetLastError();                                                           \
            if (le_ != hipSuccess) return fail(OG_EHIP, std::string(#kern) + ": " + hipGetErrorString(le_)); \
            if (g_trace) g_trace->push_back({#kern, g_launch_mod ? g_launch_mod : ""});                   \
        }                                                                                                 \
    } while (0)

// Dynamic LDS above the default limit has to be permitted per kernel before the first launch.  A launch site that goes through
// OG_LAUNCH_LDS instantiates one KernelLds per (kernel, LDS size): the node links itself into g_kernel_lds while the library is
// loaded, and init_kernel_attrs() walks the list at handle initialisation (never inside a stream capture).  So the size a kernel is
// launched with and the size it is permitted are the same constant, and a launcher that exists has its permission.
struct KernelLds {
    const void* kern;
    int lds;
    KernelLds* next;
    KernelLds(const void* k, int l);
};
KernelLds* g_kernel_lds = nullptr;
inline KernelLds::KernelLds(const void* k, int l) : kern(k), lds(l), next(g_kernel_lds) { g_kernel_lds = this; }
template <auto KERN, int LDS>
struct KernelLdsOf {
    static inline KernelLds node{(const void*)KERN, LDS};
};
#define OG_LAUNCH_LDS(kern, grid, block, lds, stream, ...)                                                \
    do {                                                                                                  \
        (void)&KernelLdsOf<(kern), (lds)>::node;                                                          \
        OG_LAUNCH(kern, grid, block, lds, stream, __VA_ARGS__);                                           \
    } while (0)
int init_kernel_attrs() {  // must not run inside a stream capture
    for (const KernelLds* k = g_kernel_lds; k; k = k->next)
        HIPCHK(hipFuncSetAttribute(k->kern, hipFuncAttributeMaxDynamicSharedMemorySize, k->lds));
    return OG_OK;
}

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
};

struct ConvLayer {  // one 3x3 conv + BN + ReLU, or one 2x2 transposed conv
    std::string name;
    int mode = 0;  // 0 conv3x3, 1 convT
    int Cin = 0, Cout = 0;      // true channel counts (for FLOP accounting)
    int Cin_p = 0, Cout_p = 0;  // padded (buffer) channel counts
    int NT = 1;
    float* d_w = nullptr;
    float* d_w_h = nullptr;   // the same weights as f16 hi/lo pairs in the H layout (opt-in split precision)
    float* d_w_f = nullptr;   // the same weights rounded once to f16, 64-channel chunks (opt-in f16 mode, k_conv_mfma_f)
    float* d_w1 = nullptr;    // 3x3 convs with NT == 2: the same weights packed for 32-column tiles (split-K launches)
    float* d_ww = nullptr;    // 3x3 convs: Winograd F(2x2,3x3) image for k_conv_wino<NT> (pack_wino)
    float* d_ww1 = nullptr;   // NT == 2 layers: the same image cut for 32-column tiles and 8-channel chunks (k_conv_wino_w)
    float* d_scale = nullptr;
    float* d_shift = nullptr;
};

struct Act {  // NHWC activation view
    float* p = nullptr;
    int C = 0;  // pixel stride (floats)
    int H = 0, W = 0;
    long long frame_stride() const { return (long long)H * W * C; }
};

struct GraphKey {
    int B, H, W, flags, capB;   // capB: frame capacity of the arena plan the graph's pointers belong to
    bool operator<(const GraphKey& o) const { return memcmp(this, &o, sizeof(GraphKey)) < 0; }
};

}  // namespace

struct og_unet {
    std::vector<int> features;
    int L = 0;
    int device = 0;   // HIP device the handle lives on (current device of the thread that finalized it): every entry point makes it
                      // the calling thread's current device, so a handle can be driven from any host thread (HIP's is per thread)
    std::map<std::string, HostTensor> host;
    std::map<std::string, std::vector<int64_t>> expected;
    bool finalized = false;
    bool host_only = false;   // og_unet_plan: layer shapes and launch decisions only -- no device, no stream, pointers are placeholders

    // parameters on device
    float* d_first_w = nullptr;  // [9][Cp0]
    float* d_first_scale = nullptr;
    float* d_first_shift = nullptr;
    std::vector<ConvLayer> enc_a, enc_b;  // enc_a[0] unused (first layer is k_conv_first)
    ConvLayer bott_a, bott_b;
    std::vector<ConvLayer> up_t, dec_a, dec_b;  // indexed by j (0 = deepest)
    float* d_head_w = nullptr;
    float head_bias = 0.f;
    float* d_zero = nullptr;

    // activation arena for (capB, H, W)
    int capB = 0, aH = 0, aW = 0;
    void* arena = nullptr;
    size_t arena_bytes = 0;
    std::vector<Act> A, CAT, P, UA, UB;
    Act BA, BB;

    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // per-launch profiling (og_unet_profile): when `prof` is set every enqueue_* brackets
    // its launch with events and records kernel symbol + algorithmic FLOPs
    struct ProfEntry {
        std::string layer, kernel;
        double flops;
        hipEvent_t e0, e1;
    };
    std::vector<ProfEntry>* prof = nullptr;
    unsigned long long* d_stamps = nullptr;  // [64 launches][1024 workgroups][4], allocated by og_unet_clock_probe
    bool probing = false;                    // set for the duration of og_unet_clock_probe only: no other call makes a kernel write stamps
    int chunk = 32;
    int use_graphs = 1;
    int conv_impl = 2;   // 0 k_conv_mfma | 1 k_conv_mfma_p (persistent, pipelined) | 2 auto: k_conv_mfma_o (3 WG/CU, single halo
                         // buffer) for full launches, k_conv_mfma_p + split-K for launches that cannot fill the chip | 3 k_conv_mfma_o, 4 WG/CU
    int tps_nt1 = 3;     // taps per step for the 32-column kernel
    int xcd_group = 1;   // see LaunchCtx::xcd_group
    int splitk_occ = 1;  // split-K parts on the occupancy kernel (0: persistent kernel)
    int splitk_min_steps = 3;  // smallest K part of a split 3x3 conv, in (chunk, tap) steps (9 = one channel chunk; 3 measured +1.4 % at one frame per chain)
    int wino = 1;        // 3x3 layers in Winograd F(2x2,3x3) form (k_conv_wino, all f32): the CANONICAL arithmetic of this library.
                         // Which layers take it is a function of the handle's options and of (H, W) alone -- never of the micro-batch
                         // size, the lane, the shard or the entry point -- so a frame's mask is a function of the frame only
                         // (features.py:234-238 has no cross-frame state either).  0: the direct kernels for every layer.
    int zero_copy = 1;   // per-frame calls: the chain reads / writes the pinned host buffers directly (see fill() in stream_impl)
    int wino_ps = 1;     // under-filled Winograd launches spread a tile's 16 positions over several workgroups (k_conv_wino_ps: bit-identical);
                         // 0 off, 1 auto, 2 / 3 / 4 force PN = 4 / 2 / 1 on every launch that qualifies
    int wino_w = 1;      // under-filled Winograd launches on k_conv_wino_w (the 16 positions over the four waves of a workgroup, finer
                         // tiles) / k_conv_wino_wp (its position rows on four workgroups): bit-identical; 0 off, 1 auto,
                         // 2 / 3 force k_conv_wino_w<1> / <2>, 4 forces k_conv_wino_wp on every Winograd layer (tests, A/B)
    int inject_fault = 0; // TEST HOOK ("inject_fault" n): the n-th conv launch from now on fails with OG_EHIP after scribbling over the arrival
                          // counters, as a launch that died half-way would leave them; the error paths must restore them (tests/test_gpu_recovery.py)
    int active_lanes = 1; // lanes of the call in progress (set by the entry points on every lane): scheduling hint for pick_wino_w
    int wino_first = 1;  // Winograd chains: first layer unfused so that the second conv takes k_conv_wino<1>
    bool wino_chain = false;   // (pick_chain_form) wino && precision == 0 && conv_impl == 2
    int splitk_nt1 = 1;  // split 3x3 launches on 32-column tiles (twice the workgroups, half the MFMAs per K part)
    int splitk_slots = 1, splitk_div = 2;  // occupancy split-K: target workgroups per CU; split when the launch fills < 1/div of them
                                           // (round-2 sweep, one to three lanes, both precisions: 1 / 2 beats round 1's 2 / 4 at 1-4 frames per launch)
    int occ_min_pct = 100; // occupancy kernel when workgroups >= pct % of the CU count (0: one full round of 2-3 per CU);
                           // measured 25..300 at 2..32 frames per launch: 100 is best or within 1 % everywhere
    int tps_nt2 = 1;     // taps per step for the 64-column kernel
    int prio_mode = 3;   // see ConvArgs::prio_mode: 3 = occupancy kernel raises its priority outside the main loop (+0.2-0.4 %
                         // after the VALU diet; 0 before it) and the persistent kernel alternates as in mode 2 (+1.2 % there)
    // Two lanes: odd micro-batches of one call run on a twin handle (own stream, arena, graphs; SHARED weights), so
    // the launch tails of one chain are filled by the other chain's kernels (+2-4 % measured, tools/two_streams.py).
    og_unet* twin = nullptr;
    int n_lanes = 0;   // lanes used per call when "dual" is on: 1..kMaxLanes, 0 = by micro-batch size
    bool is_twin = false;
    int dual = 1;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int fuse_first = 1;  // compute the first layer inside downs.0's second conv (u8 path, full launches only)
    int fuse_head = 1;   // compute the 1x1 head + threshold + area inside the last conv's epilogue (Cout_p == 32 only)
    int keep_taps = 0;   // fused head: still store the last activation tensor (og_unet_get_activation("ups.N.b"))
    int entry_f32 = 0;   // DIAGNOSTIC ("entry_f32" 1): og_unet_profile / og_unet_plan walk the chain of the NCHW-float entry point
                         // (og_unet_forward_f32: k_conv_first<float>, never the fused first layer); gray_dev then holds B x H x W floats
    struct {
        bool active = false;
        float thr = 0.5f;
        const int32_t* boxes = nullptr;
        float* logits = nullptr;
        uint8_t* mask = nullptr;
        int32_t* area = nullptr;
    } fuse;
    int convt_occ = 1;   // with conv_impl >= 2: run the transposed convs on the occupancy variant too
    int convt_w = 1;     // under-filled transposed-conv launches on k_convt_w (wave-sized tiles, operands straight to registers: bit-identical)
    int tile_h = 0;      // 0 auto (16x16 tiles for 64-channel-tile layers at <= 64x64 pixels, else 8x16) | 8 | 16
    int splitk = 0;      // OPT-IN (non-canonical): split K over workgroups on launches that would fill < 1/div of the chip.  It changes the
                         // summation order, so a frame's logits then depend on how many frames share its launch; off by default
    float* d_partial = nullptr;
    int* d_tile_counter = nullptr;   // split-K arrival counters (fused reduce), zero between launches
    int splitk_fused = 1;            // last-arriving K part reduces + runs the epilogue (0: separate k_splitk_epilogue launch)
    int32_t* d_counts = nullptr;  // fused head: per-(frame, tile, wave) foreground counts of the current chunk
    size_t counts_cap = 0;
    int wg_per_cu = 2;   // persistent grid = wg_per_cu * CUs (capped by the item count)
    int n_cu = 256;
    std::map<GraphKey, hipGraphExec_t> graphs;
    int lastB = 0;

    // staging for host-pointer entry points
    void* stage = nullptr;
    size_t stage_bytes = 0;

    // Streaming ingest engine (og_unet_stream_u8): a ring of `slots` micro-batches, each with device buffers and PINNED
    // host buffers for its inputs and outputs, so that the host -> device copy of micro-batch k+1 and the device -> host
    // copy of micro-batch k-1 run (on their own streams) under the kernel chain of micro-batch k.  Device memory is
    // bounded by slots x chunk frames whatever the length of the video (features.py:226 loads all frames first).
    struct Slot {
        uint8_t *d_in = nullptr, *d_gray = nullptr, *d_mask = nullptr, *h_in = nullptr, *h_mask = nullptr;
        int32_t *d_area = nullptr, *d_boxes = nullptr, *h_area = nullptr, *h_boxes = nullptr;
        float *d_logits = nullptr, *h_logits = nullptr;
        float* d_net = nullptr;   // resized calls: the chain's logits at network size (d_gray is then at network size too)
        hipEvent_t ev_h2d = nullptr, ev_done = nullptr, ev_out = nullptr;
        int b0 = -1, nb = 0;   // micro-batch occupying the slot (-1: free)
    };
    struct Ring {
        std::vector<Slot> slots;
        int cap = 0, H = 0, W = 0, ch = 0;
        int Hn = 0, Wn = 0;   // network size of resized calls (0: the chain runs at H x W)
        bool mask = false, logits = false;
        hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    } ring;
    int precision = 0;     // 0: exact f32 (v_mfma_f32_32x32x2_f32) -- the default and the parity reference; 1: opt-in split precision
                           // (f16 hi/lo pairs, 3 x v_mfma_f32_32x32x16_f16 per f32 product, f32 accumulation; k_conv_mfma_h);
                           // 2: opt-in f16 mode (f16 operands and 2-byte activations, one MFMA per product, f32 accumulation; k_conv_mfma_f)
    int* h_range = nullptr;   // split precision: host-mapped word the kernels raise when an activation leaves the f16 range
    int* d_range = nullptr;   //   (device view of the same word; the lanes share it)
    int h_square = 1;      // split precision, 64-column kernel on 16x16 tiles: 2x2 sub-tiles per wave (fewer LDS reads per MFMA)
    int stream_host = 1;   // og_unet_segment_u8 goes through the streaming engine (0: one-shot staging of the whole batch)
};

inline bool og_skip_device(const og_unet* h) { return !h || h->host_only || !h->finalized; }

namespace {

void expect(og_unet* h, const std::string& k, std::vector<int64_t> s) { h->expected[k] = std::move(s); }

void expect_double_conv(og_unet* h, const std::string& p, int ci, int co) {
    expect(h, p + ".net.0.weight", {co, ci, 3, 3});
    expect(h, p + ".net.3.weight", {co, co, 3, 3});
    for (const char* n : {".net.1", ".net.4"}) {
        for (const char* f : {".weight", ".bias", ".running_mean", ".running_var"}) expect(h, p + n + f, {co});
    }
}

// Fold eval-mode BatchNorm2d (eps 1e-5) into y = conv*scale + shift, in float64.
void fold_bn(const og_unet* h, const std::string& bn, int C, int Cp, std::vector<float>& scale, std::vector<float>& shift) {
    const auto& g = h->host.at(bn + ".weight").data;
    const auto& b = h->host.at(bn + ".bias").data;
    const auto& mu = h->host.at(bn + ".running_mean").data;
    const auto& var = h->host.at(bn + ".running_var").data;
    scale.assign(Cp, 0.f);
    shift.assign(Cp, 0.f);
    for (int c = 0; c < C; ++c) {
        const double s = (double)g[c] / std::sqrt((double)var[c] + 1e-5);
        scale[c] = (float)s;
        shift[c] = (float)((double)b[c] - (double)mu[c] * s);
    }
}

// Packed weight image, consumed verbatim by LDS-DMA (global_load_lds writes LDS
// linearly, so the bank swizzle lives in this global layout):
//   [n_tile][chunk][tap][row r in 0..32*NT)[8 slots of 4 floats], slot' = slot ^ ((r>>1)&7)
// row r <-> GEMM column n = n_tile*32*NT + r; slot/element <-> padded input channel k.
template <typename F>
std::vector<float> pack_gemm_b(int Ncols_p, int Kp, int taps, int NT, F&& weight_at /*(n, k, tap)->float*/) {
    const int rows = 32 * NT;
    const int n_tiles = Ncols_p / rows;
    const int n_chunks = Kp / 32;
    std::vector<float> out((size_t)Ncols_p * Kp * taps, 0.f);
    size_t o = 0;
    for (int nt = 0; nt < n_tiles; ++nt)
        for (int c = 0; c < n_chunks; ++c)
            for (int t = 0; t < taps; ++t) {
                for (int r = 0; r < rows; ++r)
                    for (int ps = 0; ps < 8; ++ps) {
                        const int sl = ps ^ ((r >> 1) & 7);
                        for (int e = 0; e < 4; ++e) out[o + (size_t)r * 32 + ps * 4 + e] = weight_at(nt * rows + r, c * 32 + sl * 4 + e, t);
                    }
                o += (size_t)rows * 32;
            }
    return out;
}

// Winograd F(2x2, 3x3) image of a 3x3 conv's weights for k_conv_wino<NT>: U = G g G^T (computed in double, rounded once),
//   [n_tile of 32 NT columns][chunk of KC = 8 NT channels][position 4i + j][column r][KC / 4 slots of 4 floats],
//   slot' = slot ^ ((r>>2)&3) (NT 2) | slot ^ ((r>>3)&1) (NT 1)
template <typename F>
std::vector<float> pack_wino(int Ncols_p, int Kp, int NT, F&& weight_at /*(n, k, tap)->float*/) {
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    const int rows = 32 * NT, KC = 8 * NT, SL = KC / 4;
    const int n_tiles = Ncols_p / rows, n_ck = Kp / KC;
    std::vector<float> out((size_t)Ncols_p * Kp * 16, 0.f);
    for (int nt = 0; nt < n_tiles; ++nt)
        for (int c = 0; c < n_ck; ++c)
            for (int r = 0; r < rows; ++r)
                for (int ps = 0; ps < SL; ++ps) {
                    const int sl = (NT == 2) ? ps ^ ((r >> 2) & 3) : ps ^ ((r >> 3) & 1);
                    for (int e = 0; e < 4; ++e) {
                        double g[3][3], t[4][3];
                        for (int tp = 0; tp < 9; ++tp) g[tp / 3][tp % 3] = (double)weight_at(nt * rows + r, c * KC + sl * 4 + e, tp);
                        for (int i = 0; i < 4; ++i)
                            for (int x = 0; x < 3; ++x) t[i][x] = G[i][0] * g[0][x] + G[i][1] * g[1][x] + G[i][2] * g[2][x];
                        for (int i = 0; i < 4; ++i)
                            for (int j = 0; j < 4; ++j) {
                                const double u = t[i][0] * G[j][0] + t[i][1] * G[j][1] + t[i][2] * G[j][2];
                                out[((((size_t)nt * n_ck + c) * 16 + (4 * i + j)) * rows + r) * KC + ps * 4 + e] = (float)u;
                            }
                    }
                }
    return out;
}

// Split-precision image of the same weights (og_kernels.hpp "H layout"): per (row, chunk, tap) the 128 bytes hold eight
// 16-byte slots, logical slot s < 4 = f16 hi of k = 32c + 8s .. +7, slot 4+s = f16 lo (scaled by 2^11) of the same k;
// physical slot = logical ^ ((r>>1)&7) as in the f32 image.  Same byte size, so it is carried in a float vector.
template <typename F>
std::vector<float> pack_gemm_b_h(int Ncols_p, int Kp, int taps, int NT, F&& weight_at /*(n, k, tap)->float*/) {
    const int rows = 32 * NT;
    const int n_tiles = Ncols_p / rows;
    const int n_chunks = Kp / 32;
    std::vector<float> out((size_t)Ncols_p * Kp * taps, 0.f);
    _Float16* o16 = (_Float16*)out.data();
    size_t o = 0;   // in halves
    for (int nt = 0; nt < n_tiles; ++nt)
        for (int c = 0; c < n_chunks; ++c)
            for (int t = 0; t < taps; ++t) {
                for (int r = 0; r < rows; ++r)
                    for (int ps = 0; ps < 8; ++ps) {
                        const int sl = ps ^ ((r >> 1) & 7);
                        for (int e = 0; e < 8; ++e) {
                            const float w = weight_at(nt * rows + r, c * 32 + (sl & 3) * 8 + e, t);
                            const _Float16 hi = (_Float16)w;
                            const _Float16 lo = (_Float16)((w - (float)hi) * 2048.0f);
                            o16[o + (size_t)r * 64 + ps * 8 + e] = (sl < 4) ? hi : lo;
                        }
                    }
                o += (size_t)rows * 64;
            }
    return out;
}

// f16-mode image (og_kernels.hpp "F layout"): per (row, 64-channel chunk, tap) the 128 bytes hold eight 16-byte slots, logical
// slot s = f16 (round to nearest even, once) of k = 64c + 8s .. +7; physical slot = logical ^ ((r>>1)&7) as in the f32 image.
// A padded Cin that is an odd multiple of 32 leaves the upper half of the last chunk zero (the kernel skips it: ConvArgs::k_half).
template <typename F>
std::vector<float> pack_gemm_b_f(int Ncols_p, int Kp, int taps, int NT, F&& weight_at /*(n, k, tap)->float*/) {
    const int rows = 32 * NT;
    const int n_tiles = Ncols_p / rows;
    const int n_chunks = (Kp + 63) / 64;
    std::vector<float> out((size_t)Ncols_p * n_chunks * 32 * taps, 0.f);
    _Float16* o16 = (_Float16*)out.data();
    size_t o = 0;   // in halves
    for (int nt = 0; nt < n_tiles; ++nt)
        for (int c = 0; c < n_chunks; ++c)
            for (int t = 0; t < taps; ++t) {
                for (int r = 0; r < rows; ++r)
                    for (int ps = 0; ps < 8; ++ps) {
                        const int sl = ps ^ ((r >> 1) & 7);
                        for (int e = 0; e < 8; ++e) {
                            const int k = c * 64 + sl * 8 + e;
                            o16[o + (size_t)r * 64 + ps * 8 + e] = (_Float16)((k < Kp) ? weight_at(nt * rows + r, k, t) : 0.f);
                        }
                    }
                o += (size_t)rows * 64;
            }
    return out;
}

int upload(const std::vector<float>& v, float** d) {
    if (g_upload_placeholder) {
        *d = (float*)8;
        return OG_OK;
    }
    HIPCHK(hipMalloc((void**)d, v.size() * sizeof(float)));
    HIPCHK(hipMemcpy(*d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    return OG_OK;
}

// cin_map: padded input channel -> original input channel (or -1)
int build_conv(og_unet* h, ConvLayer& L, const std::string& wkey, const std::string& bnkey, int Cin, int Cout,
               const std::vector<int>& cin_map) {
    L.name = wkey;
    L.mode = 0;
    L.Cin = Cin;
    L.Cout = Cout;
    L.Cin_p = (int)cin_map.size();
    L.Cout_p = cp32(Cout);
    L.NT = (L.Cout_p % 64 == 0) ? 2 : 1;
    if (h->host_only) {   // shapes only: every image a launch decision asks for "exists"
        L.d_w = L.d_w_h = L.d_w_f = L.d_ww = L.d_scale = L.d_shift = (float*)8;
        L.d_w1 = L.d_ww1 = (L.NT == 2) ? (float*)8 : nullptr;
        return OG_OK;
    }
    const auto& w = h->host.at(wkey).data;  // [Cout][Cin][3][3]
    auto at = [&](int n, int k, int t) -> float {
        const int ci = cin_map[k];
        if (n >= Cout || ci < 0) return 0.f;
        return w[((size_t)n * Cin + ci) * 9 + t];
    };
    std::vector<float> pk = pack_gemm_b(L.Cout_p, L.Cin_p, 9, L.NT, at);
    std::vector<float> sc, sh;
    fold_bn(h, bnkey, Cout, L.Cout_p, sc, sh);
    int rc;
    if ((rc = upload(pk, &L.d_w))) return rc;
    if ((rc = upload(pack_gemm_b_h(L.Cout_p, L.Cin_p, 9, L.NT, at), &L.d_w_h))) return rc;
    if ((rc = upload(pack_gemm_b_f(L.Cout_p, L.Cin_p, 9, L.NT, at), &L.d_w_f))) return rc;
    if (L.NT == 2 && (rc = upload(pack_gemm_b(L.Cout_p, L.Cin_p, 9, 1, at), &L.d_w1))) return rc;
    if ((rc = upload(pack_wino(L.Cout_p, L.Cin_p, L.NT, at), &L.d_ww))) return rc;
    if (L.NT == 2 && (rc = upload(pack_wino(L.Cout_p, L.Cin_p, 1, at), &L.d_ww1))) return rc;
    if ((rc = upload(sc, &L.d_scale))) return rc;
    if ((rc = upload(sh, &L.d_shift))) return rc;
    return OG_OK;
}

int build_convT(og_unet* h, ConvLayer& L, const std::string& p, int Cin, int Cout) {
    L.name = p;
    L.mode = 1;
    L.Cin = Cin;
    L.Cout = Cout;
    L.Cin_p = cp32(Cin);
    L.Cout_p = cp32(Cout);
    L.NT = 2;  // N = 4*Cout_p is a multiple of 128
    if (h->host_only) {
        L.d_w = L.d_w_h = L.d_w_f = L.d_w1 = L.d_scale = L.d_shift = (float*)8;
        return OG_OK;
    }
    const auto& w = h->host.at(p + ".weight").data;  // [Cin][Cout][2][2]
    const auto& bias = h->host.at(p + ".bias").data;
    const int Cop = L.Cout_p;
    auto at = [&](int n, int k, int) -> float {
        const int q = n / Cop, co = n % Cop;
        if (co >= Cout || k >= Cin) return 0.f;
        return w[((size_t)k * Cout + co) * 4 + q];
    };
    std::vector<float> pk = pack_gemm_b(4 * Cop, L.Cin_p, 1, L.NT, at);
    std::vector<float> sc(Cop, 0.f), sh(Cop, 0.f);
    for (int c = 0; c < Cout; ++c) {
        sc[c] = 1.f;
        sh[c] = bias[c];
    }
    int rc;
    if ((rc = upload(pk, &L.d_w))) return rc;
    if ((rc = upload(pack_gemm_b(4 * Cop, L.Cin_p, 1, 1, at), &L.d_w1))) return rc;   // 32-column tiles (k_convt_w)
    if ((rc = upload(pack_gemm_b_h(4 * Cop, L.Cin_p, 1, L.NT, at), &L.d_w_h))) return rc;
    if ((rc = upload(pack_gemm_b_f(4 * Cop, L.Cin_p, 1, L.NT, at), &L.d_w_f))) return rc;
    if ((rc = upload(sc, &L.d_scale))) return rc;
    if ((rc = upload(sh, &L.d_shift))) return rc;
    return OG_OK;
}

std::vector<int> ident_map(int Cin) {
    std::vector<int> m(cp32(Cin), -1);
    for (int i = 0; i < Cin; ++i) m[i] = i;
    return m;
}

void free_layer(ConvLayer& L) {
    if (L.d_w) (void)hipFree(L.d_w);
    if (L.d_w_h) (void)hipFree(L.d_w_h);
    if (L.d_w_f) (void)hipFree(L.d_w_f);
    if (L.d_w1) (void)hipFree(L.d_w1);
    if (L.d_ww) (void)hipFree(L.d_ww);
    if (L.d_ww1) (void)hipFree(L.d_ww1);
    if (L.d_scale) (void)hipFree(L.d_scale);
    if (L.d_shift) (void)hipFree(L.d_shift);
    L.d_w = L.d_w_h = L.d_w_f = L.d_w1 = L.d_ww = L.d_ww1 = L.d_scale = L.d_shift = nullptr;
}

void drop_graphs(og_unet* h) {
    for (auto& kv : h->graphs) (void)hipGraphExecDestroy(kv.second);
    h->graphs.clear();
}

// After a failed call: the fused reduces (k_conv_wino_ps / _wp, split-K) rely on arrival counters that are zero at launch and are
// re-zeroed only by a tile's LAST arriver, so a chain that stopped half-way (failed launch, failed capture, device error) may leave
// some behind -- later calls would then never elect a reducer for those tiles, or elect it early, and return stale activations with
// rc 0.  Every error path therefore clears the lane's counters (in stream order) before the error is reported.
void reset_counters(og_unet* h) {
    if (h->host_only || !h->d_tile_counter || !h->stream) return;
    (void)hipMemsetAsync(h->d_tile_counter, 0, kTileCounters * sizeof(int), h->stream);
}

// Layout of the activation arena for (B, H, W): views as OFFSETS from the arena base (pure arithmetic, no device)
struct ArenaPlan {
    std::vector<Act> A, CAT, P, UA, UB;
    Act BA, BB;
    size_t total = 0;
};
ArenaPlan arena_layout(const og_unet* h, int B, int H, int W) {
    const int L = h->L;
    ArenaPlan p;
    p.A.resize(L); p.CAT.resize(L); p.P.resize(L); p.UA.resize(L); p.UB.resize(L);
    // f16 mode (F layout): 2 bytes per channel -- Act::C, the pixel stride, stays in 4-byte units and is then HALF the channel count
    const int cdiv = (h->precision == 2) ? 2 : 1;
    auto plan = [&](Act& a, int Cch, int hh, int ww) {
        const int C = Cch / cdiv;
        a.C = C;
        a.H = hh;
        a.W = ww;
        a.p = (float*)p.total;  // offset for now
        p.total += ((size_t)B * hh * ww * C * sizeof(float) + 255) / 256 * 256;
    };
    for (int i = 0; i < L; ++i) {
        const int C = cp32(h->features[i]);
        const int hh = H >> i, ww = W >> i;
        plan(p.A[i], C, hh, ww);
        plan(p.CAT[i], 2 * C, hh, ww);
        plan(p.P[i], C, hh >> 1, ww >> 1);
        plan(p.UA[i], C, hh, ww);
        plan(p.UB[i], C, hh, ww);
    }
    const int Cb = cp32(2 * h->features[L - 1]);
    plan(p.BA, Cb, H >> L, W >> L);
    plan(p.BB, Cb, H >> L, W >> L);
    return p;
}
void adopt_arena(og_unet* h, ArenaPlan& p, void* base, int B, int H, int W) {
    auto fix = [&](Act& a) { a.p = (float*)((char*)base + (size_t)a.p); };
    for (int i = 0; i < h->L; ++i) {
        fix(p.A[i]);
        fix(p.CAT[i]);
        fix(p.P[i]);
        fix(p.UA[i]);
        fix(p.UB[i]);
    }
    fix(p.BA);
    fix(p.BB);
    h->A = p.A;
    h->CAT = p.CAT;
    h->P = p.P;
    h->UA = p.UA;
    h->UB = p.UB;
    h->BA = p.BA;
    h->BB = p.BB;
    h->capB = B;
    h->aH = H;
    h->aW = W;
}

// Activation arena.  Capacity is kept in BYTES: a call at another frame size (or a smaller micro-batch) re-plans the layer
// buffers inside the existing allocation instead of freeing and reallocating it, and captured hipGraphs stay valid as long as
// the allocation does (their key carries the plan's frame capacity), so a stream of mixed frame sizes does not thrash
// hipMalloc / graph capture.  Growth still reallocates once; og_unet_reserve() does it ahead of time.
int ensure_arena(og_unet* h, int B, int H, int W) {
    const bool same_shape = (H == h->aH && W == h->aW);
    if (h->arena && same_shape && B <= h->capB) return OG_OK;
    if (same_shape && B < h->capB) B = h->capB;
    ArenaPlan p = arena_layout(h, B, H, W);
    const size_t total = p.total;
    if (h->stream) HIPCHK(hipStreamSynchronize(h->stream));   // the old plan may still be in use
    if (!h->arena || total > h->arena_bytes) {
        drop_graphs(h);   // they hold pointers into the old allocation
        if (h->arena) {
            HIPCHK(hipFree(h->arena));
            h->arena = nullptr;
            h->arena_bytes = 0;
        }
        HIPCHK(hipMalloc(&h->arena, total));
        h->arena_bytes = total;
    }
    // Padded channels of the convT half etc. are always written (zero weights -> exact zeros), but clear on every re-plan
    // so that debug reads of never-touched bytes are defined.
    HIPCHK(hipMemsetAsync(h->arena, 0, total, h->stream));
    adopt_arena(h, p, h->arena, B, H, W);
    return OG_OK;
}

struct LaunchCtx {
    hipStream_t stream;
    int n_cu;
    int wg_per_cu;
    int xcd_group = 1;   // occupancy kernel: frame-interleaved grid.z so that a tile's column tiles share an XCD
    // og_unet_profile: the handle whose profile gets an entry per launch (nullptr: the detector's chain), the layer and its algorithmic FLOPs
    og_unet* prof = nullptr;
    const std::string* layer = nullptr;
    double flops = 0;
};

// One entry of og_unet_profile (kernel label + algorithmic FLOPs between two events): the constructor begins it, the destructor
// records its end -- OG_LAUNCH returns from the enclosing function when a launch fails, and no return can leave an entry open.
// The launchers format the label from their own template arguments, the ones that pick the kernel (nothing is formatted unless a
// profile is being taken).
struct ProfScope {
    og_unet* h;
    ProfScope(og_unet* h_, const char* layer, const char* kernel, double flops) : h(h_) { begin(layer, kernel, flops); }
    __attribute__((format(printf, 3, 4))) ProfScope(const LaunchCtx& c, const char* fmt, ...) : h(c.prof) {
        if (!h || !h->prof) return;
        char kernel[48];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(kernel, sizeof kernel, fmt, ap);
        va_end(ap);
        begin(c.layer->c_str(), kernel, c.flops);
    }
    ProfScope(const ProfScope&) = delete;
    ProfScope& operator=(const ProfScope&) = delete;
    ~ProfScope() {
        if (h && h->prof) (void)hipEventRecord(h->prof->back().e1, h->stream);
    }

private:
    void begin(const char* layer, const char* kernel, double flops) {
        if (!h || !h->prof) return;
        og_unet::ProfEntry e{layer, kernel, flops, nullptr, nullptr};
        (void)hipEventCreate(&e.e0);
        (void)hipEventCreate(&e.e1);
        (void)hipEventRecord(e.e0, h->stream);
        h->prof->push_back(e);
    }
};

// Runtime value -> template argument: f(og_const<V>{}) for the V of the list that equals v, the LAST one when none does (the
// launch sites list an option's special values first and its default last).  Every V listed is an instantiation that exists in the
// library, so a site lists exactly the values its kernel is shipped for.
template <int V0, int... Vs, typename F>
int og_pick(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) return f(og_const<V0>{});
    else return (v == V0) ? f(og_const<V0>{}) : og_pick<Vs...>(v, f);
}

// One operand of a conv launch as the kernels address it: base, frame stride, pixel stride and first channel, in 4-byte units
struct ConvView {
    float* p = nullptr;
    long long frame_stride = 0;
    int pix_stride = 0, ch_off = 0;
};

// What a conv launch of either net starts from: its operands, weights and affine, the zero page, and the neutral values of the
// rest (threshold 0.5, no split).  Every other field is zero / null until a path sets it, so nothing reaches a kernel uninitialised.
ConvArgs conv_args(const ConvView& in, const ConvView& out, const ConvView& pool, const ConvView& res, const float* wpk, const float* scale,
                   const float* shift, int aff_mod, const float* zero_page, int act) {
    ConvArgs a{};
    a.in = in.p;
    a.in_frame_stride = in.frame_stride;
    a.in_pix_stride = in.pix_stride;
    a.in_ch_off = in.ch_off;
    a.out = out.p;
    a.out_frame_stride = out.frame_stride;
    a.out_pix_stride = out.pix_stride;
    a.out_ch_off = out.ch_off;
    a.pool = pool.p;
    a.pool_frame_stride = pool.frame_stride;
    a.pool_pix_stride = pool.pix_stride;
    a.pool_ch_off = pool.ch_off;
    a.res = res.p;
    a.res_frame_stride = res.frame_stride;
    a.res_pix_stride = res.pix_stride;
    a.res_ch_off = res.ch_off;
    a.wpk = wpk;
    a.scale = scale;
    a.shift = shift;
    a.aff_mod = aff_mod;
    a.zero_page = zero_page;
    a.act = act;
    a.head_thr = 0.5f;
    a.ksplit = 1;
    a.vsplit = 1;
    return a;
}

// grid.z of every kernel that decodes blockIdx.z with og_zdecode: the layout is og_zlayout's (og_kernels.hpp, next to its inverse).
// `zdiv` = column tiles (x K parts) per spatial tile, `grid_tiles` = the GRID's tiles per frame (k_conv_wino_w<2> has half as many
// rows as a.tiles_y counts).  `wgs` > 0: the ungrouped forms, `wgs` workgroups per (frame, column tile) -- k_conv_wino_ps's 16 / PN,
// k_conv_wino_wp's 4, k_convt_w's 1.
// Sets a.frames, a.zdiv, a.zgroup_shift, a.zrcp; returns grid.z, or OG_EINVAL when it would pass the hardware's 65535.
int grid_z(const LaunchCtx& c, ConvArgs& a, int zdiv, int grid_tiles, int wgs = 0) {
    a.zdiv = zdiv;
    a.frames = a.n_spatial / (a.tiles_x * a.tiles_y);
    const og_zlay l = og_zlayout(a.frames, zdiv, grid_tiles, c.xcd_group, wgs);
    a.zgroup_shift = l.zgroup_shift;
    a.zrcp = l.zrcp;
    if (l.gz > 65535) return fail(OG_EINVAL, "micro-batch too large for one launch (grid.z): lower the chunk size");
    return (int)l.gz;
}

// Every launcher below takes its dynamic LDS size from the ConvTile its kernel takes its geometry from.
template <int NT, int MODE, int TH>
int launch_conv_t(const LaunchCtx& c, const ConvArgs& a, int n_ntiles) {
    constexpr int lds = ConvTile<NT, MODE, TH>::lds_bytes_2x(1);
    ProfScope ps(c, "k_conv_mfma<%d,%d,%d>", NT, MODE, TH);
    OG_LAUNCH_LDS((k_conv_mfma<NT, MODE, TH>), dim3((unsigned)(a.n_spatial * n_ntiles)), dim3(256), lds, c.stream, a);
    plan_inst("k_conv_mfma<%d, %d, %d>", NT, MODE, TH);
    return OG_OK;
}

// Split-K factor for a launch of `n_items` tiles over `n_chunks` 32-channel chunks: only when the
// launch would leave >= 3/4 of the workgroup slots empty (small-batch / latency mode), so that
// throughput-mode results do not depend on the micro-batch size.
inline int pick_ksplit(int n_items, int n_chunks, int slots, int ms, bool enable, int fill_div = 4) {
    if (!enable || n_chunks < 2 || n_items * fill_div > slots) return 1;
    int k = slots / n_items;
    if (k > n_chunks) k = n_chunks;
    const size_t per_item = (size_t)4 * ms * 16 * 64 * sizeof(float);
    while (k > 1 && (size_t)n_items * k * per_item > kPartialBytes) --k;
    return k < 1 ? 1 : k;
}

template <int NT, int MODE, int TH, int OCC, bool VS = false>
int launch_conv_o(const LaunchCtx& c, const ConvArgs& a_in, int n_ntiles) {
    constexpr int lds = ConvTile<NT, MODE, TH>::lds_bytes;
    static_assert(lds <= 160 * 1024, "one workgroup of this tile must fit a CU's LDS");
    ConvArgs a = a_in;
    a.stamps = nullptr;  // the probe buffer is sized for the persistent kernel's grid; this kernel's timeline is tools/ubench/occ_timeline
    if (VS) a.ksplit = 1;
    else a.vsplit = 1;
    if (a.n_spatial * n_ntiles > kTileCounters) a.tile_counter = nullptr;
    if ((MODE == 2 || MODE == 3) && a.tile_counter == nullptr) a.ksplit = 1;   // these modes split K with the fused reduce only
    ProfScope ps(c, "k_conv_mfma_o<%d,%d,%d>%s", NT, MODE, TH, a.ksplit > 1 ? "+splitK" : "");
    const int gz = grid_z(c, a, n_ntiles * a.ksplit, a.tiles_x * a.tiles_y);
    if (gz < 0) return gz;
    if (a.ksplit == 1) a.tile_counter = nullptr;
    if (a.ksplit > 1)   // raw accumulators of every K part (4 waves x MS sub-tiles x 16 registers x 64 lanes), arrivals per tile
        plan_need((long long)a.n_spatial * n_ntiles * a.ksplit * 4 * (((TH / 2) / (4 / NT)) * 16 * 64) * 4,
                  a.tile_counter ? (long long)a.n_spatial * n_ntiles : 0);
    OG_LAUNCH_LDS((k_conv_mfma_o<NT, MODE, TH, OCC, false, VS>), dim3(a.tiles_x, a.tiles_y, gz), dim3(256), lds, c.stream, a);
    plan_inst(VS ? "k_conv_mfma_o<%d, %d, %d, %d, false, true> vsplit=%d" : "k_conv_mfma_o<%d, %d, %d, %d, false, false> ksplit=%d", NT, MODE,
              TH, OCC, VS ? a.vsplit : a.ksplit);
    if constexpr (MODE == 0 || MODE == 1) {
        if (a.ksplit > 1 && a.tile_counter == nullptr) {
            OG_LAUNCH((k_splitk_epilogue<NT, MODE, TH>), dim3(a.n_spatial * n_ntiles), dim3(256), 4 * 5120, c.stream, a);
            plan_inst("k_splitk_epilogue<%d, %d, %d>", NT, MODE, TH);
        }
    }
    return OG_OK;
}

template <int NT>
constexpr int wino_lds() { return (32 / NT + 2) * 18 * (32 * NT) + 16 * 4096 + 2 * 8 * (32 * NT) * (32 * NT); }

template <int NT>
int launch_conv_wino(const LaunchCtx& c, const ConvArgs& a_in, int n_ntiles) {   // 16x16 (NT 2) / 32x16 (NT 1) pixel tiles, one workgroup per CU
    ConvArgs a = a_in;   // (a.stamps: diagnostic timeline, 8 x u64 for the first 511 workgroups)
    a.ksplit = 1;
    a.tile_counter = nullptr;
    ProfScope ps(c, "k_conv_wino<%d>", NT);
    const int gz = grid_z(c, a, n_ntiles, a.tiles_x * a.tiles_y);
    if (gz < 0) return gz;
    OG_LAUNCH_LDS(k_conv_wino<NT>, dim3(a.tiles_x, a.tiles_y, gz), dim3(256), wino_lds<NT>(), c.stream, a);
    plan_inst("k_conv_wino<%d>", NT);
    return OG_OK;
}

template <int NT, int PN>
constexpr int wino_ps_lds() {
    constexpr int KC = 8 * NT, raw_it = ((32 / NT + 2) * 18 * (KC / 4) + 255) / 256, up = 32 * NT * KC * 4, la = (PN <= 2) ? 3 : 2;
    return la * raw_it * 4096 + 2 * PN * 4096 + (la + 1) * ((PN * up > 4096) ? PN * up : 4096);
}

// k_conv_wino_ps: the same tiles as k_conv_wino, 16 / PN workgroups per (tile, column tile); needs the split-K workspace
// (raw accumulators: 256 KB per (tile, column tile)) and the arrival counters
template <int NT, int PN>
int launch_conv_wino_ps(const LaunchCtx& c, const ConvArgs& a_in, int n_ntiles) {
    constexpr int lds = wino_ps_lds<NT, PN>();
    ConvArgs a = a_in;   // (a.stamps: per-workgroup timeline of diagnostic runs, 4 x u64 for up to 1024 workgroups)
    a.ksplit = 1;
    ProfScope ps(c, "k_conv_wino_ps<%d,%d>", NT, PN);
    const int gz = grid_z(c, a, n_ntiles, a.tiles_x * a.tiles_y, 16 / PN);
    if (gz < 0) return gz;
    plan_need((long long)a.n_spatial * n_ntiles * (16 * 4 * 1024 * 4), (long long)a.n_spatial * n_ntiles);
    OG_LAUNCH_LDS((k_conv_wino_ps<NT, PN>), dim3(a.tiles_x, a.tiles_y, gz), dim3(256), lds, c.stream, a);
    plan_inst("k_conv_wino_ps<%d, %d>", NT, PN);
    return OG_OK;
}

template <int WB>
constexpr int wino_w_lds() {
    constexpr int raw_it = ((8 * WB + 2) * 18 * 8 + 255) / 256, ud = (WB == 1) ? 4 : 3;
    return 2 * raw_it * 4096 + (ud + 1) * 16384;
}

// k_conv_wino_w: 8 WB x 16-pixel tiles x 32 output channels, the 16 positions over the four waves; a.tiles_y counts 8-row tiles
// (the fused head's count slots), the grid has tiles_y / WB rows.  nt: the layer's canonical form (which weight pack a.wpk is)
template <int WB>
int launch_conv_wino_w(const LaunchCtx& c, const ConvArgs& a_in, int n_ntiles, int nt) {
    ConvArgs a = a_in;   // (a.stamps: per-workgroup timeline of diagnostic runs, 4 x u64 for up to 1024 workgroups)
    a.ksplit = 1;
    a.tile_counter = nullptr;
    const int gy = a.tiles_y / WB;
    ProfScope ps(c, "k_conv_wino_w<%d,%d>", nt, WB);
    const int gz = grid_z(c, a, n_ntiles, a.tiles_x * gy);
    if (gz < 0) return gz;
    OG_LAUNCH_LDS(k_conv_wino_w<WB>, dim3(a.tiles_x, gy, gz), dim3(256), wino_w_lds<WB>(), c.stream, a);
    plan_inst("k_conv_wino_w<%d> nt=%d", WB, nt);
    return OG_OK;
}

constexpr int kWinoWpLds = 3 * 6 * 4096 + 9 * 4096;

// k_conv_wino_wp: k_conv_wino_w<1>'s tiles, a tile's four position rows on four workgroups (grid.z x 4); needs the split-K workspace
// (64 KB per tile) and the arrival counters.  nt: as for k_conv_wino_w
int launch_conv_wino_wp(const LaunchCtx& c, const ConvArgs& a_in, int n_ntiles, int nt) {
    ConvArgs a = a_in;   // (a.stamps: per-workgroup timeline of diagnostic runs, 4 x u64 for up to 1024 workgroups)
    a.ksplit = 1;
    ProfScope ps(c, "k_conv_wino_wp<%d>", nt);
    const int gz = grid_z(c, a, n_ntiles, a.tiles_x * a.tiles_y, 4);
    if (gz < 0) return gz;
    plan_need((long long)a.n_spatial * n_ntiles * 65536, (long long)a.n_spatial * n_ntiles);
    OG_LAUNCH_LDS(k_conv_wino_wp, dim3(a.tiles_x, a.tiles_y, gz), dim3(256), kWinoWpLds, c.stream, a);
    plan_inst("k_conv_wino_wp nt=%d", nt);
    return OG_OK;
}

// k_convt_w: the transposed conv on 32-pixel x 32-column wave tiles (operands straight to registers, no LDS); grid.z = frame x
// column tile of 32 / 4 per workgroup
int launch_convt_w(const LaunchCtx& c, const ConvArgs& a_in, int n_ntiles) {
    ConvArgs a = a_in;
    ProfScope ps(c, "k_convt_w<1,1,8>");
    const int gz = grid_z(c, a, n_ntiles, a.tiles_x * a.tiles_y, 1);
    if (gz < 0) return gz;
    OG_LAUNCH(k_convt_w, dim3(a.tiles_x, (a.H + 1) / 2, gz), dim3(256), 0, c.stream, a);
    return OG_OK;
}

template <int NT, int MODE, int TH, int OCC, bool SQ = false>
int launch_conv_h(const LaunchCtx& c, const ConvArgs& a_in, int n_ntiles) {   // split-precision twin of launch_conv_o
    constexpr int lds = ConvTile<NT, MODE, TH, SQ>::lds_bytes;
    static_assert(lds <= 160 * 1024, "one workgroup of this tile must fit a CU's LDS");
    ConvArgs a = a_in;
    a.stamps = nullptr;
    if (SQ || a.tile_counter == nullptr || a.partial == nullptr || a.n_spatial * n_ntiles > kTileCounters) a.ksplit = 1;   // fused reduce only
    ProfScope ps(c, "k_conv_mfma_h<%d,%d,%d>", NT, MODE, TH);
    const int gz = grid_z(c, a, n_ntiles * a.ksplit, a.tiles_x * a.tiles_y);
    if (gz < 0) return gz;
    OG_LAUNCH_LDS((k_conv_mfma_h<NT, MODE, TH, OCC, false, SQ>), dim3(a.tiles_x, a.tiles_y, gz), dim3(256), lds, c.stream, a);
    plan_inst("k_conv_mfma_h<%d, %d, %d, %d, false, %s> ksplit=%d", NT, MODE, TH, OCC, SQ ? "true" : "false", a.ksplit);
    return OG_OK;
}

template <int NT, int MODE, int TH, int OCC, bool SQ = false>
int launch_conv_f(const LaunchCtx& c, const ConvArgs& a_in, int n_ntiles) {   // f16-mode twin of launch_conv_h (never splits K)
    constexpr int lds = ConvTile<NT, MODE, TH, SQ>::lds_bytes;
    static_assert(lds <= 160 * 1024, "one workgroup of this tile must fit a CU's LDS");
    ConvArgs a = a_in;
    a.stamps = nullptr;
    a.ksplit = 1;
    a.tile_counter = nullptr;
    ProfScope ps(c, "k_conv_mfma_f<%d,%d,%d>", NT, MODE, TH);
    const int gz = grid_z(c, a, n_ntiles, a.tiles_x * a.tiles_y);
    if (gz < 0) return gz;
    OG_LAUNCH_LDS((k_conv_mfma_f<NT, MODE, TH, OCC, false, SQ>), dim3(a.tiles_x, a.tiles_y, gz), dim3(256), lds, c.stream, a);
    // (with the K walk it was given: 64-channel chunks, and whether the last one is a half)
    plan_inst("(k_conv_mfma_f<%d, %d, %d, %d, false, %s>) chunks=%d k_half=%d", NT, MODE, TH, OCC, SQ ? "true" : "false", a.n_chunks, a.k_half);
    return OG_OK;
}

// the two reduced-precision families take the same instantiations: the handle's "precision" names the family
template <int NT, int MODE, int TH, int OCC, bool SQ = false>
int launch_conv_hf(const LaunchCtx& c, const ConvArgs& a, int n_ntiles, bool f16) {
    return f16 ? launch_conv_f<NT, MODE, TH, OCC, SQ>(c, a, n_ntiles) : launch_conv_h<NT, MODE, TH, OCC, SQ>(c, a, n_ntiles);
}

template <int NT, int MODE, int TH, int TPS>
int launch_conv_p(const LaunchCtx& c, const ConvArgs& a, int n_ntiles) {
    constexpr int lds = ConvTile<NT, MODE, TH>::lds_bytes_2x(TPS);
    const int n_items = a.n_spatial * n_ntiles * a.ksplit;
    const int slots = c.n_cu * ((lds > 80 * 1024) ? 1 : c.wg_per_cu);
    const int rounds = (n_items + slots - 1) / slots;
    const int grid = (n_items + rounds - 1) / rounds;  // <= slots, balanced: every workgroup gets rounds or rounds-1 items
    ProfScope ps(c, "k_conv_mfma_p<%d,%d,%d,%d>", NT, MODE, TH, TPS);
    if (a.ksplit > 1) plan_need((long long)n_items * 4 * (((TH / 2) / (4 / NT)) * 16 * 64) * 4, 0);
    OG_LAUNCH_LDS((k_conv_mfma_p<NT, MODE, TH, TPS>), dim3(grid), dim3(256), lds, c.stream, a, n_items);
    plan_inst("k_conv_mfma_p<%d, %d, %d, %d> ksplit=%d", NT, MODE, TH, TPS, a.ksplit);
    if (a.ksplit > 1) {
        OG_LAUNCH((k_splitk_epilogue<NT, MODE, TH>), dim3(a.n_spatial * n_ntiles), dim3(256), 4 * 5120, c.stream, a);
        plan_inst("k_splitk_epilogue<%d, %d, %d>", NT, MODE, TH);
    }
    return OG_OK;
}

// Which Winograd kernel runs a 3x3 layer that takes the Winograd form (decided by the caller from options and (H, W) alone):
// 0 = k_conv_wino / k_conv_wino_ps, 1 / 2 = k_conv_wino_w<WB>, 4 = k_conv_wino_wp.  All of them compute the same bits, so B may
// enter here.
int pick_wino_w(const og_unet* h, const ConvLayer& L, int B, int H, int W) {
    if (!h->wino_w || (L.NT == 2 && L.d_ww1 == nullptr) || H % 8 || W % 16) return 0;
    const long long w1 = (long long)B * (W / 16) * (H / 8) * (L.Cout_p / 32);   // 8 x 16-pixel x 32-channel tiles
    const bool wp_ok = h->d_partial != nullptr && h->d_tile_counter != nullptr && w1 <= kTileCounters && w1 * 65536 <= (long long)kPartialBytes;
    if (h->wino_w == 2) return 1;
    if (h->wino_w == 3) return (H % 16 == 0) ? 2 : 1;
    if (h->wino_w == 4) return wp_ok ? 4 : 1;
    const long long wgs_wino = (long long)B * (W / 16) * (H / (32 / L.NT)) * (L.Cout_p / (32 * L.NT));
    if (wgs_wino * 2 > h->n_cu) return 0;   // k_conv_wino covers more than half of the chip: its larger tiles stream less
    // One chain at a time (one lane): latency counts -- a k_conv_wino_w workgroup runs Cin / 8 chunks of 16 MFMAs per wave back to
    // back, so layers with few tiles and hundreds of channels also split the position rows (measured at one frame: 64 tiles and
    // fewer; 128 tiles are faster unsplit up to 256 channels).  Several lanes in flight: occupancy counts -- the unsplit kernel
    // stages and transforms every halo once and exchanges nothing through memory (half the CU-time per layer), and the other
    // lanes' launches fill the CUs it leaves idle (3 lanes, one frame per chain: 5.0 k frames/s against 4.4 k).
    if (h->active_lanes <= 1 && w1 * 4 <= h->n_cu && wp_ok) return 4;
    return (w1 >= 2 * h->n_cu && H % 16 == 0) ? 2 : 1;
}

// in: activation view + channel offset/count; out likewise; pool optional
int launch_conv(og_unet* h, const ConvLayer& L, int B, const Act& in, int in_off, const Act& out, int out_off, const Act* pool) {
    constexpr int TH = 8;
    if (h->inject_fault > 0 && --h->inject_fault == 0 && !g_plan) {
        if (h->d_tile_counter) (void)hipMemsetAsync(h->d_tile_counter, 0x01, kTileCounters * sizeof(int), h->stream);
        return fail(OG_EHIP, "injected launch failure (option inject_fault)");
    }
    if (L.mode == 0 && (out.H != in.H || out.W != in.W)) return fail(OG_EINVAL, "conv shape mismatch");
    if (L.mode != 0 && (out.H != 2 * in.H || out.W != 2 * in.W)) return fail(OG_EINVAL, "convT shape mismatch");
    // 16x16 tiles only for the 3x3 convs of the persistent kernel, and only when every tile is full
    const bool full16 = (L.mode == 0 && in.H % 16 == 0 && in.W % 16 == 0);
    bool big = full16 && h->tile_h == 16 && (h->conv_impl == 1 || h->conv_impl == 2);
    // auto: staged bytes per MFMA fall 42 % with 16x16 tiles (measured +2-3 % on the deep layers), but the
    // high-resolution layers and the 32-column kernel prefer three 8x16 workgroups per CU
    if (h->conv_impl == 2 && h->tile_h == 0) big = full16 && L.NT == 2 && in.H <= 64 && in.W <= 64;
    if (h->fuse.active) big = false;  // per-tile count slots are laid out for 8x16 tiles
    // F layout (f16 mode): the views' strides are already in 4-byte units (arena_layout); channel offsets become such units here
    const int cdiv = (h->precision == 2) ? 2 : 1;
    ConvArgs a = conv_args({in.p, in.frame_stride(), in.C, in_off / cdiv}, {out.p, out.frame_stride(), out.C, out_off / cdiv},
                           pool ? ConvView{pool->p, pool->frame_stride(), pool->C, 0} : ConvView{}, ConvView{}, L.d_w, L.d_scale, L.d_shift,
                           L.Cout_p, h->d_zero, (L.mode == 0) ? 1 : 0);
    a.n_chunks = L.Cin_p / 32;
    a.H = in.H;
    a.W = in.W;
    a.tiles_x = (in.W + 15) / 16;
    auto set_tile_h = [&](int th) {   // rows of a spatial tile: 16 (`big`) or 8
        a.tiles_y = (in.H + th - 1) / th;
        a.n_spatial = B * a.tiles_x * a.tiles_y;
    };
    set_tile_h(big ? 16 : 8);
    a.prio_mode = h->prio_mode;
    a.range_flag = h->d_range;
    if (h->fuse.active) {  // set by enqueue_last_with_head for exactly one launch
        a.head_w = h->d_head_w;
        a.head_bias = h->head_bias;
        a.head_thr = h->fuse.thr;
        a.head_boxes = h->fuse.boxes;
        a.head_logits = h->fuse.logits;
        a.head_mask = h->fuse.mask;
        a.head_area = h->fuse.area;
        a.head_store_act = h->keep_taps;
    }
    a.partial = h->d_partial;
    a.tile_counter = (h->splitk_fused && h->d_tile_counter) ? h->d_tile_counter : nullptr;
    const double px = (double)B * in.H * in.W;
    const LaunchCtx ctx{h->stream, h->n_cu, h->wg_per_cu, h->xcd_group, h, &L.name, 2.0 * px * ((L.mode == 0) ? 9.0 : 4.0) * L.Cin * L.Cout};
    // column tiles of the launch: 32 NT output channels each; the transposed conv is one GEMM with N = 4 Cout on 64-column tiles
    const int n_ntiles = (L.mode == 0) ? L.Cout_p / (32 * L.NT) : 4 * L.Cout_p / 64;
    if (h->precision != 0) {   // opt-in split precision (1: k_conv_mfma_h) / f16 mode (2: k_conv_mfma_f): always the occupancy-shaped kernel
        const bool f16 = h->precision == 2;
        // tile height: an MFMA step is 5x shorter here than in the f32 kernels, so barriers and staged bytes per MFMA weigh
        // more: 16-row tiles wherever they tile the image ("tile_h" 8 forces 8 rows, 16 / 0 = this rule)
        big = full16 && h->tile_h != 8;
        if (a.head_w != nullptr) big = false;   // per-tile count slots of the fused head are laid out for 8x16 tiles
        if (f16) {   // F layout: K walks 64-channel chunks; never split-K ("splitk" is refused)
            a.n_chunks = (L.Cin_p + 63) / 64;
            a.k_half = (L.Cin_p % 64) ? 1 : 0;
            a.wpk = L.d_w_f;
        } else {   // small launches (one frame per chain): split K over workgroups exactly as the f32 occupancy kernel does
            const int tiles8 = B * a.tiles_x * ((in.H + 7) / 8);
            const int k_units = a.n_chunks;   // whole channel chunks: finer parts measured 2 % slower on these (5x shorter) steps
            const int ks = pick_ksplit(tiles8 * n_ntiles, k_units, h->n_cu * h->splitk_slots, (L.NT == 2) ? 2 : 1,
                                       h->splitk != 0 && h->d_partial != nullptr && h->d_tile_counter != nullptr, h->splitk_div);
            a.ksplit = (ks > 1 && a.head_w == nullptr) ? ks : 1;
            if (a.ksplit > 1) big = false;
            a.wpk = L.d_w_h;
        }
        set_tile_h(big ? 16 : 8);
        if (L.mode != 0) return launch_conv_hf<2, 1, 8, 3>(ctx, a, n_ntiles, f16);
        return og_pick<2, 1>(L.NT, [&](auto nt) {
            constexpr int NT = decltype(nt)::value;
            if constexpr (NT == 2) {   // 16x16 tiles of the 64-column kernel: 2x2 sub-tiles per wave ("h_square")
                if (big && h->h_square) return launch_conv_hf<2, 0, 16, 2, true>(ctx, a, n_ntiles, f16);
            }
            return big ? launch_conv_hf<NT, 0, 16, 2>(ctx, a, n_ntiles, f16) : launch_conv_hf<NT, 0, 8, 3>(ctx, a, n_ntiles, f16);
        });
    }
    int impl = h->conv_impl;
    int NTu = L.NT;   // column sub-tiles per workgroup of THIS launch (32-column tiles on split 3x3 launches, see splitk_nt1)
    // Winograd form of this layer?  Decided from the handle's options and the layer's shape only (B plays no part).
    const bool use_wino = L.mode == 0 && h->wino_chain && L.d_ww != nullptr && full16 && (L.NT == 2 || in.H % 32 == 0) &&
                          (a.head_w == nullptr || L.NT == 1);
    if (!use_wino && (impl == 1 || impl == 2)) {
        const bool sk_occ = (impl == 2 && h->splitk_occ);
        const int tiles8 = B * a.tiles_x * ((in.H + 7) / 8);
        // occupancy split-K of a 3x3 conv: parts are ranges of (chunk, tap) steps, at least splitk_min_steps each
        const int k_units = (sk_occ && L.mode == 0) ? (a.n_chunks * 9) / h->splitk_min_steps : a.n_chunks;
        int ks = pick_ksplit(tiles8 * n_ntiles, k_units, h->n_cu * (sk_occ ? h->splitk_slots : h->wg_per_cu), (L.NT == 2) ? 2 : 1,
                             h->splitk != 0 && h->d_partial != nullptr, sk_occ ? h->splitk_div : 4);
        bool nt1 = false;   // 32-column tiles where they still leave room to split K
        if (ks > 1 && sk_occ && h->splitk_nt1 && L.mode == 0 && L.NT == 2 && L.d_w1 != nullptr) {
            const int ks1 = pick_ksplit(tiles8 * n_ntiles * 2, k_units, h->n_cu * h->splitk_slots, 1, true, h->splitk_div);
            if (ks1 > 1) {
                ks = ks1;
                nt1 = true;
            }
        }
        // The occupancy variant needs at least one full round of workgroups (2/CU on 16x16 tiles, 3/CU on
        // 8x16); below that the persistent kernel (2/CU, balanced static schedule, split-K when the launch
        // cannot even fill a quarter of the chip) is faster.
        const bool occ_fills = h->occ_min_pct ? (a.n_spatial * n_ntiles * 100 >= h->n_cu * h->occ_min_pct)
                                              : (a.n_spatial * n_ntiles >= h->n_cu * (big ? 2 : 3));
        const bool split = (ks > 1 && a.head_w == nullptr);  // the fused head lives in the conv epilogue: no split-K on that launch
        if (split || (impl == 2 && !occ_fills)) {
            // h->splitk_occ: the K parts run on the (leaner) occupancy kernel, one workgroup per part; else the persistent kernel
            impl = (split && impl == 2 && h->splitk_occ) ? 4 : 1;
            big = false;
            set_tile_h(8);
            a.ksplit = split ? ks : 1;
            if (impl == 4 && nt1) {
                NTu = 1;
                a.wpk = L.d_w1;
            }
        }
    }
    if (h->probing && h->prof && h->d_stamps) {  // diagnostic clock stamps: og_unet_clock_probe only
        a.stamps = h->d_stamps + 4 * 1024 * h->prof->size();
    }
    if (L.mode == 0) {
        if (use_wino) {
            if (const int wb = pick_wino_w(h, L, B, in.H, in.W)) {
                set_tile_h(8);
                a.wpk = (L.NT == 2) ? L.d_ww1 : L.d_ww;
                if (wb == 4) {
                    a.partial = h->d_partial;
                    a.tile_counter = h->d_tile_counter;
                    return launch_conv_wino_wp(ctx, a, L.Cout_p / 32, L.NT);
                }
                return (wb == 1) ? launch_conv_wino_w<1>(ctx, a, L.Cout_p / 32, L.NT) : launch_conv_wino_w<2>(ctx, a, L.Cout_p / 32, L.NT);
            }
            set_tile_h(32 / L.NT);
            a.wpk = L.d_ww;
            // A launch that leaves most of the chip idle (one frame per chain, deep layers of small micro-batches) spreads the 16
            // Winograd positions of a tile over 16 / PN workgroups (k_conv_wino_ps): the same sums, bit for bit -- a scheduling
            // choice, which is why it MAY depend on B.  PN = the coarsest split that still gives every CU a workgroup; launches
            // that fill a quarter of the chip or more stay on k_conv_wino (measured at one frame: 128 workgroups of k_conv_wino
            // beat 512 of the split form on the 256x256 layers, 64 lose to 256 on the 128x128 ones).
            const long long wgs = (long long)a.n_spatial * n_ntiles;
            int pn = 0;
            if (h->wino_ps && h->d_partial != nullptr && h->d_tile_counter != nullptr && wgs * 4 <= h->n_cu && wgs <= kTileCounters &&
                (size_t)wgs * (16 * 4 * 1024 * sizeof(float)) <= kPartialBytes) {
                pn = (wgs * 4 >= h->n_cu) ? 4 : (wgs * 8 >= h->n_cu) ? 2 : 1;
                if (h->wino_ps > 1) pn = (h->wino_ps == 2) ? 4 : (h->wino_ps == 3) ? 2 : 1;   // forced (tests, A/B)
            }
            if (pn) {
                a.partial = h->d_partial;
                a.tile_counter = h->d_tile_counter;
            }
            return og_pick<2, 1>(L.NT, [&](auto nt) {
                constexpr int NT = decltype(nt)::value;
                if (!pn) return launch_conv_wino<NT>(ctx, a, n_ntiles);
                return og_pick<1, 2, 4>(pn, [&](auto pn_) { return launch_conv_wino_ps<NT, decltype(pn_)::value>(ctx, a, n_ntiles); });
            });
        }
        // the direct kernels, by the width of this launch's column tiles
        return og_pick<2, 1>(NTu, [&](auto nt) {
            constexpr int NT = decltype(nt)::value;
            if (impl == 0) return launch_conv_t<NT, 0, TH>(ctx, a, n_ntiles);
            if (impl == 2 && big) return launch_conv_o<NT, 0, 16, 2>(ctx, a, n_ntiles);
            if (impl == 4) return launch_conv_o<NT, 0, TH, 3>(ctx, a, L.Cout_p / (32 * NT));
            if (impl == 2) return launch_conv_o<NT, 0, TH, 3>(ctx, a, n_ntiles);
            if (impl == 3) return launch_conv_o<NT, 0, TH, 4>(ctx, a, n_ntiles);
            // the persistent kernel: taps per step by option ("tps_nt2", "tps_nt1")
            if constexpr (NT == 2) {
                return og_pick<3, 1>(h->tps_nt2, [&](auto tps) {
                    constexpr int TPS = decltype(tps)::value;
                    return big ? launch_conv_p<2, 0, 16, TPS>(ctx, a, n_ntiles) : launch_conv_p<2, 0, TH, TPS>(ctx, a, n_ntiles);
                });
            } else {
                if (big) return og_pick<9, 3>(h->tps_nt1, [&](auto tps) { return launch_conv_p<1, 0, 16, decltype(tps)::value>(ctx, a, n_ntiles); });
                return og_pick<9, 3, 1>(h->tps_nt1, [&](auto tps) { return launch_conv_p<1, 0, TH, decltype(tps)::value>(ctx, a, n_ntiles); });
            }
        });
    }
    // a launch that leaves most of the chip idle (one frame per chain): the same sums on 32-pixel x 32-column wave tiles -- a
    // scheduling choice among bit-identical kernels, so B may enter
    if (h->conv_impl == 2 && a.ksplit == 1 && h->convt_w && L.d_w1 != nullptr && (long long)B * a.tiles_x * ((in.H + 7) / 8) * n_ntiles * 2 <= h->n_cu) {
        a.wpk = L.d_w1;
        return launch_convt_w(ctx, a, L.Cout_p / 32);
    }
    if (impl == 0) return launch_conv_t<2, 1, TH>(ctx, a, n_ntiles);
    if (impl == 4 || (impl >= 2 && h->convt_occ)) return launch_conv_o<2, 1, TH, 3>(ctx, a, n_ntiles);
    return launch_conv_p<2, 1, TH, 1>(ctx, a, n_ntiles);
}

enum { KIND_U8 = 0, KIND_F32 = 1 };

// The chain is: k_conv_first (reads the caller's frames) -> body (arena only) -> k_head
// (writes the caller's outputs).  Only the body is pointer-stable, so only the body is
// captured into a hipGraph (keyed by B,H,W); first and head are plain launches around it.
int enqueue_first(og_unet* h, int kind, const void* in, int B, int H, int W) {
    const int Cp0 = cp32(h->features[0]);
    const int tiles = ((W + 15) / 16) * ((H + 15) / 16);
    const Act& o = h->A[0];
    ProfScope ps(h, "downs.0.net.0.weight", h->precision == 2 ? (kind == KIND_U8 ? "k_conv_first_f<u8>" : "k_conv_first_f<f32>")
                                            : kind == KIND_U8 ? "k_conv_first<u8>" : "k_conv_first<f32>",
                 2.0 * B * H * W * 9.0 * h->features[0]);
    if (h->precision == 2 && kind == KIND_U8)
        OG_LAUNCH(k_conv_first_f<uint8_t>, dim3(B * tiles), dim3(256), 0, h->stream, (const uint8_t*)in, o.p,
                           h->d_first_w, h->d_first_scale, h->d_first_shift, H, W, Cp0, o.C, o.frame_stride(), h->d_range);
    else if (h->precision == 2)
        OG_LAUNCH(k_conv_first_f<float>, dim3(B * tiles), dim3(256), 0, h->stream, (const float*)in, o.p,
                           h->d_first_w, h->d_first_scale, h->d_first_shift, H, W, Cp0, o.C, o.frame_stride(), h->d_range);
    else if (kind == KIND_U8 && h->precision == 1)
        OG_LAUNCH((k_conv_first<uint8_t, true>), dim3(B * tiles), dim3(256), 0, h->stream, (const uint8_t*)in, o.p,
                           h->d_first_w, h->d_first_scale, h->d_first_shift, H, W, Cp0, o.C, o.frame_stride(), h->d_range);
    else if (kind == KIND_U8)
        OG_LAUNCH(k_conv_first<uint8_t>, dim3(B * tiles), dim3(256), 0, h->stream, (const uint8_t*)in, o.p,
                           h->d_first_w, h->d_first_scale, h->d_first_shift, H, W, Cp0, o.C, o.frame_stride(), (int*)nullptr);
    else if (h->precision == 1)
        OG_LAUNCH((k_conv_first<float, true>), dim3(B * tiles), dim3(256), 0, h->stream, (const float*)in, o.p,
                           h->d_first_w, h->d_first_scale, h->d_first_shift, H, W, Cp0, o.C, o.frame_stride(), h->d_range);
    else
        OG_LAUNCH(k_conv_first<float>, dim3(B * tiles), dim3(256), 0, h->stream, (const float*)in, o.p,
                           h->d_first_w, h->d_first_scale, h->d_first_shift, H, W, Cp0, o.C, o.frame_stride(), (int*)nullptr);
    return OG_OK;
}

// downs.0's second conv with the first layer computed inside it (u8 frames in, no intermediate tensor).
// Only the occupancy variant has the in-kernel producer; needs f0 <= 32, a launch that fills the chip,
// and nobody asking for the "downs.0.a" tap.
bool can_fuse_first(const og_unet* h, int kind, int B, int H, int W) {
    if (!h->fuse_first || kind != KIND_U8 || h->conv_impl != 2 || h->keep_taps || cp32(h->features[0]) != 32) return false;
    // Winograd chain: the second conv runs as k_conv_wino<1> on the first layer's stored output (less work than the fusion saves)
    if (h->wino_chain && h->wino_first && H % 32 == 0 && W % 16 == 0) return false;
    const int items = B * ((W + 15) / 16) * ((H + 7) / 8);
    return items >= 3 * h->n_cu;
}

int enqueue_first_fused(og_unet* h, const uint8_t* gray, int B, int H, int W) {
    const ConvLayer& L = h->enc_b[0];
    const Act& out = h->CAT[0];
    const Act& pool = h->P[0];
    ConvArgs a{};   // no input view (the kernel reads the u8 frame), one column tile, no split: everything not set here is zero / null
    a.n_chunks = 1;
    a.H = H;
    a.W = W;
    a.tiles_x = (W + 15) / 16;
    a.tiles_y = (H + 7) / 8;
    a.n_spatial = B * a.tiles_x * a.tiles_y;
    a.wpk = (h->precision == 2) ? L.d_w_f : (h->precision == 1) ? L.d_w_h : L.d_w;
    a.k_half = (h->precision == 2) ? 1 : 0;   // 32 input channels: half a 64-channel chunk
    a.scale = L.d_scale;
    a.shift = L.d_shift;
    a.aff_mod = L.Cout_p;
    a.out = out.p;
    a.out_frame_stride = out.frame_stride();
    a.out_pix_stride = out.C;
    a.pool = pool.p;
    a.pool_frame_stride = pool.frame_stride();
    a.pool_pix_stride = pool.C;
    a.zero_page = h->d_zero;
    a.act = 1;
    a.ksplit = 1;
    a.range_flag = h->d_range;
    a.first_u8 = gray;
    a.first_w9 = h->d_first_w;
    a.first_scale = h->d_first_scale;
    a.first_shift = h->d_first_shift;
    if (h->precision != 0) a.prio_mode = h->prio_mode;
    using T = ConvTile<1, 0, 8>;   // of all three FIRST kernels below
    constexpr int lds = T::lds_bytes + T::first_bytes;
    static_assert(3 * lds <= 160 * 1024, "three workgroups of the fused first layer per CU");
    ProfScope ps(h, "downs.0 (first + second conv fused)", h->precision == 2 ? "k_conv_mfma_f<1,0,8,FIRST>" : h->precision == 1 ? "k_conv_mfma_h<1,0,8,FIRST>" : "k_conv_mfma_o<1,0,8,FIRST>",
                 2.0 * B * H * W * 9.0 * (1.0 * h->features[0] + (double)h->features[0] * h->features[0]));
    const int gz = grid_z(LaunchCtx{h->stream, h->n_cu, h->wg_per_cu, h->xcd_group}, a, 1, a.tiles_x * a.tiles_y);   // one column tile: grid.z = B
    if (gz < 0) return gz;
    if (h->precision == 2) {
        OG_LAUNCH_LDS((k_conv_mfma_f<1, 0, 8, 3, true>), dim3(a.tiles_x, a.tiles_y, gz), dim3(256), lds, h->stream, a);
        plan_inst("(k_conv_mfma_f<1, 0, 8, 3, true>) chunks=%d k_half=%d", a.n_chunks, a.k_half);
    } else if (h->precision == 1)
        OG_LAUNCH_LDS((k_conv_mfma_h<1, 0, 8, 3, true>), dim3(a.tiles_x, a.tiles_y, gz), dim3(256), lds, h->stream, a);
    else
        OG_LAUNCH_LDS((k_conv_mfma_o<1, 0, 8, 3, true>), dim3(a.tiles_x, a.tiles_y, gz), dim3(256), lds, h->stream, a);
    return OG_OK;
}

bool can_fuse_head(const og_unet* h) {
    if (h->precision == 1 && h->keep_taps) return false;   // the fused head keeps the f32 scratch: no H-layout activation to tap
    return h->fuse_head && h->conv_impl != 0 && cp32(h->features[0]) == 32;
}

int enqueue_body(og_unet* h, int B, bool skip_last = false, bool skip_first = false) {
    const int L = h->L;
    int rc;
    for (int i = 0; i < L; ++i) {
        if (i > 0 && (rc = launch_conv(h, h->enc_a[i], B, h->P[i - 1], 0, h->A[i], 0, nullptr))) return rc;
        if (i == 0 && skip_first) continue;  // downs.0 ran as one fused launch in front of the graph
        if ((rc = launch_conv(h, h->enc_b[i], B, h->A[i], 0, h->CAT[i], 0, &h->P[i]))) return rc;
    }
    if ((rc = launch_conv(h, h->bott_a, B, h->P[L - 1], 0, h->BA, 0, nullptr))) return rc;
    if ((rc = launch_conv(h, h->bott_b, B, h->BA, 0, h->BB, 0, nullptr))) return rc;
    for (int j = 0; j < L; ++j) {
        const int i = L - 1 - j;
        const Act& src = (j == 0) ? h->BB : h->UB[i + 1];
        const int Ci = cp32(h->features[i]);
        if ((rc = launch_conv(h, h->up_t[j], B, src, 0, h->CAT[i], Ci, nullptr))) return rc;
        if ((rc = launch_conv(h, h->dec_a[j], B, h->CAT[i], 0, h->UA[i], 0, nullptr))) return rc;
        if (skip_last && j == L - 1) break;
        if ((rc = launch_conv(h, h->dec_b[j], B, h->UA[i], 0, h->UB[i], 0, nullptr))) return rc;
    }
    return OG_OK;
}

// Last conv (ups.N.net.3) with the head fused into its epilogue: replaces k_head and the 8 MB/frame round trip.
int enqueue_last_with_head(og_unet* h, int B, float thr, const int32_t* boxes, uint8_t* mask, int32_t* area, float* logits) {
    const int L = h->L;
    const Act& u = h->UA[0];
    // count slots per frame: the fused launch runs on 8x16 tiles (direct kernel) or on 32x16 tiles (k_conv_wino<1>)
    const bool wino_last = h->wino_chain && h->dec_b[L - 1].d_ww != nullptr && u.H % 32 == 0 && u.W % 16 == 0 &&
                           !pick_wino_w(h, h->dec_b[L - 1], B, u.H, u.W);   // k_conv_wino_w counts per 8x16 tile, like the direct kernel
    const int tiles = wino_last ? (u.W / 16) * (u.H / 32) : ((u.W + 15) / 16) * ((u.H + 7) / 8);
    const size_t need = (size_t)B * tiles * 4;
    if (area && need > h->counts_cap && !g_plan) {
        if (h->d_counts) {
            HIPCHK(hipStreamSynchronize(h->stream));
            HIPCHK(hipFree(h->d_counts));
            h->d_counts = nullptr;
        }
        HIPCHK(hipMalloc((void**)&h->d_counts, need * sizeof(int32_t)));
        h->counts_cap = need;
    }
    h->fuse.active = true;
    h->fuse.thr = thr;
    h->fuse.boxes = boxes;
    h->fuse.mask = mask;
    // (tried in round 4: up to 4 frames per launch adding their per-wave counts atomically into the per-frame total instead of
    //  count slots + k_sum_counts -- 2 048 atomics onto one address per frame cost more than the 4.7 us launch: 310 -> 326 us per frame)
    h->fuse.area = area ? h->d_counts : nullptr;
    h->fuse.logits = logits;
    const int rc = launch_conv(h, h->dec_b[L - 1], B, u, 0, h->UB[0], 0, nullptr);
    h->fuse.active = false;
    if (rc) return rc;
    if (area) {
        OG_LAUNCH(k_sum_counts, dim3(B), dim3(256), 0, h->stream, h->d_counts, tiles * 4, area);
    }
    return OG_OK;
}

int enqueue_head(og_unet* h, int B, int H, int W, float thr, const int32_t* boxes, uint8_t* mask, int32_t* area, float* logits) {
    const Act& u = h->UB[0];
    const int HW = H * W;
    const int bpf = (HW + 1023) / 1024;
    ProfScope ps(h, "head", h->precision == 2 ? "k_head_f" : "k_head", 2.0 * B * HW * h->features[0]);
    if (h->precision == 2)
        OG_LAUNCH(k_head_f, dim3(B * bpf), dim3(256), 0, h->stream, u.p, u.frame_stride(), u.C, h->d_head_w,
                           h->head_bias, cp32(h->features[0]), HW, W, thr, boxes, logits, mask, area, bpf);
    else if (h->precision == 1)
        OG_LAUNCH(k_head<true>, dim3(B * bpf), dim3(256), 0, h->stream, u.p, u.frame_stride(), u.C, h->d_head_w,
                           h->head_bias, cp32(h->features[0]), HW, W, thr, boxes, logits, mask, area, bpf);
    else
        OG_LAUNCH(k_head<false>, dim3(B * bpf), dim3(256), 0, h->stream, u.p, u.frame_stride(), u.C, h->d_head_w,
                           h->head_bias, cp32(h->features[0]), HW, W, thr, boxes, logits, mask, area, bpf);
    return OG_OK;
}

// One chunk of B (<= capB) frames.  Body eager, or replayed from a cached hipGraph
// (launch-bound at small B otherwise: 5*L+2 launches, MI355X_MICROARCH.md "graph-replay-floor").
// The arithmetic form of the chain is a property of the HANDLE (options) -- never of B: a ragged tail, a short shard and a
// one-frame call run the same per-output sums as a chip-filling micro-batch (launch_conv then picks, per layer, from (H, W)
// alone whether the map tiles for k_conv_wino).  Round 2 chose per micro-batch and a frame's area depended on its neighbours.
void pick_chain_form(og_unet* h, int /*B*/, int /*H*/, int /*W*/) {
    h->wino_chain = h->wino && h->precision == 0 && h->conv_impl == 2;
}

int run_chunk(og_unet* h, int kind, const void* in, int B, int H, int W, float thr, const int32_t* boxes, uint8_t* mask,
              int32_t* area, float* logits) {
    h->lastB = B;
    int rc;
    pick_chain_form(h, B, H, W);
    const bool ff = can_fuse_first(h, kind, B, H, W);
    const bool fuse = can_fuse_head(h);
    if (ff) {
        if ((rc = enqueue_first_fused(h, (const uint8_t*)in, B, H, W))) return rc;
    } else if ((rc = enqueue_first(h, kind, in, B, H, W))) {
        return rc;
    }
    // One short chain at a time (the per-frame call; one-frame chains on one lane): the host enqueues a launch in ~4 us and a kernel
    // runs ~13 us, so plain launches keep the GPU fed and a graph launch only adds its own latency (measured: 299.7 vs 305.5 us per
    // one-frame chain, unet_segment_frame 0.331 vs 0.342 ms).  Several lanes in flight need the graph: one host thread feeds them all.
    const bool eager = g_plan || !h->use_graphs || (h->active_lanes <= 1 && B <= 4);   // (a dry run captures nothing)
    if (eager) {
        if ((rc = enqueue_body(h, B, fuse, ff))) return rc;
    } else {
        GraphKey key;
        memset(&key, 0, sizeof(key));
        key.B = B;
        key.H = H;
        key.W = W;
        key.flags = (fuse ? 1 : 0) | (ff ? 2 : 0) | (h->precision ? 4 : 0) | (h->wino_chain ? 8 : 0) | (h->active_lanes > 1 ? 16 : 0) |
                    (h->precision == 2 ? 32 : 0);
        key.capB = h->capB;
        auto it = h->graphs.find(key);
        if (it == h->graphs.end()) {
            hipGraph_t g = nullptr;
            HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
            rc = enqueue_body(h, B, fuse, ff);
            hipError_t e = hipStreamEndCapture(h->stream, &g);
            if (rc) {
                if (g) (void)hipGraphDestroy(g);
                return rc;
            }
            if (e != hipSuccess) return fail(OG_EHIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
            hipGraphExec_t ge = nullptr;
            e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (e != hipSuccess) return fail(OG_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
            it = h->graphs.emplace(key, ge).first;
        }
        HIPCHK(hipGraphLaunch(it->second, h->stream));
    }
    if (fuse) return enqueue_last_with_head(h, B, thr, boxes, mask, area, logits);
    return enqueue_head(h, B, H, W, thr, boxes, mask, area, logits);
}

// Split precision only: did any activation leave the f16 range since the last check?  Call after the work has completed.
int check_range(og_unet* h) {
    if (h->h_range && *(volatile int*)h->h_range) {
        *(volatile int*)h->h_range = 0;
        return fail(OG_ERANGE, std::string(h->precision == 2 ? "f16 mode" : "split precision") +
                                   ": an activation exceeded the f16 range (|v| > 60000); the result of this call is not "
                                   "valid -- use og_unet_set_option(h, \"precision\", 0) for these weights");
    }
    return OG_OK;
}

int check_shape(og_unet* h, int B, int H, int W) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (!h->finalized) return fail(OG_ESTATE, "og_unet_finalize() has not been called");
    if (B < 0 || H <= 0 || W <= 0) return fail(OG_EINVAL, "bad B/H/W");
    const int m = 1 << h->L;
    if (H % m || W % m)
        return fail(OG_EINVAL, "H and W must be multiples of 2^n_levels (bilinear fallback of unet.py:84-85 is not implemented)");
    return OG_OK;
}

int ensure_stage(og_unet* h, size_t bytes) {
    if (bytes <= h->stage_bytes) return OG_OK;
    if (h->stage) {
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipFree(h->stage));
        h->stage = nullptr;
        h->stage_bytes = 0;
        drop_graphs(h);
    }
    HIPCHK(hipMalloc(&h->stage, bytes));
    h->stage_bytes = bytes;
    return OG_OK;
}

// Frames per kernel chain actually used: the caller's chunk, capped so that no launch of the chain exceeds grid.z = 65535
// (k_conv_mfma_o: grid.z = frame groups x column tiles [x K parts]; the widest layer decides) -- the cap is applied here
// instead of failing the launch.
int effective_chunk(const og_unet* h) {
    int max_nt = 1;
    auto upd = [&](const ConvLayer& L) {
        if (!L.d_w) return;
        const int nt = (L.mode == 0) ? L.Cout_p / (32 * L.NT) : 4 * L.Cout_p / 64;
        if (nt > max_nt) max_nt = nt;
    };
    for (auto* v : {&h->enc_a, &h->enc_b, &h->up_t, &h->dec_a, &h->dec_b})
        for (auto& l : *v) upd(l);
    upd(h->bott_a);
    upd(h->bott_b);
    int cap = (65535 / max_nt) & ~7;   // whole frame groups of up to 8
    if (cap < 1) cap = 1;
    return h->chunk < cap ? h->chunk : cap;
}

void free_ring(og_unet* h) {
    auto& r = h->ring;
    if (r.s_h2d) (void)hipStreamSynchronize(r.s_h2d);
    if (r.s_d2h) (void)hipStreamSynchronize(r.s_d2h);
    for (auto& s : r.slots) {
        for (void* p : {(void*)s.d_in, (void*)s.d_gray, (void*)s.d_mask, (void*)s.d_area, (void*)s.d_boxes, (void*)s.d_logits, (void*)s.d_net})
            if (p) (void)hipFree(p);
        for (void* p : {(void*)s.h_in, (void*)s.h_mask, (void*)s.h_area, (void*)s.h_boxes, (void*)s.h_logits})
            if (p) (void)hipHostFree(p);
        for (hipEvent_t e : {s.ev_h2d, s.ev_done, s.ev_out})
            if (e) (void)hipEventDestroy(e);
    }
    r.slots.clear();
    r.cap = 0;
    if (r.s_h2d) (void)hipStreamDestroy(r.s_h2d);
    if (r.s_d2h) (void)hipStreamDestroy(r.s_d2h);
    r.s_h2d = r.s_d2h = nullptr;
}

int ensure_ring(og_unet* h, int n_slots, int cap, int H, int W, int ch, bool mask, bool logits, int Hn = 0, int Wn = 0) {
    auto& r = h->ring;
    if ((int)r.slots.size() >= n_slots && r.cap >= cap && r.H == H && r.W == W && r.Hn == Hn && r.Wn == Wn && r.ch >= ch &&
        (r.mask || !mask) && (r.logits || !logits))
        return OG_OK;
    const bool same = r.H == H && r.W == W && r.Hn == Hn && r.Wn == Wn;
    const bool km = r.mask || mask, kl = r.logits || logits;   // keep what an earlier call needed
    const int kch = r.ch > ch ? r.ch : ch, kcap = (same && r.cap > cap) ? r.cap : cap;
    const int ks = (int)r.slots.size() > n_slots ? (int)r.slots.size() : n_slots;
    for (og_unet* t = h; t; t = t->twin)
        if (t->stream) HIPCHK(hipStreamSynchronize(t->stream));
    free_ring(h);
    HIPCHK(hipStreamCreateWithFlags(&r.s_h2d, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&r.s_d2h, hipStreamNonBlocking));
    const size_t HW = (size_t)H * W;
    r.slots.resize(ks);
    for (auto& s : r.slots) {
        HIPCHK(hipMalloc((void**)&s.d_in, kcap * HW * kch));
        HIPCHK(hipHostMalloc((void**)&s.h_in, kcap * HW * kch, hipHostMallocDefault));
        if (Hn) {   // resized: gray and logits at network size, inputs and masks at source size
            HIPCHK(hipMalloc((void**)&s.d_gray, kcap * (size_t)Hn * Wn));
            HIPCHK(hipMalloc((void**)&s.d_net, kcap * (size_t)Hn * Wn * 4));
        } else if (kch == 3) {
            HIPCHK(hipMalloc((void**)&s.d_gray, kcap * HW));
        }
        HIPCHK(hipMalloc((void**)&s.d_area, (size_t)kcap * 4));
        HIPCHK(hipHostMalloc((void**)&s.h_area, (size_t)kcap * 4, hipHostMallocDefault));
        HIPCHK(hipMalloc((void**)&s.d_boxes, (size_t)kcap * 16));
        HIPCHK(hipHostMalloc((void**)&s.h_boxes, (size_t)kcap * 16, hipHostMallocDefault));
        if (km) {
            HIPCHK(hipMalloc((void**)&s.d_mask, kcap * HW));
            HIPCHK(hipHostMalloc((void**)&s.h_mask, kcap * HW, hipHostMallocDefault));
        }
        if (kl) {
            HIPCHK(hipMalloc((void**)&s.d_logits, kcap * HW * 4));
            HIPCHK(hipHostMalloc((void**)&s.h_logits, kcap * HW * 4, hipHostMallocDefault));
        }
        HIPCHK(hipEventCreateWithFlags(&s.ev_h2d, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&s.ev_out, hipEventDisableTiming));
    }
    r.cap = kcap;
    r.H = H;
    r.W = W;
    r.ch = kch;
    r.Hn = Hn;
    r.Wn = Wn;
    r.mask = km;
    r.logits = kl;
    return OG_OK;
}

bool is_pinned_host(const void* p) {   // hipHostMalloc'd / hipHostRegister'ed (e.g. torch's pin_memory): DMA straight from it
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();   // plain pageable memory is "invalid value" to the runtime: not an error here
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

inline size_t al256(size_t x) { return (x + 255) / 256 * 256; }

// ---- frames of any size (og_unet_stream_resized_u8 / og_unet_segment_resized_u8_dev) ----
// Bytes of SOURCE frames per micro-batch of a resized call: a ring slot holds cb x H x W x C input bytes (pinned and device) and
// cb x H x W mask bytes, so large frames lower the frames per micro-batch instead of growing the ring (1080 x 1920 BGR: 10
// frames).  A frame is never split: a single frame above the cap is a micro-batch of one (at most 8192^2 x 3 = 192 MiB).
constexpr size_t kResizeSlotBytes = 64u << 20;
constexpr int kResizeMaxSide = 8192;   // largest source (and network) side a resized call accepts

int check_resized(og_unet* h, int B, int H, int W, int ch, int Hn, int Wn) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (!h->finalized) return fail(OG_ESTATE, "og_unet_finalize() has not been called");
    if (B < 0 || H <= 0 || W <= 0) return fail(OG_EINVAL, "bad B/H/W");
    if (Hn <= 0 || Wn <= 0) return fail(OG_EINVAL, "net_h and net_w must be positive");
    if (H > kResizeMaxSide || W > kResizeMaxSide || Hn > kResizeMaxSide || Wn > kResizeMaxSide)
        return fail(OG_EINVAL, "frame or network side above " + std::to_string(kResizeMaxSide));
    if (ch != 1 && ch != 3) return fail(OG_EINVAL, "channels must be 1 (gray) or 3 (BGR)");
    return check_shape(h, B, Hn, Wn);   // the network size must be a multiple of 2^n_levels
}

// frames per micro-batch of a resized call: the handle's chunk, lowered to the byte cap of a slot's source frames
int resized_chunk(const og_unet* h, int H, int W, int ch) {
    const int chunk = effective_chunk(h);
    const long long per = (long long)H * W * ch, fit = (long long)(kResizeSlotBytes / (size_t)per);
    return fit < 1 ? 1 : (fit < chunk ? (int)fit : chunk);
}

// source u8 [nb,H,W,ch] -> gray u8 [nb,Hn,Wn] (the input k_conv_first<u8> reads)
int enqueue_resize_in(hipStream_t st, int ch, const uint8_t* src, int nb, int H, int W, int Hn, int Wn, uint8_t* gray) {
    const dim3 grid((unsigned)((Hn * Wn + 255) / 256), (unsigned)nb);
    if (ch == 3)
        OG_LAUNCH(k_resize_in<3>, grid, dim3(256), 0, st, src, H, W, Hn, Wn, gray);
    else
        OG_LAUNCH(k_resize_in<1>, grid, dim3(256), 0, st, src, H, W, Hn, Wn, gray);
    return OG_OK;
}

// net logits f32 [nb,Hn,Wn] -> mask / area (inside boxes) / net_prob / prob at source size; area must be zero on entry
int enqueue_resize_out(hipStream_t st, const float* logits, int nb, int Hn, int Wn, int H, int W, float thr, const int32_t* boxes,
                       uint8_t* mask, int32_t* area, float* net_prob, float* prob) {
    const int n = H * W > Hn * Wn ? H * W : Hn * Wn;
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)nb);
    OG_LAUNCH(k_resize_out, grid, dim3(256), 0, st, logits, Hn, Wn, H, W, thr, boxes, mask, area, net_prob, prob);
    if (g_plan) {   // extents from the launch's own geometry: grid.y frames from each pointer
        plan_write("mask", mask, (long long)grid.y * H * W);
        plan_write("area", area, (long long)grid.y * 4);
        plan_write("net_prob", net_prob, (long long)grid.y * Hn * Wn * 4);
        plan_write("prob", prob, (long long)grid.y * H * W * 4);
    }
    return OG_OK;
}

// og_unet_segment_resized_u8_dev after its argument checks, on the handle's own lane (also walked by og_unet_plan_resized, where
// `scratch` is a placeholder).  scratch: cb x Hn x Wn gray bytes (al256), then cb x Hn x Wn f32 logits when net_logits is null.
int resized_dev_run(og_unet* h, const uint8_t* src, int B, int H, int W, int ch, int Hn, int Wn, float thr, const int32_t* boxes,
                    uint8_t* mask, int32_t* area, float* net_logits, float* net_prob, float* prob, int chunk, char* scratch) {
    const bool ident = H == Hn && W == Wn;   // the existing chain, head included: its bits (k_resize_in is then a copy / BGR2GRAY)
    const size_t HW = (size_t)H * W, HWn = (size_t)Hn * Wn;
    uint8_t* s_gray = (uint8_t*)scratch;
    float* s_logits = (float*)(scratch + al256((size_t)chunk * HWn));
    int rc = OG_OK;
    for (int b0 = 0; b0 < B && !rc; b0 += chunk) {
        const int nb = (B - b0 < chunk) ? B - b0 : chunk;
        const uint8_t* in = src + (size_t)b0 * HW * ch;
        const uint8_t* gray = in;
        if (!(ident && ch == 1)) {
            if ((rc = enqueue_resize_in(h->stream, ch, in, nb, H, W, Hn, Wn, s_gray))) break;
            gray = s_gray;
        }
        float* lg = net_logits ? net_logits + (size_t)b0 * HWn : s_logits;
        const int32_t* bx = boxes ? boxes + 4 * (size_t)b0 : nullptr;
        uint8_t* mk = mask ? mask + (size_t)b0 * HW : nullptr;
        int32_t* ar = area ? area + b0 : nullptr;
        float* np_ = net_prob ? net_prob + (size_t)b0 * HWn : nullptr;
        float* pr = prob ? prob + (size_t)b0 * HW : nullptr;
        if ((rc = ident ? run_chunk(h, KIND_U8, gray, nb, Hn, Wn, thr, bx, mk, ar, lg)
                        : run_chunk(h, KIND_U8, gray, nb, Hn, Wn, thr, nullptr, nullptr, nullptr, lg)))
            break;
        if (g_plan && ident) {   // the chain's head writes the caller's outputs of these nb frames
            plan_write("mask", mk, (long long)nb * HW);
            plan_write("area", ar, (long long)nb * 4);
        }
        if (g_plan) plan_write("net_logits", net_logits ? lg : nullptr, (long long)nb * HWn * 4);
        if (!ident) rc = enqueue_resize_out(h->stream, lg, nb, Hn, Wn, H, W, thr, bx, mk, ar, np_, pr);
        else if (np_ || pr) rc = enqueue_resize_out(h->stream, lg, nb, Hn, Wn, H, W, thr, nullptr, nullptr, nullptr, np_, pr);
    }
    return rc;
}

}  // namespace

#if !defined(__HIP_DEVICE_COMPILE__)
// k_bgr2gray's arithmetic on the host: OpenCV's published u8 path (15-bit fixed point); an AVX2 clone is picked at load time
__attribute__((target_clones("avx2", "default")))
#endif
static void bgr2gray_host_loop(const uint8_t* __restrict__ bgr, long long n, uint8_t* __restrict__ gray) {
    for (long long i = 0; i < n; ++i)
        gray[i] = (uint8_t)((bgr[3 * i] * 3735 + bgr[3 * i + 1] * 19235 + bgr[3 * i + 2] * 9798 + (1 << 14)) >> 15);
}

#include "og_stream.inc"
#include "og_yolo.inc"
#include "og_crops.inc"
#include "og_classic.inc"
#include "og_gated.inc"
#include "og_gate.inc"
#include "og_overlay.inc"
#include "og_sweep.inc"
#include "og_mjpeg.inc"
#include "og_mjpd.inc"
#include "og_mjps.inc"
#include "og_png.inc"
#include "og_pnge.inc"
#include "og_aug.inc"

extern "C" {

const char* og_last_error(void) { return g_err.c_str(); }
// The string names the build's answer to the GFX9 store-data hazard (og_buffer_store16, profiles/r02_epilogue_fence_audit.md):
// the Python loader refuses a library that does not say "store_nop=1" (an audit build with -DOG_STORE_NOP=0 computes wrong lanes).
#define OG_STR2(x) #x
#define OG_STR(x) OG_STR2(x)
const char* og_version(void) { return "openglottal_hip 0.3 (gfx950; store_nop=" OG_STR(OG_STORE_NOP) ")"; }

int og_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(OG_ENODEV, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    return n;
}

int og_init(int device) {
    int n = og_device_count();
    if (n <= 0) return fail(OG_ENODEV, "no HIP device visible");
    if (device < 0 || device >= n) return fail(OG_EINVAL, "device ordinal out of range");
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(OG_ENODEV, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    return OG_OK;
}

void* og_malloc(size_t bytes) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e != hipSuccess) {
        fail(OG_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
        return nullptr;
    }
    return p;
}
int og_free(void* d) {
    if (d) HIPCHK(hipFree(d));
    return OG_OK;
}
int og_memcpy_h2d(void* dst, const void* src, size_t bytes) {
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return OG_OK;
}
int og_memcpy_d2h(void* dst, const void* src, size_t bytes) {
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return OG_OK;
}

og_unet* og_unet_create(const int* features, int n_levels, int in_ch, int out_ch) {
    if (!features || n_levels < 1 || n_levels > 6) {
        fail(OG_EINVAL, "features/n_levels invalid (1..6 levels)");
        return nullptr;
    }
    if (in_ch != 1 || out_ch != 1) {
        fail(OG_EINVAL, "only in_ch=1, out_ch=1 is implemented (the configuration every reference pipeline constructs)");
        return nullptr;
    }
    for (int i = 0; i < n_levels; ++i)
        if (features[i] < 1 || features[i] > 4096) {
            fail(OG_EINVAL, "feature width out of range");
            return nullptr;
        }
    for (int i = 1; i < n_levels; ++i)
        if (features[i] != 2 * features[i - 1]) {
            // ups[2j] = ConvTranspose2d(f*2, f) consumes the previous level's f*2-channel output
            // (unet.py:68-70,82): the reference's forward only type-checks when widths double.
            fail(OG_EINVAL, "features must double per level (reference forward requires features[i+1] == 2*features[i])");
            return nullptr;
        }
    og_unet* h = new og_unet();
    h->features.assign(features, features + n_levels);
    h->L = n_levels;
    int ch = 1;
    for (int i = 0; i < n_levels; ++i) {
        expect_double_conv(h, "downs." + std::to_string(i), ch, features[i]);
        ch = features[i];
    }
    expect_double_conv(h, "bottleneck", ch, 2 * ch);
    for (int j = 0; j < n_levels; ++j) {
        const int f = features[n_levels - 1 - j];
        expect(h, "ups." + std::to_string(2 * j) + ".weight", {2 * f, f, 2, 2});
        expect(h, "ups." + std::to_string(2 * j) + ".bias", {f});
        expect_double_conv(h, "ups." + std::to_string(2 * j + 1), 2 * f, f);
    }
    expect(h, "head.weight", {1, features[0], 1, 1});
    expect(h, "head.bias", {1});
    return h;
}

void og_unet_destroy(og_unet* h) {
    if (!h) return;
    DeviceGuard dg_(h->device, og_skip_device(h));   // frees and stream teardown on the handle's device, the caller's restored
    if (h->twin) {
        og_unet_destroy(h->twin);
        h->twin = nullptr;
    }
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    drop_graphs(h);
    if (h->host_only) {   // placeholders only: nothing to release on any device
        delete h;
        return;
    }
    if (!h->is_twin) {  // a twin borrows every weight pointer from its owner
        for (auto* v : {&h->enc_a, &h->enc_b, &h->up_t, &h->dec_a, &h->dec_b})
            for (auto& l : *v) free_layer(l);
        free_layer(h->bott_a);
        free_layer(h->bott_b);
        for (float* p : {h->d_first_w, h->d_first_scale, h->d_first_shift, h->d_head_w, h->d_zero})
            if (p) (void)hipFree(p);
        if (h->h_range) (void)hipHostFree(h->h_range);
    }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    if (h->arena) (void)hipFree(h->arena);
    if (h->stage) (void)hipFree(h->stage);
    free_ring(h);
    if (h->d_stamps) (void)hipFree(h->d_stamps);
    if (h->d_partial) (void)hipFree(h->d_partial);
    if (h->d_tile_counter) (void)hipFree(h->d_tile_counter);
    if (h->d_counts) (void)hipFree(h->d_counts);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int og_unet_set_tensor(og_unet* h, const char* key, const void* host, const int64_t* shape, int ndim, int dtype) {
    if (!h || !key || !host) return fail(OG_EINVAL, "null argument");
    if (h->finalized) return fail(OG_ESTATE, "handle already finalized");
    const std::string k(key);
    const std::string nbt = ".num_batches_tracked";
    if (k.size() > nbt.size() && k.compare(k.size() - nbt.size(), nbt.size(), nbt) == 0) {
        const std::string bnw = k.substr(0, k.size() - nbt.size()) + ".weight";
        if (!h->expected.count(bnw)) return fail(OG_EINVAL, "unexpected key " + k);
        return OG_OK;  // accepted and ignored (eval-mode BN does not use it)
    }
    auto it = h->expected.find(k);
    if (it == h->expected.end()) return fail(OG_EINVAL, "unexpected key " + k);
    if (dtype != OG_DTYPE_F32) return fail(OG_EINVAL, "tensor " + k + " must be float32");
    if (ndim < 0 || (ndim > 0 && !shape)) return fail(OG_EINVAL, "bad shape for " + k);
    std::vector<int64_t> s(shape, shape + ndim);
    if (s != it->second) {
        std::string m = "size mismatch for " + k + ": expected [";
        for (auto v : it->second) m += std::to_string(v) + ",";
        m += "] got [";
        for (auto v : s) m += std::to_string(v) + ",";
        return fail(OG_EINVAL, m + "]");
    }
    size_t n = 1;
    for (auto v : s) n *= (size_t)v;
    HostTensor t;
    t.shape = s;
    t.data.assign((const float*)host, (const float*)host + n);
    h->host[k] = std::move(t);
    return OG_OK;
}

int og_unet_finalize(og_unet* h) {
    if (!h) return fail(OG_EINVAL, "null handle");
    if (h->finalized) return OG_OK;
    std::string missing;
    for (auto& kv : h->expected)
        if (!h->host.count(kv.first)) missing += (missing.empty() ? "" : ", ") + kv.first;
    if (!missing.empty() && !h->host_only) return fail(OG_EINVAL, "missing key(s) in state_dict: " + missing);

    const int L = h->L;
    int rc;
    if (!h->host_only) {
        int dev = 0;
        hipDeviceProp_t prop;
        HIPCHK(hipGetDevice(&dev));
        HIPCHK(hipGetDeviceProperties(&prop, dev));
        h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        h->device = dev;
        HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreate(&h->ev0));
        HIPCHK(hipEventCreate(&h->ev1));
        HIPCHK(hipMalloc((void**)&h->d_zero, 4096));
        HIPCHK(hipMemset(h->d_zero, 0, 4096));
        HIPCHK(hipMalloc((void**)&h->d_partial, kPartialBytes));
        HIPCHK(hipMalloc((void**)&h->d_tile_counter, kTileCounters * sizeof(int)));
        HIPCHK(hipMemset(h->d_tile_counter, 0, kTileCounters * sizeof(int)));
        HIPCHK(hipHostMalloc((void**)&h->h_range, sizeof(int), hipHostMallocMapped));
        *h->h_range = 0;
        HIPCHK(hipHostGetDevicePointer((void**)&h->d_range, h->h_range, 0));
        if ((rc = init_kernel_attrs())) return rc;
    } else {   // og_unet_plan: an MI355X's CU count, placeholder pointers
        h->n_cu = 256;
        h->d_zero = (float*)8;
        h->d_partial = (float*)8;
        h->d_tile_counter = (int*)8;
        h->d_first_w = h->d_first_scale = h->d_first_shift = h->d_head_w = (float*)8;
    }
    if (!h->host_only) {  // first layer: [Cout][1][3][3] -> [9][Cp0]
        const int f0 = h->features[0], Cp0 = cp32(f0);
        const auto& w = h->host.at("downs.0.net.0.weight").data;
        std::vector<float> w9((size_t)9 * Cp0, 0.f), sc, sh;
        for (int co = 0; co < f0; ++co)
            for (int t = 0; t < 9; ++t) w9[(size_t)t * Cp0 + co] = w[(size_t)co * 9 + t];
        fold_bn(h, "downs.0.net.1", f0, Cp0, sc, sh);
        if ((rc = upload(w9, &h->d_first_w))) return rc;
        if ((rc = upload(sc, &h->d_first_scale))) return rc;
        if ((rc = upload(sh, &h->d_first_shift))) return rc;
    }
    h->enc_a.resize(L);
    h->enc_b.resize(L);
    int ch = 1;
    for (int i = 0; i < L; ++i) {
        const std::string p = "downs." + std::to_string(i);
        const int f = h->features[i];
        if (i > 0 && (rc = build_conv(h, h->enc_a[i], p + ".net.0.weight", p + ".net.1", ch, f, ident_map(ch)))) return rc;
        if ((rc = build_conv(h, h->enc_b[i], p + ".net.3.weight", p + ".net.4", f, f, ident_map(f)))) return rc;
        ch = f;
    }
    if ((rc = build_conv(h, h->bott_a, "bottleneck.net.0.weight", "bottleneck.net.1", ch, 2 * ch, ident_map(ch)))) return rc;
    if ((rc = build_conv(h, h->bott_b, "bottleneck.net.3.weight", "bottleneck.net.4", 2 * ch, 2 * ch, ident_map(2 * ch)))) return rc;
    h->up_t.resize(L);
    h->dec_a.resize(L);
    h->dec_b.resize(L);
    for (int j = 0; j < L; ++j) {
        const int f = h->features[L - 1 - j];
        const int Cp = cp32(f);
        const std::string pt = "ups." + std::to_string(2 * j), pd = "ups." + std::to_string(2 * j + 1);
        if ((rc = build_convT(h, h->up_t[j], pt, 2 * f, f))) return rc;
        // cat([skip, up]) (unet.py:86): original ci<f is the skip, ci>=f the up-sampled half
        std::vector<int> m(2 * Cp, -1);
        for (int c = 0; c < f; ++c) {
            m[c] = c;
            m[Cp + c] = f + c;
        }
        if ((rc = build_conv(h, h->dec_a[j], pd + ".net.0.weight", pd + ".net.1", 2 * f, f, m))) return rc;
        if ((rc = build_conv(h, h->dec_b[j], pd + ".net.3.weight", pd + ".net.4", f, f, ident_map(f)))) return rc;
    }
    if (!h->host_only) {
        const int f0 = h->features[0], Cp0 = cp32(f0);
        std::vector<float> hw(Cp0, 0.f);
        const auto& w = h->host.at("head.weight").data;
        for (int c = 0; c < f0; ++c) hw[c] = w[c];
        if ((rc = upload(hw, &h->d_head_w))) return rc;
        h->head_bias = h->host.at("head.bias").data[0];
    }
    h->host.clear();
    h->finalized = true;
    // extra lanes: same weights (pointers shared), own stream / events / split-K workspace; arena on demand.
    // h -> twin -> twin's twin: micro-batch k of a call runs on lane k % n_lanes.
    og_unet* prev = h;
    for (int lane = 1; lane < kMaxLanes; ++lane) {
        og_unet* t = new og_unet();
        t->is_twin = true;
        t->features = h->features;
        t->L = h->L;
        t->finalized = true;
        t->d_first_w = h->d_first_w;
        t->d_first_scale = h->d_first_scale;
        t->d_first_shift = h->d_first_shift;
        t->enc_a = h->enc_a;
        t->enc_b = h->enc_b;
        t->bott_a = h->bott_a;
        t->bott_b = h->bott_b;
        t->up_t = h->up_t;
        t->dec_a = h->dec_a;
        t->dec_b = h->dec_b;
        t->d_head_w = h->d_head_w;
        t->head_bias = h->head_bias;
        t->d_zero = h->d_zero;
        t->h_range = h->h_range;
        t->d_range = h->d_range;
        t->n_cu = h->n_cu;
        t->device = h->device;
        prev->twin = t;
        prev = t;
        if (h->host_only) {
            t->host_only = true;
            t->d_partial = (float*)8;
            t->d_tile_counter = (int*)8;
            continue;
        }
        HIPCHK(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreate(&t->ev0));
        HIPCHK(hipEventCreate(&t->ev1));
        HIPCHK(hipMalloc((void**)&t->d_partial, kPartialBytes));
        HIPCHK(hipMalloc((void**)&t->d_tile_counter, kTileCounters * sizeof(int)));
        HIPCHK(hipMemset(t->d_tile_counter, 0, kTileCounters * sizeof(int)));
        HIPCHK(hipEventCreateWithFlags(&t->ev_join, hipEventDisableTiming));
    }
    if (h->host_only) return OG_OK;
    HIPCHK(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    return OG_OK;
}

int og_unet_reserve(og_unet* h, int frames_per_launch, int H, int W) {
    OG_SCOPE(h);
    int rc = check_shape(h, frames_per_launch, H, W);
    if (rc) return rc;
    if (frames_per_launch < 1) return fail(OG_EINVAL, "frames_per_launch must be >= 1");
    for (og_unet* t = h; t; t = t->twin)
        if ((rc = ensure_arena(t, frames_per_launch, H, W))) return rc;
    return OG_OK;
}

int og_unet_set_chunk(og_unet* h, int n) {
    if (!h || n < 1 || n > 4096) return fail(OG_EINVAL, "chunk must be in 1..4096");
    h->chunk = n;
    for (og_unet* t = h->twin; t; t = t->twin) t->chunk = n;
    return OG_OK;
}

int og_unet_set_graphs(og_unet* h, int enable) {
    if (!h) return fail(OG_EINVAL, "null handle");
    h->use_graphs = enable ? 1 : 0;
    for (og_unet* t = h->twin; t; t = t->twin) t->use_graphs = h->use_graphs;
    return OG_OK;
}

int og_unet_set_option(og_unet* h, const char* name, int value) {
    if (!h || !name) return fail(OG_EINVAL, "null argument");
    OG_SCOPE(h);
    const std::string n(name);
    int* slot = nullptr;
    if (n == "conv_impl" && value >= 0 && value <= 3) slot = &h->conv_impl;
    else if (n == "tps_nt1" && (value == 1 || value == 3 || value == 9)) slot = &h->tps_nt1;
    else if (n == "tps_nt2" && (value == 1 || value == 3)) slot = &h->tps_nt2;
    else if (n == "xcd_group" && (value == 0 || value == 1)) slot = &h->xcd_group;
    else if (n == "splitk_occ" && (value == 0 || value == 1)) slot = &h->splitk_occ;
    else if (n == "splitk_nt1" && (value == 0 || value == 1)) slot = &h->splitk_nt1;
    else if (n == "wino" && (value == 0 || value == 1)) slot = &h->wino;
    else if (n == "wino_first" && (value == 0 || value == 1)) slot = &h->wino_first;
    else if (n == "wino_ps" && value >= 0 && value <= 4) slot = &h->wino_ps;
    else if (n == "zero_copy" && (value == 0 || value == 1)) slot = &h->zero_copy;
    else if (n == "wino_w" && value >= 0 && value <= 4) slot = &h->wino_w;
    else if (n == "inject_fault" && value >= 0 && value <= 1000) slot = &h->inject_fault;
    else if (n == "splitk_fused" && (value == 0 || value == 1)) slot = &h->splitk_fused;
    else if (n == "splitk_slots" && value >= 1 && value <= 4) slot = &h->splitk_slots;
    else if (n == "splitk_min_steps" && value >= 1 && value <= 9) slot = &h->splitk_min_steps;
    else if (n == "splitk_div" && value >= 1 && value <= 8) slot = &h->splitk_div;
    else if (n == "occ_min_pct" && value >= 0 && value <= 400) slot = &h->occ_min_pct;
    else if (n == "wg_per_cu" && value >= 1 && value <= 2) slot = &h->wg_per_cu;
    else if (n == "prio_mode" && value >= 0 && value <= 3) slot = &h->prio_mode;
    else if (n == "splitk" && (value == 0 || value == 1)) slot = &h->splitk;
    else if (n == "tile_h" && (value == 0 || value == 8 || value == 16)) slot = &h->tile_h;
    else if (n == "convt_occ" && (value == 0 || value == 1)) slot = &h->convt_occ;
    else if (n == "convt_w" && (value == 0 || value == 1)) slot = &h->convt_w;
    else if (n == "fuse_head" && (value == 0 || value == 1)) slot = &h->fuse_head;
    else if (n == "fuse_first" && (value == 0 || value == 1)) slot = &h->fuse_first;
    else if (n == "keep_taps" && (value == 0 || value == 1)) slot = &h->keep_taps;
    else if (n == "entry_f32" && (value == 0 || value == 1)) slot = &h->entry_f32;
    else if (n == "dual" && (value == 0 || value == 1)) slot = &h->dual;
    else if (n == "lanes" && value >= 0 && value <= kMaxLanes) slot = &h->n_lanes;
    else if (n == "stream" && (value == 0 || value == 1)) slot = &h->stream_host;
    else if (n == "precision" && value >= 0 && value <= 2) slot = &h->precision;
    else if (n == "h_square" && (value == 0 || value == 1)) slot = &h->h_square;
    if (!slot) return fail(OG_EINVAL, "unknown option or bad value: " + n);
    if ((slot == &h->precision && value == 2 && h->splitk) || (slot == &h->splitk && value == 1 && h->precision == 2))
        return fail(OG_EINVAL, "f16 mode (precision 2) never splits K: \"splitk\" 1 and \"precision\" 2 exclude each other");
    if (*slot != value) {
        if (h->stream) HIPCHK(hipStreamSynchronize(h->stream));
        drop_graphs(h);
        if (slot == &h->precision && (value == 2 || *slot == 2)) h->aH = h->aW = 0;   // other bytes per channel: the next call re-plans the arena
        *slot = value;
    }
    if (h->twin && n != "inject_fault") return og_unet_set_option(h->twin, name, value);   // (the test hook arms the first lane only)
    return OG_OK;
}

int og_unet_sync(og_unet* h) {
    if (!h || !h->stream) return fail(OG_ESTATE, "handle not finalized");
    OG_SCOPE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    return check_range(h);
}

void* og_unet_stream(og_unet* h) { return h ? (void*)h->stream : nullptr; }

int og_timer_start(og_unet* h) {
    if (!h || !h->stream) return fail(OG_ESTATE, "handle not finalized");
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    return OG_OK;
}
int og_timer_stop(og_unet* h, float* ms) {
    if (!h || !h->stream || !ms) return fail(OG_ESTATE, "handle not finalized");
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipEventSynchronize(h->ev1));
    HIPCHK(hipEventElapsedTime(ms, h->ev0, h->ev1));
    return OG_OK;
}

int og_unet_segment_u8_dev(og_unet* h, const uint8_t* gray, int B, int H, int W, float thr, const int32_t* boxes,
                           uint8_t* mask, int32_t* area, float* logits) {
    OG_SCOPE(h);
    int rc = check_shape(h, B, H, W);
    if (rc) return rc;
    OG_ALIGN(boxes);
    OG_ALIGN(area);
    OG_ALIGN(logits);
    if (!gray && B > 0) return fail(OG_EINVAL, "gray is null");
    if (B == 0) return OG_OK;
    const int chunk = effective_chunk(h);
    const int cb = chunk < B ? chunk : B;
    if ((rc = ensure_arena(h, cb, H, W))) return rc;
    if (area) HIPCHK(hipMemsetAsync(area, 0, (size_t)B * sizeof(int32_t), h->stream));
    const size_t HW = (size_t)H * W;
    const int n_chunks = (B + chunk - 1) / chunk;
    og_unet* lanes[kMaxLanes] = {h};
    int n_lanes = 1;
    // more lanes the smaller the micro-batch: at batch 1 a chain is 23 launches of ~15 us that each fill a fraction of the chip
    const int want = h->n_lanes ? h->n_lanes : (chunk <= 16 ? 3 : 2);   // measured: 3 lanes +15 % at 1 frame/launch, +2 % at 16, -1 % at 32
    if (h->dual)
        for (og_unet* t = h->twin; t && n_lanes < want && n_lanes < n_chunks; t = t->twin) lanes[n_lanes++] = t;
    for (int l = 1; l < n_lanes; ++l)   // every allocation BEFORE the fork: nothing below can fail between fork and join except a launch
        if ((rc = ensure_arena(lanes[l], cb, H, W))) return rc;
    for (int l = 0; l < n_lanes; ++l) lanes[l]->active_lanes = n_lanes;
    if (n_lanes > 1) HIPCHK(hipEventRecord(h->ev_fork, h->stream));
    int forked = 1;
    for (int l = 1; l < n_lanes && !rc; ++l) {  // a lane's chain must see everything enqueued so far on this stream (area memset, caller's H2D copies)
        if (hipStreamWaitEvent(lanes[l]->stream, h->ev_fork, 0) != hipSuccess) rc = fail(OG_EHIP, "hipStreamWaitEvent(fork)");
        else forked = l + 1;
    }
    int k = 0;
    for (int b0 = 0; b0 < B && !rc; b0 += chunk, ++k) {
        const int nb = (B - b0 < chunk) ? B - b0 : chunk;
        rc = run_chunk(lanes[k % n_lanes], KIND_U8, gray + b0 * HW, nb, H, W, thr, boxes ? boxes + 4 * b0 : nullptr,
                       mask ? mask + b0 * HW : nullptr, area ? area + b0 : nullptr, logits ? logits + b0 * HW : nullptr);
    }
    // join ALSO on error: whatever the lanes already have in flight still writes the caller's mask / area / logits buffers,
    // so this stream (and with it og_unet_sync / the host variant's copies) must wait for it before the caller may free them
    const std::string err = g_err;
    for (int l = 1; l < forked; ++l) {
        if (hipEventRecord(lanes[l]->ev_join, lanes[l]->stream) != hipSuccess || hipStreamWaitEvent(h->stream, lanes[l]->ev_join, 0) != hipSuccess) {
            (void)hipStreamSynchronize(lanes[l]->stream);   // last resort: block here rather than leave the lane running
            if (!rc) rc = fail(OG_EHIP, "lane join failed");
        }
    }
    if (rc) {
        g_err = err.empty() ? g_err : err;
        for (int l = 0; l < n_lanes; ++l) {
            reset_counters(lanes[l]);
            if (l > 0) (void)hipStreamSynchronize(lanes[l]->stream);
        }
        (void)hipStreamSynchronize(h->stream);   // error path only: nothing of this call is in flight when the error is reported
    }
    return rc;
}

// The frame loop with the video on the HOST (features.py:226,234-245), streamed: see og_unet::Ring.
// Hn > 0 (resized call, frames of H x W != Hn x Wn): per micro-batch the source frames go up into the slot, k_resize_in writes the
// network-size gray frames (it replaces k_bgr2gray), the chain runs at Hn x Wn with its logits in the slot, and k_resize_out writes
// mask and area at source size; the micro-batch is lowered to kResizeSlotBytes of source frames.  Zero copy stays off for these calls
// (the chain does not read the caller's frames: k_resize_in does, and the resize pair is not written for host-mapped buffers).
static int stream_impl(og_unet* h, const uint8_t* frames, const uint8_t* const* frame_ptrs, int B, int H, int W, int ch, float thr,
                       const int32_t* boxes, uint8_t* mask, int32_t* area, float* logits, int Hn = 0, int Wn = 0) {
    OG_SCOPE(h);
    const bool rs = Hn > 0;
    int rc = rs ? check_resized(h, B, H, W, ch, Hn, Wn) : check_shape(h, B, H, W);
    if (rc) return rc;
    if (ch != 1 && ch != 3) return fail(OG_EINVAL, "channels must be 1 (gray) or 3 (BGR)");
    OG_ALIGN(frame_ptrs);
    OG_ALIGN(boxes);
    OG_ALIGN(area);
    OG_ALIGN(logits);
    if (B == 0) return OG_OK;
    if (!frames && !frame_ptrs) return fail(OG_EINVAL, "frames is null");
    if (frame_ptrs)
        for (int i = 0; i < B; ++i)
            if (!frame_ptrs[i]) return fail(OG_EINVAL, "frame_ptrs[" + std::to_string(i) + "] is null");
    if (rs) logits = nullptr;
    const int cH = rs ? Hn : H, cW = rs ? Wn : W;   // the chain's frame size
    const int chunk = rs ? resized_chunk(h, H, W, ch) : effective_chunk(h);
    const int cb = chunk < B ? chunk : B;
    const int n_chunks = (B + chunk - 1) / chunk;
    og_unet* lanes[kMaxLanes] = {h};
    int n_lanes = 1;
    const int want = h->n_lanes ? h->n_lanes : (chunk <= 16 ? 3 : 2);
    if (h->dual)
        for (og_unet* t = h->twin; t && n_lanes < want && n_lanes < n_chunks; t = t->twin) lanes[n_lanes++] = t;
    for (int l = 0; l < n_lanes; ++l)
        if ((rc = ensure_arena(lanes[l], cb, cH, cW))) return rc;
    for (int l = 0; l < n_lanes; ++l) lanes[l]->active_lanes = n_lanes;
    const int n_slots = (n_chunks < n_lanes + 2) ? n_chunks : n_lanes + 2;   // one being filled, one per lane computing, one draining
    if ((rc = ensure_ring(h, n_slots, cb, H, W, ch, mask != nullptr, logits != nullptr, rs ? Hn : 0, rs ? Wn : 0))) return rc;
    auto& R = h->ring;
    const size_t HW = (size_t)H * W, fb = HW * ch;
    const bool pinned = frames != nullptr && is_pinned_host(frames);
    const bool single = n_chunks == 1;

    auto retire = [&](og_unet::Slot& s) -> int {   // wait for the slot's outputs and hand them to the caller
        if (s.b0 < 0) return OG_OK;
        const int b0 = s.b0, nb = s.nb;
        s.b0 = -1;
        HIPCHK(hipEventSynchronize(s.ev_out));
        if (area) memcpy(area + b0, s.h_area, (size_t)nb * 4);
        if (mask) memcpy(mask + b0 * HW, s.h_mask, nb * HW);
        if (logits) memcpy(logits + b0 * HW, s.h_logits, nb * HW * 4);
        return OG_OK;
    };
    auto fill = [&](og_unet::Slot& s, og_unet* lane, int b0, int nb) -> int {
        const uint8_t* src = frames ? frames + (size_t)b0 * fb : nullptr;
        if (frame_ptrs) {   // a list of separately allocated frames: gathered here, one copy per frame, into the pinned slot
            for (int j = 0; j < nb; ++j) memcpy(s.h_in + (size_t)j * fb, frame_ptrs[b0 + j], fb);
            src = s.h_in;
        } else if (!pinned) {   // pageable memory: stage through the slot's pinned buffer so that the DMA is asynchronous
            memcpy(s.h_in, src, nb * fb);
            src = s.h_in;
        }
        // a call that is ONE micro-batch has nothing to overlap: its copies go on the compute stream, in order, and the two
        // cross-stream hand-overs (tens of microseconds each on a one-frame call) disappear
        const hipStream_t s_in = single ? lane->stream : R.s_h2d, s_out = single ? lane->stream : R.s_d2h;
        // The per-frame call (utils.py:235-237: one frame in, one mask out): every copy command costs a launch floor (~5 us) on the
        // one stream there is, more than moving 64 KB costs.  So the kernels read the frame from, and write the mask / area to, the
        // slot's PINNED host buffers directly (mapped into the device's address space; the writes are visible to the host once the
        // completion event has fired): no H2D, no D2H, no memset command.
        bool zc = !rs && single && nb <= 4 && h->zero_copy && !logits && (src == s.h_in || pinned);
        uint8_t* z_in = nullptr;
        uint8_t* z_mask = nullptr;
        int32_t* z_area = nullptr;
        int32_t* z_boxes = nullptr;
        if (zc && hipHostGetDevicePointer((void**)&z_in, (void*)src, 0) != hipSuccess) {
            (void)hipGetLastError();   // a caller-pinned source that is not mapped into the device's address space: the copy path
            zc = false;
        }
        if (boxes) memcpy(s.h_boxes, boxes + 4 * (size_t)b0, (size_t)nb * 16);
        if (zc) {
            if (mask) HIPCHK(hipHostGetDevicePointer((void**)&z_mask, s.h_mask, 0));
            if (area) {
                HIPCHK(hipHostGetDevicePointer((void**)&z_area, s.h_area, 0));
                memset(s.h_area, 0, (size_t)nb * 4);
            }
            if (boxes) HIPCHK(hipHostGetDevicePointer((void**)&z_boxes, s.h_boxes, 0));
        } else {
            HIPCHK(hipMemcpyAsync(s.d_in, src, nb * fb, hipMemcpyHostToDevice, s_in));
            if (boxes) HIPCHK(hipMemcpyAsync(s.d_boxes, s.h_boxes, (size_t)nb * 16, hipMemcpyHostToDevice, s_in));
        }
        if (!single) {
            HIPCHK(hipEventRecord(s.ev_h2d, R.s_h2d));
            HIPCHK(hipStreamWaitEvent(lane->stream, s.ev_h2d, 0));
        }
        const uint8_t* gray = zc ? z_in : s.d_in;
        if (rs) {
            if (area) HIPCHK(hipMemsetAsync(s.d_area, 0, (size_t)nb * 4, lane->stream));
            int rc2 = enqueue_resize_in(lane->stream, ch, s.d_in, nb, H, W, Hn, Wn, s.d_gray);
            if (!rc2) rc2 = run_chunk(lane, KIND_U8, s.d_gray, nb, Hn, Wn, thr, nullptr, nullptr, nullptr, s.d_net);
            if (!rc2) rc2 = enqueue_resize_out(lane->stream, s.d_net, nb, Hn, Wn, H, W, thr, boxes ? s.d_boxes : nullptr,
                                               mask ? s.d_mask : nullptr, area ? s.d_area : nullptr, nullptr, nullptr);
            if (rc2) return rc2;
        } else if (ch == 3) {   // cv2.cvtColor(frm_bgr, COLOR_BGR2GRAY) of features.py:235, on the device, in front of the chain
            const long long n = (long long)nb * H * W;
            hipLaunchKernelGGL(k_bgr2gray, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, lane->stream, gray, s.d_gray, n);
            HIPCHK(hipGetLastError());
            gray = s.d_gray;
        }
        if (!rs) {
            if (area && !zc) HIPCHK(hipMemsetAsync(s.d_area, 0, (size_t)nb * 4, lane->stream));
            int rc2 = zc ? run_chunk(lane, KIND_U8, gray, nb, H, W, thr, z_boxes, z_mask, z_area, nullptr)
                         : run_chunk(lane, KIND_U8, gray, nb, H, W, thr, boxes ? s.d_boxes : nullptr, mask ? s.d_mask : nullptr,
                                     area ? s.d_area : nullptr, logits ? s.d_logits : nullptr);
            if (rc2) return rc2;
        }
        if (zc) {
            HIPCHK(hipEventRecord(s.ev_out, s_out));
            s.b0 = b0;
            s.nb = nb;
            return OG_OK;
        }
        if (!single) {
            HIPCHK(hipEventRecord(s.ev_done, lane->stream));
            HIPCHK(hipStreamWaitEvent(R.s_d2h, s.ev_done, 0));
        }
        if (area) HIPCHK(hipMemcpyAsync(s.h_area, s.d_area, (size_t)nb * 4, hipMemcpyDeviceToHost, s_out));
        if (mask) HIPCHK(hipMemcpyAsync(s.h_mask, s.d_mask, nb * HW, hipMemcpyDeviceToHost, s_out));
        if (logits) HIPCHK(hipMemcpyAsync(s.h_logits, s.d_logits, nb * HW * 4, hipMemcpyDeviceToHost, s_out));
        HIPCHK(hipEventRecord(s.ev_out, s_out));
        s.b0 = b0;
        s.nb = nb;
        return OG_OK;
    };

    int k = 0;
    for (int b0 = 0; b0 < B && !rc; b0 += chunk, ++k) {
        og_unet::Slot& s = R.slots[k % n_slots];
        if ((rc = retire(s))) break;   // frees the slot: its previous micro-batch (k - n_slots) is complete and delivered
        rc = fill(s, lanes[k % n_lanes], b0, (B - b0 < chunk) ? B - b0 : chunk);
    }
    for (int i = 0; i < n_slots; ++i) {   // drain in age order; on error still wait for everything in flight (caller-owned buffers)
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

int og_unet_stream_u8(og_unet* h, const uint8_t* frames, int B, int H, int W, int channels, float thr, const int32_t* boxes,
                      uint8_t* mask, int32_t* area) {
    return stream_impl(h, frames, nullptr, B, H, W, channels, thr, boxes, mask, area, nullptr);
}

int og_unet_stream_frames_u8(og_unet* h, const uint8_t* const* frame_ptrs, int B, int H, int W, int channels, float thr,
                             const int32_t* boxes, uint8_t* mask, int32_t* area) {
    if (!frame_ptrs && B > 0) return fail(OG_EINVAL, "frame_ptrs is null");
    return stream_impl(h, nullptr, frame_ptrs, B, H, W, channels, thr, boxes, mask, area, nullptr);
}

int og_unet_stream_resized_u8(og_unet* h, const uint8_t* frames, int B, int H, int W, int channels, int net_h, int net_w, float thr,
                              const int32_t* boxes, uint8_t* mask, int32_t* area) {
    if (H == net_h && W == net_w && H > 0 && W > 0 && H <= kResizeMaxSide && W <= kResizeMaxSide)   // already at network size
        return stream_impl(h, frames, nullptr, B, H, W, channels, thr, boxes, mask, area, nullptr);
    return stream_impl(h, frames, nullptr, B, H, W, channels, thr, boxes, mask, area, nullptr, net_h, net_w);
}

int og_unet_stream_frames_resized_u8(og_unet* h, const uint8_t* const* frame_ptrs, int B, int H, int W, int channels, int net_h,
                                     int net_w, float thr, const int32_t* boxes, uint8_t* mask, int32_t* area) {
    if (!frame_ptrs && B > 0) return fail(OG_EINVAL, "frame_ptrs is null");
    if (H == net_h && W == net_w && H > 0 && W > 0 && H <= kResizeMaxSide && W <= kResizeMaxSide)
        return stream_impl(h, nullptr, frame_ptrs, B, H, W, channels, thr, boxes, mask, area, nullptr);
    return stream_impl(h, nullptr, frame_ptrs, B, H, W, channels, thr, boxes, mask, area, nullptr, net_h, net_w);
}

int og_unet_segment_resized_u8_dev(og_unet* h, const uint8_t* src, int B, int H, int W, int channels, int net_h, int net_w, float thr,
                                   const int32_t* boxes, uint8_t* mask, int32_t* area, float* net_logits, float* net_prob, float* prob) {
    OG_SCOPE(h);
    int rc = check_resized(h, B, H, W, channels, net_h, net_w);
    if (rc) return rc;
    OG_ALIGN(boxes);
    OG_ALIGN(area);
    OG_ALIGN(net_logits);
    OG_ALIGN(net_prob);
    OG_ALIGN(prob);
    if (!src && B > 0) return fail(OG_EINVAL, "src is null");
    if (B == 0) return OG_OK;
    const int chunk = resized_chunk(h, H, W, channels), cb = chunk < B ? chunk : B;
    const size_t HWn = (size_t)net_h * net_w;
    if ((rc = ensure_arena(h, cb, net_h, net_w))) return rc;
    if ((rc = ensure_stage(h, al256((size_t)cb * HWn) + (net_logits ? 0 : al256((size_t)cb * HWn * 4))))) return rc;
    h->active_lanes = 1;
    if (area) HIPCHK(hipMemsetAsync(area, 0, (size_t)B * sizeof(int32_t), h->stream));
    rc = resized_dev_run(h, src, B, H, W, channels, net_h, net_w, thr, boxes, mask, area, net_logits, net_prob, prob, cb, (char*)h->stage);
    if (rc) {
        const std::string err = g_err;
        reset_counters(h);
        (void)hipStreamSynchronize(h->stream);   // error path only: nothing of this call is in flight when the error is reported
        g_err = err;
    }
    return rc;
}

int og_linear_taps_host(int src_len, int dst_len, int32_t* i0, int32_t* i1, float* frac, int32_t* a1) {
    if (src_len <= 0 || dst_len <= 0 || !i0 || !i1 || !frac || !a1) return fail(OG_EINVAL, "bad argument");
    OG_ALIGN(i0);
    OG_ALIGN(i1);
    OG_ALIGN(frac);
    OG_ALIGN(a1);
    for (int d = 0; d < dst_len; ++d) {
        int k0, k1;
        float f;
        og_linear_pos(d, src_len, dst_len, k0, k1, f);
        i0[d] = k0;
        i1[d] = k1;
        frac[d] = f;
        a1[d] = og_linear_coef(f);
    }
    return OG_OK;
}

int og_unet_segment_u8(og_unet* h, const uint8_t* gray, int B, int H, int W, float thr, const int32_t* boxes,
                       uint8_t* mask, int32_t* area, float* logits) {
    if (h && h->stream_host) return stream_impl(h, gray, nullptr, B, H, W, 1, thr, boxes, mask, area, logits);
    // one-shot staging of the whole batch ("stream" option 0; kept as the reference the streaming path is tested against)
    OG_SCOPE(h);
    int rc = check_shape(h, B, H, W);
    if (rc) return rc;
    OG_ALIGN(boxes);
    OG_ALIGN(area);
    OG_ALIGN(logits);
    if (B == 0) return OG_OK;
    if (!gray) return fail(OG_EINVAL, "gray is null");
    const size_t HW = (size_t)H * W;
    const size_t o_gray = 0, o_mask = al256(B * HW), o_area = o_mask + al256(B * HW), o_box = o_area + al256(B * 4),
                 o_log = o_box + al256(B * 16), tot = o_log + (logits ? al256(B * HW * 4) : 0);
    if ((rc = ensure_stage(h, tot))) return rc;
    char* s = (char*)h->stage;
    HIPCHK(hipMemcpyAsync(s + o_gray, gray, B * HW, hipMemcpyHostToDevice, h->stream));
    if (boxes) HIPCHK(hipMemcpyAsync(s + o_box, boxes, (size_t)B * 16, hipMemcpyHostToDevice, h->stream));
    rc = og_unet_segment_u8_dev(h, (const uint8_t*)(s + o_gray), B, H, W, thr, boxes ? (const int32_t*)(s + o_box) : nullptr,
                                mask ? (uint8_t*)(s + o_mask) : nullptr, area ? (int32_t*)(s + o_area) : nullptr,
                                logits ? (float*)(s + o_log) : nullptr);
    if (rc) return rc;
    if (mask) HIPCHK(hipMemcpyAsync(mask, s + o_mask, B * HW, hipMemcpyDeviceToHost, h->stream));
    if (area) HIPCHK(hipMemcpyAsync(area, s + o_area, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    if (logits) HIPCHK(hipMemcpyAsync(logits, s + o_log, B * HW * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return check_range(h);
}

int og_unet_forward_f32(og_unet* h, const float* x, int B, int H, int W, float* logits) {
    OG_SCOPE(h);
    int rc = check_shape(h, B, H, W);
    if (rc) return rc;
    if (B == 0) return OG_OK;
    if (!x || !logits) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(x);
    OG_ALIGN(logits);
    const size_t HW = (size_t)H * W;
    const size_t o_in = 0, o_out = al256(B * HW * 4), tot = o_out + al256(B * HW * 4);
    if ((rc = ensure_stage(h, tot))) return rc;
    char* s = (char*)h->stage;
    HIPCHK(hipMemcpyAsync(s + o_in, x, B * HW * 4, hipMemcpyHostToDevice, h->stream));
    const int chunk = effective_chunk(h);
    const int cb = chunk < B ? chunk : B;
    if ((rc = ensure_arena(h, cb, H, W))) return rc;
    const int taps_saved = h->keep_taps;
    h->active_lanes = 1;
    h->keep_taps = 1;  // the parity/debug entry point keeps every layer-boundary tensor readable
    for (int b0 = 0; b0 < B && !rc; b0 += chunk) {
        const int nb = (B - b0 < chunk) ? B - b0 : chunk;
        rc = run_chunk(h, KIND_F32, (const float*)(s + o_in) + b0 * HW, nb, H, W, 0.5f, nullptr, nullptr, nullptr,
                       (float*)(s + o_out) + b0 * HW);
    }
    h->keep_taps = taps_saved;
    if (rc) {
        const std::string err = g_err;
        reset_counters(h);
        (void)hipStreamSynchronize(h->stream);
        g_err = err;
        return rc;
    }
    HIPCHK(hipMemcpyAsync(logits, s + o_out, B * HW * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return check_range(h);
}

int og_mask_area_dev(og_unet* h, const uint8_t* mask, int B, int H, int W, const int32_t* boxes, int32_t* area) {
    if (!h || !h->finalized) return fail(OG_ESTATE, "handle not finalized");
    OG_SCOPE(h);
    if (!mask || !area || B < 0 || H <= 0 || W <= 0) return fail(OG_EINVAL, "bad argument");
    OG_ALIGN(boxes);
    OG_ALIGN(area);
    if (B == 0) return OG_OK;
    HIPCHK(hipMemsetAsync(area, 0, (size_t)B * 4, h->stream));
    const int HW = H * W, bpf = (HW + 4095) / 4096;
    hipLaunchKernelGGL(k_mask_area, dim3(B * bpf), dim3(256), 0, h->stream, mask, HW, W, boxes, area, bpf);
    HIPCHK(hipGetLastError());
    return OG_OK;
}

int og_bgr2gray_host(const uint8_t* bgr, long long n_pixels, uint8_t* gray) {
    if (n_pixels < 0 || (n_pixels > 0 && (!bgr || !gray))) return fail(OG_EINVAL, "bad argument");
    bgr2gray_host_loop(bgr, n_pixels, gray);
    return OG_OK;
}

int og_bgr2gray_dev(og_unet* h, const uint8_t* bgr, int B, int H, int W, uint8_t* gray) {
    if (!h || !h->finalized) return fail(OG_ESTATE, "handle not finalized");
    OG_SCOPE(h);
    if (!bgr || !gray || B < 0 || H <= 0 || W <= 0) return fail(OG_EINVAL, "bad argument");
    const long long n = (long long)B * H * W;
    if (n == 0) return OG_OK;
    hipLaunchKernelGGL(k_bgr2gray, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, bgr, gray, n);
    HIPCHK(hipGetLastError());
    return OG_OK;
}

int og_canvas_letterbox_u8_dev(og_unet* h, const uint8_t* packed, const int64_t* offsets, const int32_t* shapes, int B, int channels,
                               int size, const int32_t* geom, int value, uint8_t* out) {
    if (!h || !h->finalized) return fail(OG_ESTATE, "handle not finalized");
    OG_SCOPE(h);
    if (B < 0 || size <= 0 || (channels != 1 && channels != 3) || value < 0 || value > 255) return fail(OG_EINVAL, "bad argument");
    if (B == 0) return OG_OK;
    if (!packed || !offsets || !shapes || !geom || !out) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(offsets);
    OG_ALIGN(shapes);
    OG_ALIGN(geom);
    const size_t SS = (size_t)size * size * channels;
    for (int b0 = 0; b0 < B; b0 += 65535) {   // grid.y <= 65535
        const int nb = (B - b0 < 65535) ? B - b0 : 65535;
        const dim3 grid((size * size + 255) / 256, nb);
        if (channels == 1)
            hipLaunchKernelGGL(k_canvas_letterbox<1>, grid, dim3(256), 0, h->stream, packed, (const long long*)offsets + b0, shapes + 2 * b0,
                               geom + 4 * b0, size, value, out + b0 * SS);
        else
            hipLaunchKernelGGL(k_canvas_letterbox<3>, grid, dim3(256), 0, h->stream, packed, (const long long*)offsets + b0, shapes + 2 * b0,
                               geom + 4 * b0, size, value, out + b0 * SS);
        HIPCHK(hipGetLastError());
    }
    return OG_OK;
}

int og_canvas_letterbox_u8(og_unet* h, const uint8_t* packed, const int64_t* offsets, const int32_t* shapes, int B, int channels, int size,
                           const int32_t* geom, int value, uint8_t* out) {
    if (!h || !h->finalized) return fail(OG_ESTATE, "handle not finalized");
    OG_SCOPE(h);
    if (B < 0 || size <= 0 || (channels != 1 && channels != 3)) return fail(OG_EINVAL, "bad argument");
    if (B == 0) return OG_OK;
    if (!packed || !offsets || !shapes || !geom || !out) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(offsets);
    OG_ALIGN(shapes);
    OG_ALIGN(geom);
    size_t total = 0;
    for (int b = 0; b < B; ++b) {   // host variant: the records are readable here, so check them
        const long long hh = shapes[2 * b], ww = shapes[2 * b + 1];
        if (hh <= 0 || ww <= 0 || offsets[b] < 0) return fail(OG_EINVAL, "bad frame record " + std::to_string(b));
        const size_t end = (size_t)offsets[b] + (size_t)hh * ww * channels;
        if (end > total) total = end;
    }
    const size_t SS = (size_t)size * size * channels;
    const size_t o_pk = 0, o_off = al256(total), o_shp = o_off + al256((size_t)B * 8), o_geo = o_shp + al256((size_t)B * 8),
                 o_out = o_geo + al256((size_t)B * 16), tot = o_out + al256(B * SS);
    int rc;
    if ((rc = ensure_stage(h, tot))) return rc;
    char* s = (char*)h->stage;
    HIPCHK(hipMemcpyAsync(s + o_pk, packed, total, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(s + o_off, offsets, (size_t)B * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(s + o_shp, shapes, (size_t)B * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(s + o_geo, geom, (size_t)B * 16, hipMemcpyHostToDevice, h->stream));
    if ((rc = og_canvas_letterbox_u8_dev(h, (const uint8_t*)(s + o_pk), (const int64_t*)(s + o_off), (const int32_t*)(s + o_shp), B, channels,
                                         size, (const int32_t*)(s + o_geo), value, (uint8_t*)(s + o_out))))
        return rc;
    HIPCHK(hipMemcpyAsync(out, s + o_out, B * SS, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return OG_OK;
}

int og_mask_stats_dev(og_unet* h, const uint8_t* pred, const uint8_t* gt, int B, int H, int W, const int32_t* boxes, int32_t* stats) {
    if (!h || !h->finalized) return fail(OG_ESTATE, "handle not finalized");
    OG_SCOPE(h);
    if (!pred || !gt || !stats || B < 0 || H <= 0 || W <= 0) return fail(OG_EINVAL, "bad argument");
    OG_ALIGN(boxes);
    OG_ALIGN(stats);
    if (B == 0) return OG_OK;
    HIPCHK(hipMemsetAsync(stats, 0, (size_t)B * 12, h->stream));
    const int HW = H * W, bpf = (HW + 4095) / 4096;
    hipLaunchKernelGGL(k_mask_stats, dim3(B * bpf), dim3(256), 0, h->stream, pred, gt, HW, W, boxes, stats, bpf);
    HIPCHK(hipGetLastError());
    return OG_OK;
}

int og_unet_segment_crops_u8_dev(og_unet* h, const uint8_t* gray, int B, int H, int W, const int32_t* boxes, const int32_t* geom,
                                 int size, float thr, uint8_t* tiles_scratch, uint8_t* tile_masks_scratch, uint8_t* out_masks) {
    OG_SCOPE(h);
    int rc = check_shape(h, B, size, size);
    if (rc) return rc;
    if (B == 0) return OG_OK;
    if (!gray || !boxes || !geom || !tiles_scratch || !tile_masks_scratch || !out_masks || H <= 0 || W <= 0)
        return fail(OG_EINVAL, "null buffer / bad size");
    OG_ALIGN(boxes);
    OG_ALIGN(geom);
    const size_t HW = (size_t)H * W, SS = (size_t)size * size;
    for (int b0 = 0; b0 < B; b0 += 65535) {   // grid.y <= 65535
        const int nb = (B - b0 < 65535) ? B - b0 : 65535;
        hipLaunchKernelGGL(k_crop_letterbox, dim3((size * size + 255) / 256, nb), dim3(256), 0, h->stream, gray + b0 * HW, H, W, boxes + 4 * b0,
                           geom + 4 * b0, size, tiles_scratch + b0 * SS);
        HIPCHK(hipGetLastError());
    }
    if ((rc = og_unet_segment_u8_dev(h, tiles_scratch, B, size, size, thr, nullptr, tile_masks_scratch, nullptr, nullptr))) return rc;
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = (B - b0 < 65535) ? B - b0 : 65535;
        hipLaunchKernelGGL(k_unletterbox_paste, dim3((H * W + 255) / 256, nb), dim3(256), 0, h->stream, tile_masks_scratch + b0 * SS, size,
                           boxes + 4 * b0, geom + 4 * b0, H, W, out_masks + b0 * HW);
        HIPCHK(hipGetLastError());
    }
    return OG_OK;
}

int og_unet_segment_crops_u8(og_unet* h, const uint8_t* gray, int B, int H, int W, const int32_t* boxes, const int32_t* geom, int size,
                             float thr, uint8_t* out_masks) {
    OG_SCOPE(h);
    int rc = check_shape(h, B, size, size);
    if (rc) return rc;
    if (B == 0) return OG_OK;
    if (!gray || !boxes || !geom || !out_masks || H <= 0 || W <= 0) return fail(OG_EINVAL, "null buffer / bad size");
    OG_ALIGN(boxes);
    OG_ALIGN(geom);
    for (int b = 0; b < B; ++b) {   // "no detection" (x1 < 0) and empty boxes are legal (all-zero mask); anything else must index inside
        const int32_t *bx = boxes + 4 * b, *g = geom + 4 * b;
        if (bx[0] < 0 || bx[2] <= bx[0] || bx[3] <= bx[1]) continue;
        if (bx[1] < 0 || bx[2] > W || bx[3] > H)
            return fail(OG_EINVAL, "box " + std::to_string(b) + " reaches outside the frame (clamp it as python slicing does, normalize_box)");
        if (g[0] < 0 || g[1] < 0 || g[2] <= 0 || g[3] <= 0 || g[0] + g[2] > size || g[1] + g[3] > size)
            return fail(OG_EINVAL, "geom " + std::to_string(b) + " does not fit the size x size tile");
    }
    const size_t HW = (size_t)H * W, SS = (size_t)size * size;
    const size_t o_gray = 0, o_box = al256(B * HW), o_geo = o_box + al256((size_t)B * 16), o_til = o_geo + al256((size_t)B * 16),
                 o_tm = o_til + al256(B * SS), o_out = o_tm + al256(B * SS), tot = o_out + al256(B * HW);
    // a dedicated staging area: og_unet_segment_u8_dev does not touch h->stage, so it can be reused here
    if ((rc = ensure_stage(h, tot))) return rc;
    char* s = (char*)h->stage;
    HIPCHK(hipMemcpyAsync(s + o_gray, gray, B * HW, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(s + o_box, boxes, (size_t)B * 16, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(s + o_geo, geom, (size_t)B * 16, hipMemcpyHostToDevice, h->stream));
    rc = og_unet_segment_crops_u8_dev(h, (const uint8_t*)(s + o_gray), B, H, W, (const int32_t*)(s + o_box), (const int32_t*)(s + o_geo),
                                      size, thr, (uint8_t*)(s + o_til), (uint8_t*)(s + o_tm), (uint8_t*)(s + o_out));
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out_masks, s + o_out, B * HW, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return OG_OK;
}

int og_unet_get_activation(og_unet* h, const char* name, int B, float* out, size_t cap, int* dims) {
    if (!h || !h->finalized || !h->arena) return fail(OG_ESTATE, "no forward has run yet");
    if (!name || !out || !dims || B < 1 || B > h->lastB) return fail(OG_EINVAL, "bad argument (B must be <= last chunk size)");
    OG_ALIGN(out);
    OG_ALIGN(dims);
    const std::string n(name);
    const int L = h->L;
    const Act* a = nullptr;
    int off = 0, C = 0;
    auto level_of_up = [&](int k) { return L - 1 - k / 2; };
    if (n.rfind("downs.", 0) == 0 && n.size() >= 9) {
        const int i = atoi(n.c_str() + 6);
        if (i < 0 || i >= L) return fail(OG_EINVAL, "bad layer " + n);
        C = h->features[i];
        if (n.substr(n.size() - 2) == ".a") a = &h->A[i];
        else if (n.substr(n.size() - 2) == ".b") a = &h->CAT[i];
    } else if (n.rfind("pool", 0) == 0) {
        const int i = atoi(n.c_str() + 4);
        if (i < 0 || i >= L) return fail(OG_EINVAL, "bad layer " + n);
        a = &h->P[i];
        C = h->features[i];
    } else if (n == "bottleneck.a") {
        a = &h->BA;
        C = 2 * h->features[L - 1];
    } else if (n == "bottleneck.b") {
        a = &h->BB;
        C = 2 * h->features[L - 1];
    } else if (n.rfind("ups.", 0) == 0) {
        const int k = atoi(n.c_str() + 4);
        if (k < 0 || k >= 2 * L) return fail(OG_EINVAL, "bad layer " + n);
        const int i = level_of_up(k);
        C = h->features[i];
        if (k % 2 == 0) {
            a = &h->CAT[i];
            off = cp32(h->features[i]);
        } else if (n.substr(n.size() - 2) == ".a") a = &h->UA[i];
        else if (n.substr(n.size() - 2) == ".b") a = &h->UB[i];
    }
    if (!a) return fail(OG_EINVAL, "unknown activation name " + n);
    dims[0] = C;
    dims[1] = a->H;
    dims[2] = a->W;
    const size_t need = (size_t)B * C * a->H * a->W;
    if (cap < need) return fail(OG_EINVAL, "capacity too small");
    std::vector<float> tmp((size_t)B * a->frame_stride());
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(tmp.data(), a->p, tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
    const size_t HW = (size_t)a->H * a->W;
    if (h->precision == 2) {   // F layout: channel c of a pixel is the f16 at byte 2c; returned widened to f32
        const _Float16* t16 = (const _Float16*)tmp.data();
        for (int b = 0; b < B; ++b)
            for (int c = 0; c < C; ++c)
                for (size_t p = 0; p < HW; ++p) out[((size_t)b * C + c) * HW + p] = (float)t16[((size_t)b * HW + p) * a->C * 2 + off + c];
        return OG_OK;
    }
    if (h->precision == 1) {   // H layout: channel c of a pixel = hi + lo * 2^-11, hi / lo halves of its 32-channel chunk
        const _Float16* t16 = (const _Float16*)tmp.data();
        for (int b = 0; b < B; ++b)
            for (int c = 0; c < C; ++c) {
                const int cc = off + c, chunk = cc / 32, w = cc % 32;
                const size_t hoff = (size_t)chunk * 64 + (size_t)(w / 8) * 8 + (w % 8);   // in halves, within the pixel
                for (size_t p = 0; p < HW; ++p) {
                    const _Float16* px = t16 + ((size_t)b * HW + p) * a->C * 2;
                    out[((size_t)b * C + c) * HW + p] = (float)px[hoff] + (float)px[hoff + 32] * (1.0f / 2048.0f);
                }
            }
        return OG_OK;
    }
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c)
            for (size_t p = 0; p < HW; ++p) out[((size_t)b * C + c) * HW + p] = tmp[((size_t)b * HW + p) * a->C + off + c];
    return OG_OK;
}

int og_unet_profile(og_unet* h, const uint8_t* gray_dev, int B, int H, int W, int reps, int max_entries, char* layers,
                    char* kernels, float* ms, double* flops, int* n_entries) {
    OG_SCOPE(h);
    int rc = check_shape(h, B, H, W);
    if (rc) return rc;
    if (!gray_dev || B < 1 || reps < 1 || !layers || !kernels || !ms || !flops || !n_entries)
        return fail(OG_EINVAL, "bad argument");
    if ((rc = ensure_arena(h, B, H, W))) return rc;
    if ((rc = ensure_stage(h, al256((size_t)B * 4)))) return rc;
    std::vector<double> acc;
    std::vector<og_unet::ProfEntry> first;
    h->active_lanes = 1;   // the profile is one chain on one lane
    for (int r = 0; r < reps; ++r) {
        std::vector<og_unet::ProfEntry> tr;
        h->prof = &tr;
        HIPCHK(hipMemsetAsync(h->stage, 0, (size_t)B * 4, h->stream));
        pick_chain_form(h, B, H, W);
        const int kind = h->entry_f32 ? KIND_F32 : KIND_U8;
        const bool ff = can_fuse_first(h, kind, B, H, W);
        rc = ff ? enqueue_first_fused(h, gray_dev, B, H, W) : enqueue_first(h, kind, gray_dev, B, H, W);
        const bool fuse = can_fuse_head(h);
        if (!rc) rc = enqueue_body(h, B, fuse, ff);
        if (!rc)
            rc = fuse ? enqueue_last_with_head(h, B, 0.5f, nullptr, nullptr, (int32_t*)h->stage, nullptr)
                      : enqueue_head(h, B, H, W, 0.5f, nullptr, nullptr, (int32_t*)h->stage, nullptr);
        h->prof = nullptr;
        hipError_t e = hipStreamSynchronize(h->stream);
        if (acc.empty()) acc.assign(tr.size(), 0.0);
        for (size_t i = 0; i < tr.size(); ++i) {
            float t = 0.f;
            if (!rc && e == hipSuccess) (void)hipEventElapsedTime(&t, tr[i].e0, tr[i].e1);
            acc[i] += t;
            (void)hipEventDestroy(tr[i].e0);
            (void)hipEventDestroy(tr[i].e1);
        }
        if (r == 0) first = tr;
        if (rc) return rc;
        if (e != hipSuccess) return fail(OG_EHIP, std::string("profile sync: ") + hipGetErrorString(e));
    }
    const int n = (int)first.size();
    *n_entries = n;
    if (n > max_entries) return fail(OG_EINVAL, "max_entries too small");
    for (int i = 0; i < n; ++i) {
        snprintf(layers + 64 * i, 64, "%s", first[i].layer.c_str());
        snprintf(kernels + 64 * i, 64, "%s", first[i].kernel.c_str());
        ms[i] = (float)(acc[i] / reps);
        flops[i] = first[i].flops;
    }
    return OG_OK;
}

int og_unet_clock_probe(og_unet* h, const uint8_t* gray_dev, int B, int H, int W, int max_entries, double* mhz, int* n_entries) {
    OG_SCOPE(h);
    int rc = check_shape(h, B, H, W);
    if (rc) return rc;
    if (!gray_dev || !mhz || !n_entries || B < 1) return fail(OG_EINVAL, "bad argument");
    if ((rc = ensure_arena(h, B, H, W))) return rc;
    if ((rc = ensure_stage(h, al256((size_t)B * 4)))) return rc;
    const size_t nst = (size_t)64 * 1024 * 4;
    if (!h->d_stamps) HIPCHK(hipMalloc((void**)&h->d_stamps, nst * 8));
    HIPCHK(hipMemsetAsync(h->d_stamps, 0, nst * 8, h->stream));
    std::vector<og_unet::ProfEntry> tr;
    h->prof = &tr;
    h->probing = true;
    h->active_lanes = 1;
    pick_chain_form(h, B, H, W);   // the chain the product runs (og_unet_profile's), not whatever form the last call left behind
    rc = enqueue_first(h, KIND_U8, gray_dev, B, H, W);
    if (!rc) rc = enqueue_body(h, B);
    h->prof = nullptr;
    h->probing = false;
    hipError_t e = hipStreamSynchronize(h->stream);
    for (auto& t : tr) {
        (void)hipEventDestroy(t.e0);
        (void)hipEventDestroy(t.e1);
    }
    if (rc) return rc;
    if (e != hipSuccess) return fail(OG_EHIP, std::string("clock probe sync: ") + hipGetErrorString(e));
    std::vector<unsigned long long> st(nst);
    HIPCHK(hipMemcpy(st.data(), h->d_stamps, nst * 8, hipMemcpyDeviceToHost));
    const int n = (int)tr.size() < 64 ? (int)tr.size() : 64;
    *n_entries = n;
    if (n > max_entries) return fail(OG_EINVAL, "max_entries too small");
    for (int i = 0; i < n; ++i) {
        std::vector<double> v;
        for (int w = 0; w < 1024; ++w) {
            const unsigned long long* q = &st[((size_t)i * 1024 + w) * 4];
            const unsigned long long r0 = q[1] & 0xFFFFFFFFFFull, r1 = q[3] & 0xFFFFFFFFFFull;
            if (r1 > r0 && q[2] > q[0]) v.push_back((double)(q[2] - q[0]) / (double)(r1 - r0) * 100.0);
        }
        if (v.empty()) {
            mhz[i] = 0.0;
            continue;
        }
        std::sort(v.begin(), v.end());
        mhz[i] = v[v.size() / 2];  // median over workgroups; s_memrealtime ticks at 100 MHz
    }
    return OG_OK;
}

int og_unet_clock_probe_raw(og_unet* h, int entry, unsigned long long* out4x1024) {
    if (!h || !h->d_stamps || entry < 0 || entry >= 64 || !out4x1024) return fail(OG_EINVAL, "bad argument / no probe run yet");
    HIPCHK(hipMemcpy(out4x1024, h->d_stamps + (size_t)entry * 4096, 4096 * 8, hipMemcpyDeviceToHost));
    return OG_OK;
}

int og_unet_plan(const int* features, int n_levels, int B, int H, int W, int lanes, const char* options, char* out, size_t cap,
                 long long* arena_bytes) {
    if (!out || cap == 0 || B < 1) return fail(OG_EINVAL, "bad argument");
    og_unet* h = og_unet_create(features, n_levels, 1, 1);
    if (!h) return OG_EINVAL;
    h->host_only = true;
    int rc = og_unet_finalize(h);
    if (!rc) rc = check_shape(h, B, H, W);
    std::string opt = options ? options : "";
    for (size_t p0 = 0; !rc && p0 < opt.size();) {   // "name=value,name=value"
        size_t p1 = opt.find(',', p0);
        if (p1 == std::string::npos) p1 = opt.size();
        const std::string kv = opt.substr(p0, p1 - p0);
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) rc = fail(OG_EINVAL, "option without '=': " + kv);
        else rc = og_unet_set_option(h, kv.substr(0, eq).c_str(), atoi(kv.c_str() + eq + 1));
        p0 = p1 + 1;
    }
    Plan plan;
    if (!rc) {
        ArenaPlan ap = arena_layout(h, B, H, W);
        if (arena_bytes) *arena_bytes = (long long)ap.total;
        adopt_arena(h, ap, (void*)4096, B, H, W);   // a placeholder base: nothing dereferences it in a dry run
        h->active_lanes = lanes < 1 ? 1 : lanes;
        g_plan = &plan;
        // the product's chain for one micro-batch of u8 frames with areas wanted (run_chunk without the hipGraph plumbing)
        pick_chain_form(h, B, H, W);
        const int kind = h->entry_f32 ? KIND_F32 : KIND_U8;   // ("entry_f32" 1: the first launch of og_unet_forward_f32's chain)
        const bool ff = can_fuse_first(h, kind, B, H, W), fuse = can_fuse_head(h);
        rc = ff ? enqueue_first_fused(h, (const uint8_t*)4096, B, H, W) : enqueue_first(h, kind, (const void*)4096, B, H, W);
        if (!rc) rc = enqueue_body(h, B, fuse, ff);
        if (!rc) rc = fuse ? enqueue_last_with_head(h, B, 0.5f, nullptr, nullptr, (int32_t*)4096, nullptr)
                           : enqueue_head(h, B, H, W, 0.5f, nullptr, nullptr, (int32_t*)4096, nullptr);
        g_plan = nullptr;
    }
    og_unet_destroy(h);
    if (rc) return rc;
    return og_plan_text(plan, kPlanNoLast, out, cap);
}

int og_unet_plan_resized(const int* features, int n_levels, int B, int H, int W, int channels, int net_h, int net_w, int lanes,
                         const char* options, char* out, size_t cap, long long* arena_bytes) {
    if (!out || cap == 0 || B < 1) return fail(OG_EINVAL, "bad argument");
    og_unet* h = og_unet_create(features, n_levels, 1, 1);
    if (!h) return OG_EINVAL;
    h->host_only = true;
    int rc = og_unet_finalize(h);
    if (!rc) rc = check_resized(h, B, H, W, channels, net_h, net_w);
    std::string opt = options ? options : "";
    for (size_t p0 = 0; !rc && p0 < opt.size();) {   // "name=value,name=value"
        size_t p1 = opt.find(',', p0);
        if (p1 == std::string::npos) p1 = opt.size();
        const std::string kv = opt.substr(p0, p1 - p0);
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) rc = fail(OG_EINVAL, "option without '=': " + kv);
        else rc = og_unet_set_option(h, kv.substr(0, eq).c_str(), atoi(kv.c_str() + eq + 1));
        p0 = p1 + 1;
    }
    Plan plan;
    if (!rc) {
        const int chunk = resized_chunk(h, H, W, channels), cb = chunk < B ? chunk : B;
        ArenaPlan ap = arena_layout(h, cb, net_h, net_w);
        if (arena_bytes) *arena_bytes = (long long)ap.total;
        adopt_arena(h, ap, (void*)4096, cb, net_h, net_w);   // placeholder bases: nothing dereferences them in a dry run
        h->active_lanes = lanes < 1 ? 1 : lanes;
        // og_unet_segment_resized_u8_dev with every caller-owned output asked for, each at its own placeholder base
        const uintptr_t gap = (uintptr_t)1 << 40;
        uint8_t* mask = (uint8_t*)(1 * gap);
        int32_t* area = (int32_t*)(2 * gap);
        float* net_logits = (float*)(3 * gap);
        float* net_prob = (float*)(4 * gap);
        float* prob = (float*)(5 * gap);
        plan.bases = {{"mask", mask}, {"area", area}, {"net_logits", net_logits}, {"net_prob", net_prob}, {"prob", prob}};
        g_plan = &plan;
        rc = resized_dev_run(h, (const uint8_t*)(6 * gap), B, H, W, channels, net_h, net_w, 0.5f, (const int32_t*)(7 * gap), mask, area,
                             net_logits, net_prob, prob, cb, (char*)(8 * gap));
        g_plan = nullptr;
    }
    og_unet_destroy(h);
    if (rc) return rc;
    return og_plan_text(plan, kPlanWrites, out, cap);
}

long long og_workspace_limit(int which) { return which == 0 ? (long long)kPartialBytes : which == 1 ? kTileCounters : which == 2 ? 65535 : 160 * 1024; }

double og_unet_flops_per_frame(og_unet* h, int H, int W) {
    if (!h) return 0.0;
    const int L = h->L;
    double mac = 0;
    int ch = 1;
    for (int i = 0; i < L; ++i) {
        const double px = (double)(H >> i) * (W >> i);
        mac += px * 9.0 * ch * h->features[i] + px * 9.0 * h->features[i] * h->features[i];
        ch = h->features[i];
    }
    const double pb = (double)(H >> L) * (W >> L);
    mac += pb * 9.0 * ch * 2 * ch + pb * 9.0 * 2 * ch * 2 * ch;
    for (int i = L - 1; i >= 0; --i) {
        const double f = h->features[i];
        const double pin = (double)(H >> (i + 1)) * (W >> (i + 1));
        const double px = (double)(H >> i) * (W >> i);
        mac += pin * 4.0 * (2 * f) * f;             // ConvTranspose2d(2f, f, 2, 2)
        mac += px * 9.0 * (2 * f) * f + px * 9.0 * f * f;
    }
    mac += (double)H * W * h->features[0];           // head 1x1
    return 2.0 * mac;
}

}  // extern "C"
