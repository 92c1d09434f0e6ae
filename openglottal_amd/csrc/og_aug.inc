// Crop-training batches augmented on the device (include_enc/openglottal_hip_aug.h): flips, rotation, rescale with crop or pad,
// noise, blur, brightness and contrast of the reference's `_tensor_and_augment`, in its order, on tiles that stay resident as u8.
// Included by og_api.hip after og_pnge.inc; the kernels live here too.  A handle of its own on the streaming base of og_stream.inc:
// one stream, the workspace of ONE micro-batch, two pinned host slots for the records.  Per micro-batch: k_aug_rotate, k_aug_scale,
// k_aug_blur, k_aug_contrast (k_aug_plain alone without augmentation).  The host twin and the kernels call the same inline functions,
// all written without contraction, and agree bit for bit.
// With OG_PNG_HOST_ONLY defined (after og_png.inc, in the same translation unit) only the twin is compiled, no HIP
// (tools/aug_host_check.cpp builds it under sanitizers).
#include "../../include_enc/openglottal_hip_aug.h"

#include <cmath>

constexpr int kAugMinS = 8, kAugMaxS = 1024, kAugMaxChunk = 1024;
constexpr int kAugMaxScale = 2;       // ceil(S / 2) <= new_size <= 2 S: at most 5 taps per axis
constexpr int kAugMaxTaps = 8;
constexpr int kAugBlock = 1024;       // pixels per block of the contrast mean: 256 lanes, 4 pixels each
constexpr int kAugThreads = 256;
static_assert(sizeof(og_aug_params) == 64 && offsetof(og_aug_params, noise_key) == 24 && offsetof(og_aug_params, k1) == 32 &&
                  offsetof(og_aug_params, contrast) == 56,
              "layout stated in the header");

// ---- the arithmetic: host twin and kernels ---------------------------------------------------------------------------------------
OG_PNG_HD uint32_t og_aug_bits(float v) {
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    return b;
}
OG_PNG_HD float og_aug_float(uint32_t b) {
    float v;
    __builtin_memcpy(&v, &b, 4);
    return v;
}
OG_PNG_HD float og_aug_clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }
OG_PNG_HD float og_aug_unit(uint8_t v) { return (float)v / 255.0f; }

OG_PNG_HD uint64_t og_aug_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// The standard normal deviate of (key, i): Box-Muller, sqrt(-2 ln u1) cos(2 pi u2), u1 and u2 from the two halves of a 64-bit word.
// ln: u1 = m 2^e, m in (sqrt(1/2), sqrt 2], ln m = 2 atanh(s), s = (m - 1) / (m + 1), the series to s^9.  cos: a quadrant from two bits,
// the angle inside it from 23, sine and cosine on [0, pi/2] by their series to a^13 and a^14.  Only integer operations, +, *, fmaf,
// sqrt and division.
OG_PNG_HD float og_aug_noise(uint64_t key, uint64_t i) {
#pragma clang fp contract(off)
    const uint64_t x = og_aug_mix(og_aug_mix(key + 0x9E3779B97F4A7C15ull) + (i + 1) * 0x9E3779B97F4A7C15ull);   // splitmix64 from the mixed key
    const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
    const float u1 = ((float)(hi >> 9) + 0.5f) * 1.1920928955078125e-07f;   // (k + 1/2) 2^-23: exact, inside (0, 1)
    const uint32_t ub = og_aug_bits(u1);
    int e = (int)(ub >> 23) - 127;
    float m = og_aug_float((ub & 0x007FFFFFu) | 0x3F800000u);
    if (m > 1.41421354f) {
        m *= 0.5f;
        e += 1;
    }
    const float f = m - 1.0f;
    const float s = f / (2.0f + f);
    const float z = s * s;
    const float p = fmaf(z, fmaf(z, fmaf(z, fmaf(z, 0.111111111f, 0.142857143f), 0.2f), 0.333333333f), 1.0f);
    const float ln = fmaf((float)e, 0.693147182f, 2.0f * s * p);
    float r2 = -2.0f * ln;
    r2 = r2 < 0.0f ? 0.0f : r2;
    const float radius = sqrtf(r2);
    const float t = ((float)((lo >> 7) & 0x007FFFFFu) + 0.5f) * 1.1920928955078125e-07f;
    const float a = t * 1.57079637f, q = a * a;
    const float sn = a * fmaf(q, fmaf(q, fmaf(q, fmaf(q, fmaf(q, fmaf(q, 1.60590438e-10f, -2.50521084e-08f), 2.75573192e-06f), -1.98412698e-04f),
                                           8.33333333e-03f), -1.66666667e-01f), 1.0f);
    const float cs = fmaf(q, fmaf(q, fmaf(q, fmaf(q, fmaf(q, fmaf(q, fmaf(q, -1.14707456e-11f, 2.08767570e-09f), -2.75573192e-07f), 2.48015873e-05f),
                                           -1.38888889e-03f), 4.16666667e-02f), -0.5f), 1.0f);
    const uint32_t quad = lo >> 30;
    const float c = quad == 0 ? cs : quad == 1 ? -sn : quad == 2 ? -cs : sn;
    return radius * c;
}

// ROTATE, one output pixel.  img(y, x) / msk(y, x): the (flipped) input at an index INSIDE [0, S)^2.
template <class FI, class FM>
OG_PNG_HD void og_aug_rotate_px(FI&& img, FM&& msk, int S, float c, float s, int i, int j, float* oI, uint8_t* oM) {
#pragma clang fp contract(off)
    const float half = 0.5f * (float)S, ctr = 0.5f * (float)(S - 1);
    const float X = ((float)j + 0.5f) - half, Y = ((float)i + 0.5f) - half;
    const float sx = (c * X - s * Y) + ctr, sy = (s * X + c * Y) + ctr;
    const float fx0 = floorf(sx), fy0 = floorf(sy);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float tx = sx - fx0, ty = sy - fy0, ux = 1.0f - tx, uy = 1.0f - ty;
    const bool xa = x0 >= 0 && x0 < S, xb = x0 + 1 >= 0 && x0 + 1 < S, ya = y0 >= 0 && y0 < S, yb = y0 + 1 >= 0 && y0 + 1 < S;
    const float v00 = (ya && xa) ? img(y0, x0) : 0.0f, v01 = (ya && xb) ? img(y0, x0 + 1) : 0.0f;
    const float v10 = (yb && xa) ? img(y0 + 1, x0) : 0.0f, v11 = (yb && xb) ? img(y0 + 1, x0 + 1) : 0.0f;
    *oI = ((v00 * (ux * uy) + v01 * (tx * uy)) + v10 * (ux * ty)) + v11 * (tx * ty);
    const int nx = (int)rintf(sx), ny = (int)rintf(sy);   // round half to even
    *oM = (nx >= 0 && nx < S && ny >= 0 && ny < S) ? msk(ny, nx) : (uint8_t)0;
}

// the taps of output index i of an antialiased bilinear resize in -> out: input indices [lo, lo + n), weights normalised
struct OgAugTaps {
    int lo, n;
    float w[kAugMaxTaps];
};
OG_PNG_HD void og_aug_aa_taps(int in, int out, int i, OgAugTaps* t) {
#pragma clang fp contract(off)
    const float scale = (float)in / (float)out;
    const float sup = scale >= 1.0f ? scale : 1.0f;
    const float inv = scale >= 1.0f ? 1.0f / scale : 1.0f;
    const float c = scale * ((float)i + 0.5f);
    int lo = (int)(c - sup + 0.5f), hi = (int)(c + sup + 0.5f);
    lo = lo < 0 ? 0 : lo;
    hi = hi > in ? in : hi;
    int n = hi - lo;
    n = n < 0 ? 0 : (n > kAugMaxTaps ? kAugMaxTaps : n);   // (at most 5 inside the limits)
    float total = 0.0f;
    for (int k = 0; k < n; ++k) {
        const float x = ((float)(k + lo) - c + 0.5f) * inv;
        const float ax = x < 0.0f ? -x : x;
        const float w = ax < 1.0f ? 1.0f - ax : 0.0f;
        t->w[k] = w;
        total += w;
    }
    for (int k = 0; k < n; ++k) t->w[k] = total != 0.0f ? t->w[k] / total : 0.0f;
    t->lo = lo;
    t->n = n;
}
OG_PNG_HD int og_aug_nearest(int in, int out, int d) {
#pragma clang fp contract(off)
    const float scale = (float)in / (float)out;
    const int s = (int)floorf((float)d * scale);
    return s < in - 1 ? s : in - 1;
}

// RESCALE with its crop or pad, one pixel (y, x) of the S x S window; new_size != 0
template <class FI, class FM>
OG_PNG_HD void og_aug_scale_px(FI&& img, FM&& msk, int S, int new_size, int y, int x, float* oI, uint8_t* oM) {
#pragma clang fp contract(off)
    const int shift = new_size > S ? (new_size - S) / 2 : -((S - new_size) / 2);
    const int r = y + shift, q = x + shift;
    if (r < 0 || r >= new_size || q < 0 || q >= new_size) {
        *oI = 0.0f;
        *oM = 0;
        return;
    }
    OgAugTaps ty, tx;
    og_aug_aa_taps(S, new_size, r, &ty);
    og_aug_aa_taps(S, new_size, q, &tx);
    float acc = 0.0f;
    for (int ky = 0; ky < ty.n; ++ky) {
        float row = 0.0f;
        for (int kx = 0; kx < tx.n; ++kx) row += tx.w[kx] * img(ty.lo + ky, tx.lo + kx);
        acc += ty.w[ky] * row;
    }
    *oI = acc;
    *oM = msk(og_aug_nearest(S, new_size, r), og_aug_nearest(S, new_size, q));
}

OG_PNG_HD float og_aug_noise_px(float v, float sigma, uint64_t key, uint64_t i) {
#pragma clang fp contract(off)
    const float n = og_aug_noise(key, i) * sigma;
    return og_aug_clamp01(v + n);
}

OG_PNG_HD int og_aug_reflect(int v, int S) { return v < 0 ? -v : (v >= S ? 2 * S - 2 - v : v); }
// BLUR, one pixel; ks 3 or 5
template <class FI>
OG_PNG_HD float og_aug_blur_px(FI&& img, int S, int ks, const float* k1, int y, int x) {
#pragma clang fp contract(off)
    const int r = ks / 2;
    float acc = 0.0f;
    for (int dy = 0; dy < ks; ++dy) {
        const int yy = og_aug_reflect(y + dy - r, S);
        for (int dx = 0; dx < ks; ++dx) acc += (k1[dy] * k1[dx]) * img(yy, og_aug_reflect(x + dx - r, S));
    }
    return acc;
}
OG_PNG_HD float og_aug_bright_px(float v, float f) {
#pragma clang fp contract(off)
    return og_aug_clamp01(v * f);
}
OG_PNG_HD float og_aug_contrast_px(float v, float r, float mean) {
#pragma clang fp contract(off)
    const float a = r * v, b = (1.0f - r) * mean;
    return og_aug_clamp01(a + b);
}
OG_PNG_HD float og_aug_mean(float sum, int S) { return sum / (float)(S * S); }

#ifndef OG_PNG_HOST_ONLY
// ---- kernels ---------------------------------------------------------------------------------------------------------------------
// (flipped) pixel (y, x) of a u8 tile
__device__ __forceinline__ int aug_flip_at(int y, int x, int S, uint32_t flips) {
    return ((flips & 2u) ? S - 1 - y : y) * S + ((flips & 1u) ? S - 1 - x : x);
}

// grid (ceil(S^2 / 256), nb): a lane per pixel.  rot_img [nb,S,S] f32, rot_msk [nb,S,S] u8 (0 or 1).
__global__ __launch_bounds__(kAugThreads) void k_aug_rotate(const uint8_t* __restrict__ images, const uint8_t* __restrict__ masks, int N, int S,
                                                            const int32_t* __restrict__ idx, const og_aug_params* __restrict__ params,
                                                            float* __restrict__ rot_img, uint8_t* __restrict__ rot_msk) {
    const int b = blockIdx.y, px = blockIdx.x * kAugThreads + threadIdx.x, P = S * S;
    if (px >= P) return;
    const int n = idx[b];
    const og_aug_params& p = params[b];
    float oI = 0.0f;
    uint8_t oM = 0;
    if (n >= 0 && n < N) {   // (an index outside the tiles reads nothing)
        const uint8_t* im = images + (long long)n * P;
        const uint8_t* mk = masks + (long long)n * P;
        const uint32_t flips = p.flips;
        og_aug_rotate_px([&](int y, int x) { return og_aug_unit(im[aug_flip_at(y, x, S, flips)]); },
                         [&](int y, int x) { return (uint8_t)(mk[aug_flip_at(y, x, S, flips)] > 0 ? 1 : 0); }, S, p.cos_t, p.sin_t, px / S, px % S, &oI,
                         &oM);
    }
    rot_img[(long long)b * P + px] = oI;
    rot_msk[(long long)b * P + px] = oM;
}

// grid (ceil(S^2 / 256), nb).  sc_img [nb,S,S] f32; out_msk: the caller's, f32 0 or 1.
__global__ __launch_bounds__(kAugThreads) void k_aug_scale(const float* __restrict__ rot_img, const uint8_t* __restrict__ rot_msk, int S,
                                                           const og_aug_params* __restrict__ params, float* __restrict__ sc_img,
                                                           float* __restrict__ out_msk) {
    const int b = blockIdx.y, px = blockIdx.x * kAugThreads + threadIdx.x, P = S * S;
    if (px >= P) return;
    const og_aug_params& p = params[b];
    const float* im = rot_img + (long long)b * P;
    const uint8_t* mk = rot_msk + (long long)b * P;
    float v = im[px];
    uint8_t m = mk[px];
    if (p.new_size != 0)
        og_aug_scale_px([&](int y, int x) { return im[y * S + x]; }, [&](int y, int x) { return mk[y * S + x]; }, S, p.new_size, px / S, px % S, &v, &m);
    if (p.noise_sigma != 0.0f) v = og_aug_noise_px(v, p.noise_sigma, p.noise_key, (uint64_t)px);
    sc_img[(long long)b * P + px] = v;
    out_msk[(long long)b * P + px] = m ? 1.0f : 0.0f;
}

// grid (ceil(S^2 / 1024), nb): a workgroup per block of the mean.  bl_img [nb,S,S] f32, sums [nb][gridDim.x].
__global__ __launch_bounds__(kAugThreads) void k_aug_blur(const float* __restrict__ sc_img, int S, const og_aug_params* __restrict__ params,
                                                          float* __restrict__ bl_img, float* __restrict__ sums) {
    __shared__ float s_sum[kAugThreads];
    const int b = blockIdx.y, t = threadIdx.x, P = S * S;
    const og_aug_params& p = params[b];
    const float* im = sc_img + (long long)b * P;
    float lane = 0.0f;
#pragma unroll
    for (int q = 0; q < kAugBlock / kAugThreads; ++q) {
        const int px = blockIdx.x * kAugBlock + q * kAugThreads + t;
        float v = 0.0f;
        if (px < P) {
            v = im[px];
            if (p.ks != 0) v = og_aug_blur_px([&](int y, int x) { return im[y * S + x]; }, S, p.ks, p.k1, px / S, px % S);
            if (p.brightness != 0.0f) v = og_aug_bright_px(v, p.brightness);
            bl_img[(long long)b * P + px] = v;
        }
        lane += v;
    }
    s_sum[t] = lane;
    __syncthreads();
#pragma unroll
    for (int d = kAugThreads / 2; d > 0; d >>= 1) {
        if (t < d) s_sum[t] += s_sum[t + d];
        __syncthreads();
    }
    if (t == 0) sums[(long long)b * gridDim.x + blockIdx.x] = s_sum[0];
}

// grid (ceil(S^2 / 1024), nb).  out_img: the caller's.
__global__ __launch_bounds__(kAugThreads) void k_aug_contrast(const float* __restrict__ bl_img, int S, const og_aug_params* __restrict__ params,
                                                              const float* __restrict__ sums, float* __restrict__ out_img) {
    __shared__ float s_part[kAugMaxS * kAugMaxS / kAugBlock];
    __shared__ float s_mean;
    const int b = blockIdx.y, t = threadIdx.x, P = S * S, nblk = gridDim.x;
    const float r = params[b].contrast;
    if (r != 0.0f) {
        for (int k = t; k < nblk; k += kAugThreads) s_part[k] = sums[(long long)b * nblk + k];
        __syncthreads();
        if (t == 0) {
            float sum = 0.0f;
            for (int k = 0; k < nblk; ++k) sum += s_part[k];
            s_mean = og_aug_mean(sum, S);
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < kAugBlock / kAugThreads; ++q) {
        const int px = blockIdx.x * kAugBlock + q * kAugThreads + t;
        if (px >= P) continue;
        const float v = bl_img[(long long)b * P + px];
        out_img[(long long)b * P + px] = r != 0.0f ? og_aug_contrast_px(v, r, s_mean) : v;
    }
}

// grid (ceil(S^2 / 256), nb): augment = 0
__global__ __launch_bounds__(kAugThreads) void k_aug_plain(const uint8_t* __restrict__ images, const uint8_t* __restrict__ masks, int N, int S,
                                                           const int32_t* __restrict__ idx, float* __restrict__ out_img, float* __restrict__ out_msk) {
    const int b = blockIdx.y, px = blockIdx.x * kAugThreads + threadIdx.x, P = S * S;
    if (px >= P) return;
    const int n = idx[b];
    const bool ok = n >= 0 && n < N;
    out_img[(long long)b * P + px] = ok ? og_aug_unit(images[(long long)n * P + px]) : 0.0f;
    out_msk[(long long)b * P + px] = (ok && masks[(long long)n * P + px] > 0) ? 1.0f : 0.0f;
}
#endif   // OG_PNG_HOST_ONLY

// ---- host side -------------------------------------------------------------------------------------------------------------------
#ifndef OG_PNG_HOST_ONLY
struct og_aug : OgStreamHandle {
    OgBuf<uint8_t> d_ws;   // two f32 planes and one u8 plane per sample, the blocks' sums, the records
    struct Slot {
        OgBuf<uint8_t> h_par{true};
        hipEvent_t ev = nullptr;
        bool used = false;
    } slots[2];
    unsigned turn = 0;
};
#endif

namespace {

int check_aug_S(int S) {
    if (S < kAugMinS || S > kAugMaxS) return fail(OG_EINVAL, "S must be " + std::to_string(kAugMinS) + ".." + std::to_string(kAugMaxS));
    return OG_OK;
}
bool aug_finite(float v) { return v == v && v - v == 0.0f; }
int check_aug_params(const og_aug_params& p, int S, long long at) {
    const std::string who = "record " + std::to_string(at) + ": ";
    if (p.flips > 3u) return fail(OG_EINVAL, who + "flips has bits above 1");
    if (!aug_finite(p.cos_t) || !aug_finite(p.sin_t) || p.cos_t < -1.0f || p.cos_t > 1.0f || p.sin_t < -1.0f || p.sin_t > 1.0f)
        return fail(OG_EINVAL, who + "cos_t and sin_t must lie in [-1, 1]");
    if (p.new_size != 0 && (p.new_size < (S + 1) / 2 || p.new_size > kAugMaxScale * S))
        return fail(OG_EINVAL, who + "new_size must be 0 or " + std::to_string((S + 1) / 2) + ".." + std::to_string(kAugMaxScale * S));
    if (!aug_finite(p.noise_sigma) || p.noise_sigma < 0.0f) return fail(OG_EINVAL, who + "noise_sigma must be finite and not negative");
    if (p.ks != 0 && p.ks != 3 && p.ks != 5) return fail(OG_EINVAL, who + "ks must be 0, 3 or 5");
    for (int k = 0; k < p.ks; ++k)
        if (!aug_finite(p.k1[k])) return fail(OG_EINVAL, who + "k1 must be finite");
    if (!aug_finite(p.brightness) || p.brightness < 0.0f) return fail(OG_EINVAL, who + "brightness must be finite and not negative");
    if (!aug_finite(p.contrast) || p.contrast < 0.0f) return fail(OG_EINVAL, who + "contrast must be finite and not negative");
    return OG_OK;
}

// the twin's stages on whole planes
void aug_flip_host(const float* in, const uint8_t* im, int S, uint32_t flips, float* out, uint8_t* om) {
    for (int y = 0; y < S; ++y)
        for (int x = 0; x < S; ++x) {
            const int src = ((flips & 2u) ? S - 1 - y : y) * S + ((flips & 1u) ? S - 1 - x : x);
            out[y * S + x] = in[src];
            if (im) om[y * S + x] = im[src];
        }
}
void aug_rotate_host(const float* in, const uint8_t* im, int S, float c, float s, float* out, uint8_t* om) {
    for (int y = 0; y < S; ++y)
        for (int x = 0; x < S; ++x) {
            uint8_t m;
            og_aug_rotate_px([&](int yy, int xx) { return in[yy * S + xx]; }, [&](int yy, int xx) { return im ? im[yy * S + xx] : (uint8_t)0; }, S, c, s, y,
                             x, &out[y * S + x], &m);
            if (im) om[y * S + x] = m;
        }
}
void aug_scale_host(const float* in, const uint8_t* im, int S, int new_size, float* out, uint8_t* om) {
    for (int y = 0; y < S; ++y)
        for (int x = 0; x < S; ++x) {
            uint8_t m;
            og_aug_scale_px([&](int yy, int xx) { return in[yy * S + xx]; }, [&](int yy, int xx) { return im ? im[yy * S + xx] : (uint8_t)0; }, S, new_size,
                            y, x, &out[y * S + x], &m);
            if (im) om[y * S + x] = m;
        }
}
// the mean of a plane in the order of k_aug_blur and k_aug_contrast
float aug_mean_host(const float* v, int S) {
    const int P = S * S;
    float sum = 0.0f;
    for (int base = 0; base < P; base += kAugBlock) {
        float lanes[kAugThreads];
        for (int t = 0; t < kAugThreads; ++t) {
            float lane = 0.0f;
            for (int q = 0; q < kAugBlock / kAugThreads; ++q) {
                const int px = base + q * kAugThreads + t;
                lane += px < P ? v[px] : 0.0f;
            }
            lanes[t] = lane;
        }
        for (int d = kAugThreads / 2; d > 0; d >>= 1)
            for (int t = 0; t < d; ++t) lanes[t] += lanes[t + d];
        sum += lanes[0];
    }
    return og_aug_mean(sum, S);
}

// one stage, 1..7; an off stage copies
void aug_stage_host(int stage, const float* in, const uint8_t* im, int S, const og_aug_params& p, float* out, uint8_t* om) {
    const size_t P = (size_t)S * S;
    const bool geo = stage == 1 || stage == 2 || (stage == 3 && p.new_size != 0);
    if (!geo && im) memcpy(om, im, P);
    switch (stage) {
        case 1: aug_flip_host(in, im, S, p.flips, out, om); return;
        case 2: aug_rotate_host(in, im, S, p.cos_t, p.sin_t, out, om); return;
        case 3:
            if (p.new_size != 0) { aug_scale_host(in, im, S, p.new_size, out, om); return; }
            break;
        case 4:
            if (p.noise_sigma != 0.0f) {
                for (size_t i = 0; i < P; ++i) out[i] = og_aug_noise_px(in[i], p.noise_sigma, p.noise_key, i);
                return;
            }
            break;
        case 5:
            if (p.ks != 0) {
                for (int y = 0; y < S; ++y)
                    for (int x = 0; x < S; ++x) out[y * S + x] = og_aug_blur_px([&](int yy, int xx) { return in[yy * S + xx]; }, S, p.ks, p.k1, y, x);
                return;
            }
            break;
        case 6:
            if (p.brightness != 0.0f) {
                for (size_t i = 0; i < P; ++i) out[i] = og_aug_bright_px(in[i], p.brightness);
                return;
            }
            break;
        default:
            if (p.contrast != 0.0f) {
                const float mean = aug_mean_host(in, S);
                for (size_t i = 0; i < P; ++i) out[i] = og_aug_contrast_px(in[i], p.contrast, mean);
                return;
            }
            break;
    }
    memcpy(out, in, P * sizeof(float));
}

#ifndef OG_PNG_HOST_ONLY
int aug_blocks(int S) { return (S * S + kAugBlock - 1) / kAugBlock; }
long long aug_up16(long long v) { return (v + 15) & ~15ll; }
// device workspace of a micro-batch of nb samples: every part a multiple of 16 bytes
long long aug_ws_bytes(int S, int nb, int augment) {
    if (!augment) return 0;
    const long long P = (long long)S * S;
    return 2 * aug_up16(4 * P * nb) + aug_up16(P * nb) + aug_up16(4ll * aug_blocks(S) * nb) + (long long)sizeof(og_aug_params) * nb;
}
int aug_chunk(int chunk, int S) {
    const long long fit = kMjpegBatchBytes / aug_ws_bytes(S, 1, 1);
    return (int)(fit < 1 ? 1 : (fit < chunk ? fit : chunk));
}
og_aug_params* aug_ws_params(uint8_t* ws, int S, int cb) { return (og_aug_params*)(ws + aug_ws_bytes(S, cb, 1) - (long long)sizeof(og_aug_params) * cb); }

void aug_free(og_aug* h) {
    og_release(h->d_ws);
    for (auto& s : h->slots) {
        og_release(s.h_par);
        if (s.ev) (void)hipEventDestroy(s.ev);
    }
}

// One micro-batch of nb samples.  ws: the handle's workspace, laid out for cb >= nb samples (a placeholder in a dry run), its records
// already on the device.
int aug_batch(hipStream_t st, uint8_t* ws, int cb, const uint8_t* images, const uint8_t* masks, int N, int S, const int32_t* idx, int nb,
              int augment, float* out_img, float* out_msk) {
    const long long P = (long long)S * S;
    const dim3 lanes((unsigned)((P + kAugThreads - 1) / kAugThreads), (unsigned)nb), blocks((unsigned)aug_blocks(S), (unsigned)nb);
    if (!augment) {
        OG_LAUNCH(k_aug_plain, lanes, dim3(kAugThreads), 0, st, images, masks, N, S, idx, out_img, out_msk);
        if (g_plan) {
            plan_write("out_img", out_img, 4 * P * nb);
            plan_write("out_msk", out_msk, 4 * P * nb);
        }
        return OG_OK;
    }
    float* a = (float*)ws;
    float* bb = (float*)(ws + aug_up16(4 * P * cb));
    uint8_t* mk = ws + 2 * aug_up16(4 * P * cb);
    float* sums = (float*)(mk + aug_up16(P * cb));
    const og_aug_params* par = aug_ws_params(ws, S, cb);
    plan_need(aug_ws_bytes(S, nb, 1), 0);
    OG_LAUNCH(k_aug_rotate, lanes, dim3(kAugThreads), 0, st, images, masks, N, S, idx, par, a, mk);
    OG_LAUNCH(k_aug_scale, lanes, dim3(kAugThreads), 0, st, (const float*)a, (const uint8_t*)mk, S, par, bb, out_msk);
    if (g_plan) plan_write("out_msk", out_msk, 4 * P * nb);
    OG_LAUNCH(k_aug_blur, blocks, dim3(kAugThreads), 0, st, (const float*)bb, S, par, a, sums);
    if (g_plan) g_plan->recs.back().lds = 4 * kAugThreads;   // static LDS: stated, so that the plan tells the truth
    OG_LAUNCH(k_aug_contrast, blocks, dim3(kAugThreads), 0, st, (const float*)a, S, par, (const float*)sums, out_img);
    if (g_plan) {
        g_plan->recs.back().lds = 4 * (kAugMaxS * kAugMaxS / kAugBlock) + 4;
        plan_write("out_img", out_img, 4 * P * nb);
    }
    return OG_OK;
}
#endif   // OG_PNG_HOST_ONLY

}  // namespace

extern "C" {

long long og_aug_limit(int which) {
    switch (which) {
        case 0: return kAugMinS;
        case 1: return kAugMaxS;
        case 2: return kAugMaxChunk;
        case 3: return 128;
        case 4: return kAugMaxScale;
        case 5: return (long long)sizeof(og_aug_params);
        case 6: return kAugBlock;
        case 7: return kAugMaxTaps;
        default: return -1;
    }
}

int og_aug_stage_host(int stage, const float* in_img, const uint8_t* in_msk, int S, const og_aug_params* p, float* out_img, uint8_t* out_msk) {
    if (stage < 1 || stage > 7) return fail(OG_EINVAL, "stage must be 1..7");
    int rc = check_aug_S(S);
    if (rc) return rc;
    if (!in_img || !out_img || !p) return fail(OG_EINVAL, "null buffer");
    if ((in_msk == nullptr) != (out_msk == nullptr)) return fail(OG_EINVAL, "in_msk and out_msk must both be given or both be NULL");
    OG_ALIGN(in_img);
    OG_ALIGN(out_img);
    OG_ALIGN(p);
    if ((rc = check_aug_params(*p, S, 0))) return rc;
    aug_stage_host(stage, in_img, in_msk, S, *p, out_img, out_msk);
    return OG_OK;
}

int og_aug_apply_host(const uint8_t* image, const uint8_t* mask, int S, const og_aug_params* p, int augment, float* out_img, float* out_msk) {
    int rc = check_aug_S(S);
    if (rc) return rc;
    if (!image || !mask || !out_img || !out_msk || (augment && !p)) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(out_img);
    OG_ALIGN(out_msk);
    OG_ALIGN(p);
    if (augment && (rc = check_aug_params(*p, S, 0))) return rc;
    const size_t P = (size_t)S * S;
    std::vector<float> a(P), b(P);
    std::vector<uint8_t> ma(P), mb(P);
    for (size_t i = 0; i < P; ++i) {
        a[i] = og_aug_unit(image[i]);
        ma[i] = mask[i] > 0 ? 1 : 0;
    }
    if (augment)
        for (int stage = 1; stage <= 7; ++stage) {
            aug_stage_host(stage, a.data(), ma.data(), S, *p, b.data(), mb.data());
            a.swap(b);
            ma.swap(mb);
        }
    for (size_t i = 0; i < P; ++i) {
        out_img[i] = a[i];
        out_msk[i] = ma[i] ? 1.0f : 0.0f;
    }
    return OG_OK;
}

int og_aug_noise_host(uint64_t key, size_t n, float* out) {
    if (n > 0 && !out) return fail(OG_EINVAL, "null buffer");
    OG_ALIGN(out);
    for (size_t i = 0; i < n; ++i) out[i] = og_aug_noise(key, i);
    return OG_OK;
}

#ifndef OG_PNG_HOST_ONLY
og_aug* og_aug_create(void) { return new og_aug(); }

void og_aug_destroy(og_aug* h) {
    og_stream_destroy(h, [h] { aug_free(h); });
}

int og_aug_sync(og_aug* h) { return og_stream_sync(h); }

int og_aug_set_chunk(og_aug* h, int chunk) { return og_stream_set_chunk(h, chunk, kAugMaxChunk); }

int og_aug_batch_u8_dev(og_aug* h, const uint8_t* images_dev, const uint8_t* masks_dev, int N, int S, const int32_t* idx_dev,
                        const og_aug_params* params, int b, int augment, float* out_img_dev, float* out_msk_dev) {
    if (!h) return fail(OG_EINVAL, "null handle");
    int rc = check_aug_S(S);
    if (rc) return rc;
    if (N < 1) return fail(OG_EINVAL, "N must be positive");
    if (b < 0) return fail(OG_EINVAL, "bad b");
    OG_ALIGN(idx_dev);
    OG_ALIGN(params);
    OG_ALIGN(out_img_dev);
    OG_ALIGN(out_msk_dev);
    if (b == 0) return OG_OK;
    if (!images_dev || !masks_dev || !idx_dev || !out_img_dev || !out_msk_dev || (augment && !params)) return fail(OG_EINVAL, "null buffer");
    if (augment)
        for (int i = 0; i < b; ++i)
            if ((rc = check_aug_params(params[i], S, i))) return rc;
    if ((rc = og_stream_ready(h))) return rc;
    OG_SCOPE(h);
    const int chunk = aug_chunk(h->chunk, S), cb = chunk < b ? chunk : b;
    const size_t P = (size_t)S * S, rec = sizeof(og_aug_params);
    if (augment) {
        if ((rc = h->d_ws.grow(h, (size_t)aug_ws_bytes(S, cb, 1), "aug"))) return rc;
        for (auto& s : h->slots) {
            if ((rc = s.h_par.grow(h, cb * rec, "aug"))) return rc;
            if (!s.ev) HIPCHK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
        }
    }
    // (a workspace that grew earlier for a larger micro-batch is laid out for THIS call's cb: the layout is a function of cb alone)
    auto run = [&]() -> int {
        for (int b0 = 0; b0 < b; b0 += chunk) {
            const int nb = (b - b0 < chunk) ? b - b0 : chunk;
            if (augment) {
                og_aug::Slot& s = h->slots[h->turn++ & 1];
                if (s.used) HIPCHK(hipEventSynchronize(s.ev));   // the slot's last copy has left it
                memcpy(s.h_par, params + b0, nb * rec);
                HIPCHK(hipMemcpyAsync(aug_ws_params(h->d_ws, S, cb), s.h_par, nb * rec, hipMemcpyHostToDevice, h->stream));
                HIPCHK(hipEventRecord(s.ev, h->stream));
                s.used = true;
            }
            const int rc2 = aug_batch(h->stream, h->d_ws, cb, images_dev, masks_dev, N, S, idx_dev + b0, nb, augment, out_img_dev + b0 * P, out_msk_dev + b0 * P);
            if (rc2) return rc2;
        }
        return OG_OK;
    };
    rc = run();
    if (rc) og_stream_drain(h);
    return rc;
}

int og_aug_plan(int b, int S, int chunk, int augment, char* out, size_t cap, long long* workspace_bytes) {
    if (!out || cap == 0 || b < 1) return fail(OG_EINVAL, "bad argument");
    int rc = check_aug_S(S);
    if (rc) return rc;
    if ((rc = og_check_chunk(chunk, kAugMaxChunk))) return rc;
    const int mb = aug_chunk(chunk, S), cb = mb < b ? mb : b;
    const long long P = (long long)S * S;
    if (workspace_bytes) *workspace_bytes = aug_ws_bytes(S, cb, augment);
    const uintptr_t gap = (uintptr_t)1 << 40;   // placeholder bases: nothing dereferences them in a dry run
    float* oi = (float*)(1 * gap);
    float* om = (float*)(2 * gap);
    Plan plan;
    plan.bases = {{"out_img", oi}, {"out_msk", om}};
    g_plan = &plan;
    for (int b0 = 0; b0 < b && !rc; b0 += mb) {
        const int nb = (b - b0 < mb) ? b - b0 : mb;
        rc = aug_batch(nullptr, (uint8_t*)(3 * gap), cb, (const uint8_t*)(4 * gap), (const uint8_t*)(5 * gap), 1, S, (const int32_t*)(6 * gap) + b0, nb,
                       augment, oi + b0 * P, om + b0 * P);
    }
    g_plan = nullptr;
    if (rc) return rc;
    return og_plan_text(plan, kPlanWrites, out, cap);
}
#endif   // OG_PNG_HOST_ONLY

}  // extern "C"
