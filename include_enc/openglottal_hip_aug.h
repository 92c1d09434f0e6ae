/*
 * openglottal_hip_aug.h — crop-training batches AUGMENTED on the device (fourteenth header; the conventions of openglottal_hip.h --
 * return codes, og_last_error, *_dev entry points asynchronous on the handle's stream, device restore, a failed call leaves the handle
 * usable -- all hold, and the entries mirror the thirteenth header, openglottal_hip_pnge.h, which this one joins in include_enc/).
 * What `CroppedGlottisDataset._tensor_and_augment` (scripts/train_unet_crop.py:167-204; the same chain in openglottal/data.py:284-329)
 * does per sample on a DataLoader worker: the tiles of the crop cache stay resident as u8 [N,S,S], and one call turns a list of sample
 * indices into the augmented f32 [b,1,S,S] image and mask batch `model(imgs)` consumes, in device memory.
 *
 * THE RECORD.  Every sample has one og_aug_params, 64 bytes, that holds only numbers the HOST drew or computed; no transcendental
 * function runs on the device.  The stages run in this order on I = u8 / 255 (f32) and M = (u8 > 0):
 *   1 FLIP       bit 0 of `flips`: horizontal, bit 1: vertical; index reversal of I and M.
 *   2 ROTATE     always.  torch.nn.functional.grid_sample(padding_mode="zeros", align_corners=False) over torchvision's affine grid:
 *                output pixel (i, j) has X = j + 0.5 - S/2, Y = i + 0.5 - S/2 and reads the source index
 *                (cos_t * X - sin_t * Y + (S - 1)/2,  sin_t * X + cos_t * Y + (S - 1)/2), cos_t / sin_t the f32 of the f64 cosine and
 *                sine of radians(angle).  I: bilinear, a tap outside the image counts as 0.  M: nearest, round half to even, 0 outside.
 *   3 RESCALE    when new_size = int(S * scale) != 0.  I: antialiased bilinear (F.interpolate(mode="bilinear", align_corners=False,
 *                antialias=True)), separable, rows first: per output index c = (in/out)(i + 0.5), support sup = max(in/out, 1), taps
 *                k in [max(0, int(c - sup + 0.5)), min(in, int(c + sup + 0.5))), weight max(0, 1 - |(k - c + 0.5) * (1 / sup)|)
 *                divided by the taps' sum.  M: mode="nearest": src = min(int(floorf(dst * ((float)in / out))), in - 1).  Then, fused
 *                into the resize so that only the S x S window is computed: new_size > S takes the centre crop at
 *                off = (new_size - S) / 2; otherwise zeros are padded, pl = pad / 2 left and top, pad - pl right and bottom.
 *   4 NOISE      when noise_sigma != 0: clamp(I + n * noise_sigma, 0, 1), n = og_aug_noise(noise_key, pixel index y * S + x): a
 *                standard normal deviate from a counter-based generator (two rounds of a 64-bit mixer, Box-Muller with a logarithm
 *                and a cosine written out in integer operations, +, *, fmaf and the correctly rounded sqrt and division), one
 *                __host__ __device__ function: host and device agree bit for bit.
 *   5 BLUR       when ks is 3 or 5: reflect padding by ks / 2, then sum of (k1[y] * k1[x]) * tap, rows outer, columns inner, left to
 *                right.  k1: the host's f32 of torchvision's kernel, exp(-0.5 (x / sigma)^2) over linspace(-(ks-1)/2, (ks-1)/2, ks),
 *                divided by its sum.
 *   6 BRIGHTNESS when brightness != 0: clamp(I * brightness, 0, 1).
 *   7 CONTRAST   when contrast != 0: clamp(contrast * I + (1 - contrast) * mean, 0, 1).  mean = sum / (float)(S * S); the sum in ONE
 *                fixed order: blocks of og_aug_limit(6) = 1024 consecutive pixels (the last one filled with zeros); in a block lane t
 *                of 256 adds its pixels t, t + 256, t + 512, t + 768 in that order, then a tree, lane t += lane t + d for
 *                d = 128, 64, .., 1; the blocks' sums are then added in index order.
 * A stage that is off passes its input through unchanged, bit for bit.  All of the arithmetic is written without contraction (no fused
 * multiply-add except where fmaf is spelled out), so the twin (og_aug_*_host) and the kernels round alike.
 * With augment = 0 a call gives u8 / 255 and (u8 > 0) only: the validation loader.
 *
 * UNPINNED.  torchvision is not part of this project's build image: the torchvision-level rule (TF.rotate's matrix, TF.resize's
 * antialias default for tensors, TF.gaussian_blur's kernel, TF.adjust_contrast's blend) is restated from its sources as recalled, and
 * the antialias default in particular is unpinned.  The torch functionals the rule reduces to (grid_sample, interpolate, conv2d, pad)
 * ARE the tests' oracle.  The noise cannot equal torch.randn_like's stream: it has the distribution, not the numbers.
 * OUT OF SCOPE: the training loop and the loss (autograd, AdamW: PyTorch-ROCm's), multi-channel images, non-square tiles,
 * expand=True rotation, torch.randn's stream, torchvision parity beyond the torch functionals.
 *
 * LAUNCHES per micro-batch of nb = min(chunk, 256 MiB / per-sample workspace) samples, at most four:
 *   k_aug_rotate    a lane per pixel: gathers sample idx[b] from the resident tiles, the flips folded into the tap addresses; rotated
 *                   f32 I and u8 M into the workspace.  An index outside [0, N) reads nothing and gives an all-zero sample.
 *   k_aug_scale     a lane per pixel: resize with the crop or pad, noise; writes the final mask.
 *   k_aug_blur      a workgroup per block of 1024 pixels: blur, brightness, the block's sum.
 *   k_aug_contrast  a workgroup per block: joins the sums, applies the contrast, writes the final image.
 *   k_aug_plain     (augment = 0 only, the one launch of that mode) a lane per pixel.
 * Every tap is bounds-checked: zero or reflect padding is part of the rule, and no tap reads outside its tile.
 * LIMITS (og_aug_limit): 8 <= S <= 1024, chunk 1..1024, new_size 0 or ceil(S / 2)..2 S.
 * MEMORY: per sample of a micro-batch 9 S^2 bytes (two f32 planes, one u8), 4 bytes per block and the 64-byte record; it does not
 * grow with N or b.  Two pinned host slots of chunk records.
 *
 * ALIGNMENT: idx 4 bytes, params 8, the f32 outputs 4, u8 buffers any address.  A violation is OG_EINVAL before anything is launched,
 * copied or written.
 */
#ifndef OPENGLOTTAL_HIP_AUG_H
#define OPENGLOTTAL_HIP_AUG_H

#include "openglottal_hip_pnge.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct og_aug og_aug;

typedef struct og_aug_params {
    uint32_t flips;        /*  0: bit 0 horizontal, bit 1 vertical; no other bit */
    float cos_t;           /*  4: (float)cos(radians(angle)), the cosine in f64 */
    float sin_t;           /*  8: (float)sin(radians(angle)) */
    int32_t new_size;      /* 12: int(S * scale); 0: no rescale */
    float noise_sigma;     /* 16: 0: no noise */
    int32_t ks;            /* 20: 0 (no blur), 3 or 5 */
    uint64_t noise_key;    /* 24: the sample's noise stream */
    float k1[5];           /* 32: the 1-D blur weights, k1[0 .. ks) used */
    float brightness;      /* 52: the factor; 0: off */
    float contrast;        /* 56: the ratio; 0: off */
    uint32_t reserved;     /* 60: 0 */
} og_aug_params;           /* 64 bytes */

/* which: 0 smallest S, 1 largest S, 2 max chunk, 3 the default chunk, 4 the largest new_size / S (the smallest is ceil(S / 2)),
 * 5 sizeof(og_aug_params), 6 pixels per block of the contrast mean, 7 the most taps per axis of the resize; otherwise -1 */
long long og_aug_limit(int which);

/* Host only, no handle, no device: the same inline functions the kernels call.  Images are f32 [S,S], masks u8 [S,S] holding 0 or 1;
 * in and out must not overlap. */

/* One stage (1..7, see THE RECORD) on one sample's intermediates.  Stages 4..7 copy the mask; in_msk and out_msk may both be NULL. */
int og_aug_stage_host(int stage, const float* in_img, const uint8_t* in_msk, int S, const og_aug_params* p, float* out_img, uint8_t* out_msk);

/* The whole chain on one sample: image and mask u8 [S,S] -> f32 [S,S] each (the mask 0.0 or 1.0).  augment = 0: u8 / 255 and (u8 > 0)
 * only, and p may be NULL. */
int og_aug_apply_host(const uint8_t* image, const uint8_t* mask, int S, const og_aug_params* p, int augment, float* out_img, float* out_msk);

/* out[i] = the deviate of pixel index i of stream `key`, i < n. */
int og_aug_noise_host(uint64_t key, size_t n, float* out);

/* The device is the one current at the first call that touches it; the handle owns its stream and workspace.  chunk 128. */
og_aug* og_aug_create(void);
void og_aug_destroy(og_aug* h);
int og_aug_sync(og_aug* h);
int og_aug_set_chunk(og_aug* h, int chunk);

/* images_dev, masks_dev [N,S,S] u8 resident tiles; idx_dev [b] int32 on the device, repeated indices are legal; params [b] records in
 * HOST memory (ignored, and may be NULL, with augment = 0), every one checked against the limits before anything runs;
 * out_img_dev, out_msk_dev [b,1,S,S] f32.  b = 0 is a no-op.  Asynchronous on the handle's stream; params may be reused on return. */
int og_aug_batch_u8_dev(og_aug* h, const uint8_t* images_dev, const uint8_t* masks_dev, int N, int S, const int32_t* idx_dev,
                        const og_aug_params* params, int b, int augment, float* out_img_dev, float* out_msk_dev);

/* Dry run of og_aug_batch_u8_dev without a device: one line per launch in the columns of og_pnge_plan,
 * kernel|gx|gy|gz|block|lds|workspace|counters|writes ("out_img=END;out_msk=END" or "-").  Returns the number of launches;
 * *workspace_bytes = the device workspace of the call. */
int og_aug_plan(int b, int S, int chunk, int augment, char* out, size_t cap, long long* workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
