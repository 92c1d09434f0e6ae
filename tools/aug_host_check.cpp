// The host twin of the device augmentation under sanitizers: a stand-alone program around the host-only build of
// openglottal_amd/csrc/og_aug.inc (the per-pixel functions the kernels call and the stages composed of them), with og_png.inc before it
// for the host-only plumbing (fail, OG_ALIGN, og_last_error).
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/aug_host_check.cpp -o aug_host_check
//       (g++: add -static-libasan -static-libubsan, clang++: -static-libsan, so that the runtimes are part of the program)
//   python tools/aug_cases_corpus.py cases.bin && ./aug_host_check cases.bin
//
// cases.bin: u32 count, then per case u32 S, the 64 bytes of the og_aug_params record, S * S image bytes, S * S mask bytes (little
// endian).  Every buffer is a heap block of exactly its declared size -- the tiles S * S bytes, every f32 plane 4 * S * S, the record
// 64 -- so a read or a write one byte outside any of them is reported.  Per case: the whole chain (og_aug_apply_host), the seven
// stages one after the other (og_aug_stage_host) which must give the chain's bits, and the plain path.  Exit code 0 unless an entry
// fails, the two disagree, or a sanitizer reports.  The sum printed is that of the chain's image bits, for the caller to compare.
#define OG_PNG_HOST_ONLY
#include "../openglottal_amd/csrc/og_png.inc"
#include "../openglottal_amd/csrc/og_aug.inc"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    std::vector<uint8_t> all;
    uint8_t buf[1 << 16];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + n);
    fclose(f);
    auto u32 = [&all](size_t at) { return (uint32_t)all[at] | (uint32_t)all[at + 1] << 8 | (uint32_t)all[at + 2] << 16 | (uint32_t)all[at + 3] << 24; };
    if (all.size() < 4) return 2;
    const uint32_t count = u32(0);
    size_t at = 4;
    long long pixels = 0;
    unsigned long long sum = 0;
    for (uint32_t i = 0; i < count; ++i) {
        if (at + 4 + sizeof(og_aug_params) > all.size()) return 2;
        const int S = (int)u32(at);
        at += 4;
        og_aug_params* p = (og_aug_params*)malloc(sizeof(og_aug_params));
        memcpy(p, all.data() + at, sizeof(og_aug_params));
        at += sizeof(og_aug_params);
        if (S < 1 || S > kAugMaxS) return 2;
        const size_t P = (size_t)S * S;
        if (at + 2 * P > all.size()) return 2;
        uint8_t* image = (uint8_t*)malloc(P);
        uint8_t* mask = (uint8_t*)malloc(P);
        memcpy(image, all.data() + at, P);
        memcpy(mask, all.data() + at + P, P);
        at += 2 * P;
        float* oi = (float*)malloc(4 * P);
        float* om = (float*)malloc(4 * P);
        float* pi = (float*)malloc(4 * P);
        float* pm = (float*)malloc(4 * P);
        if (og_aug_apply_host(image, mask, S, p, 1, oi, om) != OG_OK || og_aug_apply_host(image, mask, S, nullptr, 0, pi, pm) != OG_OK) {
            fprintf(stderr, "case %u: %s\n", i, og_last_error());
            return 1;
        }
        float* a = (float*)malloc(4 * P);
        float* b = (float*)malloc(4 * P);
        uint8_t* ma = (uint8_t*)malloc(P);
        uint8_t* mb = (uint8_t*)malloc(P);
        for (size_t k = 0; k < P; ++k) {
            a[k] = (float)image[k] / 255.0f;
            ma[k] = mask[k] > 0 ? 1 : 0;
            if (pi[k] != a[k] || pm[k] != (float)ma[k]) {
                fprintf(stderr, "case %u: the plain path differs at pixel %zu\n", i, k);
                return 1;
            }
        }
        for (int stage = 1; stage <= 7; ++stage) {
            if (og_aug_stage_host(stage, a, ma, S, p, b, mb) != OG_OK) {
                fprintf(stderr, "case %u stage %d: %s\n", i, stage, og_last_error());
                return 1;
            }
            float* t = a;
            a = b;
            b = t;
            uint8_t* u = ma;
            ma = mb;
            mb = u;
        }
        for (size_t k = 0; k < P; ++k) {
            if (memcmp(&a[k], &oi[k], 4) != 0 || om[k] != (float)ma[k]) {
                fprintf(stderr, "case %u: the stages and the chain differ at pixel %zu\n", i, k);
                return 1;
            }
            uint32_t bits;
            memcpy(&bits, &oi[k], 4);
            sum += bits;
        }
        pixels += (long long)P;
        free(mb); free(ma); free(b); free(a); free(pm); free(pi); free(om); free(oi); free(mask); free(image); free(p);
    }
    // the refusals write nothing: blocks of one element are enough
    float* one = (float*)malloc(4);
    uint8_t* px = (uint8_t*)malloc(1);
    og_aug_params* bad = (og_aug_params*)calloc(1, sizeof(og_aug_params));
    bad->cos_t = 1.0f;
    bad->ks = 4;
    if (og_aug_apply_host(px, px, 7, bad, 1, one, one) != OG_EINVAL || og_aug_apply_host(px, px, 8, bad, 1, one, one) != OG_EINVAL ||
        og_aug_stage_host(9, one, px, 8, bad, one, px) != OG_EINVAL || og_aug_stage_host(5, one, px, 8, bad, one, px) != OG_EINVAL ||
        og_aug_noise_host(1, 1, nullptr) != OG_EINVAL || og_aug_noise_host(1, 1, one) != OG_OK)
        return 1;
    free(bad);
    free(px);
    free(one);
    printf("%u cases, %lld pixels, image bits sum %llu\n", count, pixels, sum);
    return 0;
}
