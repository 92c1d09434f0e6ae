// Host-only check of the grid.z layout (og_zlayout) and its inverse (og_zdecode), the pair every conv kernel's blockIdx.z goes
// through.  Includes only og_kernels.hpp; no GPU, no HIP call.  tests/test_zdecode.py builds it for the host with
// -fsanitize=address,undefined and runs it:
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/zdecode_check.hip -o zdecode_check && ./zdecode_check
// 1. quotient: for every gz in 1..65535 and every bz < 65535, og_zdecode's frame-group quotient equals bz / gz (zgroup_shift 0,
//    zdiv = gz: then b is the quotient and zr the remainder);
// 2. layouts: over the parameter grid of the launchers (frames, zdiv, grid_tiles, xcd_group, wgs), every combination whose gz fits
//    the hardware's 65535: og_zlayout equals the launch layer's rule restated below as plain integer code, and decoding every
//    bz < gz / wgs hits every (frame < frames, zr < zdiv) exactly once, with b >= frames in the last frame group only; for the
//    ungrouped forms (wgs > 0) og_zdecode<false> gives the same pair.
#include "../openglottal_amd/csrc/og_kernels.hpp"

#include <cstdio>
#include <vector>

static int n_fail = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (n_fail++ < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                 \
    } while (0)

int main() {
    long long n_q = 0, n_layouts = 0, n_decoded = 0;
    for (int gz = 1; gz <= 65535; ++gz) {
        ConvArgs a{};
        a.zdiv = gz;
        a.zgroup_shift = 0;
        a.zrcp = 1.0f / (float)gz;
        for (int bz = 0, q = 0, r = 0; bz < 65535; ++bz) {   // q = bz / gz, r = bz % gz, counted up: the check itself divides nothing
            int zr, b;
            og_zdecode(a, bz, zr, b);
            if (b != q || zr != r) CHECK(false, "gz %d bz %d -> b %d zr %d, expected %d %d", gz, bz, b, zr, q, r);
            if (++r == gz) { r = 0; ++q; }
        }
        n_q += 65535;
    }

    std::vector<int> frames_set, zdiv_set;
    for (int f = 1; f <= 40; ++f) frames_set.push_back(f);
    for (int f : {63, 64, 65, 255, 256, 1000, 4096}) frames_set.push_back(f);
    for (int z = 1; z <= 36; ++z) zdiv_set.push_back(z);
    for (int z : {64, 72, 128, 144}) zdiv_set.push_back(z);
    std::vector<unsigned char> seen;
    for (int frames : frames_set)
        for (int zdiv : zdiv_set)
            for (int grid_tiles : {1, 2, 3, 4, 6, 8, 12})
                for (int xcd_group = 0; xcd_group < 2; ++xcd_group)
                    for (int wgs : {0, 1, 4, 8, 16}) {
                        // the launch layer's rule as it stood before og_zlayout, in plain integer code
                        int shift = 0;
                        if (wgs == 0 && xcd_group && zdiv > 1) {
                            int txy = grid_tiles, g = 8;
                            while (g > 1 && txy % 2 == 0) { txy /= 2; g /= 2; }
                            while (g > frames) g /= 2;
                            while ((1 << shift) < g) ++shift;
                        }
                        const int G = 1 << shift, groups = (frames + G - 1) / G;
                        const float zrcp = 1.0f / (float)(zdiv * G);
                        const long long gz = (long long)groups * G * zdiv * (wgs ? wgs : 1);
                        const og_zlay l = og_zlayout(frames, zdiv, grid_tiles, xcd_group != 0, wgs);
                        CHECK(l.zgroup_shift == shift && l.zrcp == zrcp && l.gz == gz, "layout frames %d zdiv %d tiles %d xcd %d wgs %d", frames, zdiv,
                              grid_tiles, xcd_group, wgs);
                        if (gz > 65535) continue;
                        ++n_layouts;
                        ConvArgs a{};
                        a.zdiv = zdiv;
                        a.frames = frames;
                        a.zgroup_shift = l.zgroup_shift;
                        a.zrcp = l.zrcp;
                        const int nz = (int)(l.gz / (wgs ? wgs : 1));   // the `wgs` forms peel their workgroup index off first
                        seen.assign((size_t)frames * zdiv, 0);
                        for (int bz = 0; bz < nz; ++bz) {
                            int zr, b;
                            og_zdecode(a, bz, zr, b);
                            ++n_decoded;
                            if (wgs) {   // the ungrouped forms may skip the shifts
                                int zr0, b0;
                                og_zdecode<false>(a, bz, zr0, b0);
                                CHECK(zr0 == zr && b0 == b, "og_zdecode<false>: frames %d zdiv %d wgs %d bz %d", frames, zdiv, wgs, bz);
                            }
                            CHECK(zr >= 0 && zr < zdiv && b >= 0, "range: frames %d zdiv %d shift %d bz %d -> b %d zr %d", frames, zdiv, shift, bz, b, zr);
                            if (zr < 0 || zr >= zdiv || b < 0) continue;
                            if (b >= frames) {
                                CHECK(b < groups * G && b / G == groups - 1, "tail outside the last group: frames %d shift %d bz %d b %d", frames, shift, bz, b);
                                continue;
                            }
                            CHECK(seen[(size_t)b * zdiv + zr]++ == 0, "hit twice: frames %d zdiv %d shift %d bz %d", frames, zdiv, shift, bz);
                        }
                        for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == 1, "not hit: frames %d zdiv %d shift %d item %zu", frames, zdiv, shift, i);
                    }
    std::printf("zdecode_check: %lld quotients, %lld layouts, %lld decodes, %d failures\n", n_q, n_layouts, n_decoded, n_fail);
    return n_fail ? 1 : 0;
}
