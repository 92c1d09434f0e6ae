// The host twin of the device PNG encoder under sanitizers: a stand-alone program around the host-only build of
// openglottal_amd/csrc/og_pnge.inc (the filter, the run tokens, the code construction, the block and file writers: the inline
// functions the kernels call), with og_png.inc before it for the decoder that judges the result.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/pnge_host_check.cpp -o pnge_host_check
//       (g++: add -static-libasan -static-libubsan, clang++: -static-libsan, so that the runtimes are part of the program)
//   python tools/pnge_cases_corpus.py cases.bin && ./pnge_host_check cases.bin
//
// cases.bin: u32 count, then per case u32 H, W, C, S and the H * W * C bytes of the frame (little endian).  Every frame is copied into a
// heap block of exactly its size; the raw stream goes into a block of exactly H * (1 + W * C) bytes, its zlib stream into one of exactly
// 6 + N + 5 * nseg bytes, the file into one of exactly og_pnge_bound bytes.  So a read or a write one byte outside any of them is
// reported.  The file is then decoded by og_pngd_decode_host and the stream inflated by og_pngd_inflate_host, both into exact blocks.
// Exit code 0 unless an entry fails, the pixels or the raw bytes do not come back, a size passes its bound, or a sanitizer reports.
#define OG_PNG_HOST_ONLY
#include "../openglottal_amd/csrc/og_png.inc"
#include "../openglottal_amd/csrc/og_pnge.inc"

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
    long long file_bytes = 0, raw_bytes = 0, stored = 0;
    for (uint32_t i = 0; i < count; ++i) {
        if (at + 16 > all.size()) return 2;
        const int H = (int)u32(at), W = (int)u32(at + 4), C = (int)u32(at + 8), S = (int)u32(at + 12);
        at += 16;
        const long long bound = og_pnge_bound(H, W, C, S);
        if (bound < 0) {
            fprintf(stderr, "case %u: %s\n", i, og_last_error());
            return 1;
        }
        const size_t px = (size_t)H * W * C, N = (size_t)H * (1 + (size_t)W * C), zb = 6 + N + 5 * ((N + S - 1) / S);
        if (at + px > all.size()) return 2;
        uint8_t* frame = (uint8_t*)malloc(px);
        memcpy(frame, all.data() + at, px);
        at += px;
        uint8_t* raw = (uint8_t*)malloc(N);
        uint8_t* z = (uint8_t*)malloc(zb);
        uint8_t* png = (uint8_t*)malloc((size_t)bound);
        size_t zn = 0;
        int size = 0;
        if (og_pnge_filter_host(frame, H, W, C, raw, N) != OG_OK || og_pnge_deflate_host(raw, N, S, z, zb, &zn) != OG_OK ||
            og_pnge_encode_host(frame, H, W, C, S, png, (size_t)bound, &size) != OG_OK) {
            fprintf(stderr, "case %u: %s\n", i, og_last_error());
            return 1;
        }
        if (zn > zb || size > bound || (size_t)size != kPngeFixed + zn || memcmp(png + kPngeBefore - 2, z, zn) != 0) {
            fprintf(stderr, "case %u: sizes %zu (bound %zu) and %d (bound %lld), or the file does not hold the stream\n", i, zn, zb, size, bound);
            return 1;
        }
        uint8_t* exact = (uint8_t*)malloc((size_t)size);   // the decoder reads the file from a block of exactly its size
        memcpy(exact, png, (size_t)size);
        uint8_t* back = (uint8_t*)malloc(px);
        uint8_t* raw2 = (uint8_t*)malloc(N);
        int st = -1, st2 = -1;
        size_t produced = 0;
        if (og_pngd_decode_host(exact, (size_t)size, C, back, px, &st) != OG_OK || og_pngd_inflate_host(z, zn, raw2, N, &produced, &st2) != OG_OK) {
            fprintf(stderr, "case %u: %s\n", i, og_last_error());
            return 1;
        }
        if (st != 0 || st2 != 0 || produced != N || memcmp(back, frame, px) != 0 || memcmp(raw2, raw, N) != 0) {
            fprintf(stderr, "case %u: status %d / %d, %zu of %zu raw bytes, or other bytes came back\n", i, st, st2, produced, N);
            return 1;
        }
        if ((size_t)size == (size_t)bound) ++stored;
        file_bytes += size;
        raw_bytes += (long long)N;
        free(raw2);
        free(back);
        free(exact);
        free(png);
        free(z);
        free(raw);
        free(frame);
    }
    // the refusals write nothing: a block of one byte is enough
    uint8_t* one = (uint8_t*)malloc(1);
    uint8_t px4[4] = {1, 2, 3, 4};
    int size = 0;
    size_t zn = 0;
    if (og_pnge_encode_host(px4, 2, 2, 1, 64, one, 1, &size) != OG_EINVAL || og_pnge_filter_host(px4, 2, 2, 1, one, 1) != OG_EINVAL ||
        og_pnge_deflate_host(px4, 4, 64, one, 1, &zn) != OG_EINVAL || og_pnge_bound(2, 2, 2, 64) != -1 || og_pnge_bound(2, 2, 1, 96) != -1)
        return 1;
    free(one);
    printf("%u cases, %lld raw bytes, %lld file bytes, %lld files at their bound\n", count, raw_bytes, file_bytes, stored);
    return 0;
}
