// The host twin of the device PNG decoder under sanitizers: a stand-alone program around the host-only build of
// openglottal_amd/csrc/og_png.inc (the parser, og_png_zlib and the rest of the twin: the inline functions the kernels call).
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/png_host_fuzz.cpp -o png_host_fuzz
//       (g++: add -static-libasan -static-libubsan, clang++: -static-libsan, so that the runtimes are part of the program)
//   python tools/png_fuzz_corpus.py corpus.bin && ./png_host_fuzz corpus.bin
//
// corpus.bin: u32 count, then per case u32 length and the bytes (little endian).  Every case is copied into a heap block of exactly
// its length and decoded, at C = 3 and at C = 1, into a heap block of exactly H * W * C bytes; its joined zlib stream goes through
// og_pngd_inflate_host into a block of exactly H * (1 + rb) bytes.  So a read or a write one byte outside any of them is reported.
// Prints the number of cases per status; exit code 0 unless a case breaks the contract (an unknown status, bytes that are not 0
// behind a non-zero status, two channel counts that disagree on the status, or a sanitizer report).
#define OG_PNG_HOST_ONLY
#include "../openglottal_amd/csrc/og_png.inc"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s corpus.bin\n", argv[0]);
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
    long seen[kPngStatusMax + 1] = {0};
    std::vector<uint8_t> blob;
    std::vector<int64_t> offsets{0};
    for (uint32_t i = 0; i < count; ++i) {
        if (at + 4 > all.size()) return 2;
        const uint32_t len = u32(at);
        at += 4;
        if (at + len > all.size()) return 2;
        uint8_t* png = (uint8_t*)malloc(len ? len : 1);   // exactly its length (a zero-length case still needs an address)
        memcpy(png, all.data() + at, len);
        blob.insert(blob.end(), png, png + len);
        offsets.push_back((int64_t)blob.size());
        at += len;
        og_png_info info;
        if (og_pngd_parse_host(png, len, &info) != OG_OK) return 1;
        int status[2] = {-1, -1};
        for (int c = 0; c < 2; ++c) {
            const int C = c ? 1 : 3;
            const size_t need = info.status ? 1 : (size_t)info.H * info.W * C;
            uint8_t* out = (uint8_t*)malloc(need);
            if (og_pngd_decode_host(png, len, C, out, need, &status[c]) != OG_OK) return 1;
            bool dirty = false;
            if (status[c] != 0 && status[c] != 6)
                for (size_t k = 0; k < need; ++k) dirty |= out[k] != 0;
            free(out);
            if (status[c] < 0 || status[c] > kPngStatusMax || (info.status != 0) != (status[c] == 6) || dirty) {
                fprintf(stderr, "case %u: status %d after parser status %d%s\n", i, status[c], info.status, dirty ? ", bytes that are not 0" : "");
                return 1;
            }
        }
        if (status[0] != status[1]) {
            fprintf(stderr, "case %u: status %d at C = 3, %d at C = 1\n", i, status[0], status[1]);
            return 1;
        }
        if (!info.status) {   // the stream alone
            PngParsed p;
            png_parse(png, len, &p);
            const std::vector<uint8_t> z = png_join(png, p);
            uint8_t* zs = (uint8_t*)malloc(z.size() ? z.size() : 1);
            memcpy(zs, z.data(), z.size());
            uint8_t* raw = (uint8_t*)malloc((size_t)info.raw_bytes);
            size_t produced = 0;
            int st = -1;
            if (og_pngd_inflate_host(zs, z.size(), raw, (size_t)info.raw_bytes, &produced, &st) != OG_OK) return 1;
            if (st < 0 || st > 5 || produced > (size_t)info.raw_bytes) return 1;
            free(raw);
            free(zs);
        }
        ++seen[status[0]];
        free(png);
    }
    // the records of the whole corpus as one call, every buffer exactly sized
    const int B = (int)count;
    uint8_t* exact = (uint8_t*)malloc(blob.size() ? blob.size() : 1);
    memcpy(exact, blob.data(), blob.size());
    std::vector<og_png_rec> recs((size_t)B + 1);
    std::vector<int64_t> zoffsets((size_t)B + 1);
    uint8_t* zblob = (uint8_t*)malloc(blob.size() ? blob.size() : 1);
    uint8_t* pals = (uint8_t*)malloc((size_t)(B + 1) * 768);
    int npals = 0;
    int64_t totals[3] = {0, 0, 0};
    if (og_pngd_records_host(exact, offsets.data(), B, 3, recs.data(), zblob, blob.size(), zoffsets.data(), pals, B + 1, &npals, totals) != OG_OK) return 1;
    free(pals);
    free(zblob);
    free(exact);
    printf("%u cases, %d palettes, %lld pixel bytes; per status:", count, npals, (long long)totals[0]);
    for (int s = 0; s <= kPngStatusMax; ++s) printf(" %d:%ld", s, seen[s]);
    printf("\n");
    return 0;
}
