// The host twin of the device JPEG decoder under sanitizers: a stand-alone program around the host-only build of
// openglottal_amd/csrc/og_mjpd.inc (the parser, og_jpegd_interval and the rest of the twin: the inline functions the kernels call).
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/mjpd_host_fuzz.cpp -o mjpd_host_fuzz
//       (g++: add -static-libasan -static-libubsan, clang++: -static-libsan, so that the runtimes are part of the program)
//   python tools/mjpd_fuzz_corpus.py corpus.bin && ./mjpd_host_fuzz corpus.bin
//
// corpus.bin: u32 count, then per case u32 length and the bytes (little endian).  Every case is copied into a heap block of exactly
// its length and decoded into a heap block of exactly H * W * 3 bytes, so a read or a write one byte outside either is reported.
// Prints the number of cases per status; exit code 0 unless a case breaks the contract (an unknown status, or a sanitizer report).
#define OG_MJPD_HOST_ONLY
#include "../openglottal_amd/csrc/og_mjpd.inc"

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
    long seen[kMjpdStatusMax + 1] = {0};
    std::vector<uint8_t> blob;
    std::vector<int64_t> offsets{0};
    for (uint32_t i = 0; i < count; ++i) {
        if (at + 4 > all.size()) return 2;
        const uint32_t len = u32(at);
        at += 4;
        if (at + len > all.size()) return 2;
        uint8_t* jpeg = (uint8_t*)malloc(len ? len : 1);   // exactly its length (a zero-length case still needs an address)
        memcpy(jpeg, all.data() + at, len);
        blob.insert(blob.end(), jpeg, jpeg + len);
        offsets.push_back((int64_t)blob.size());
        at += len;
        og_jpegd_info info;
        if (og_jpegd_parse_host(jpeg, len, &info) != OG_OK) return 1;
        int status = -1;
        const size_t need = info.status ? 1 : (size_t)info.H * info.W * 3;
        uint8_t* out = (uint8_t*)malloc(need);
        if (og_jpegd_decode_host(jpeg, len, out, need, &status) != OG_OK) return 1;
        if (status < 0 || status > kMjpdStatusMax || (info.status != 0) != (status == 6)) {
            fprintf(stderr, "case %u: status %d after parser status %d\n", i, status, info.status);
            return 1;
        }
        ++seen[status];
        free(out);
        free(jpeg);
    }
    // the records of the whole corpus as one call, the blob again exactly sized
    const int B = (int)count;
    uint8_t* exact = (uint8_t*)malloc(blob.size() ? blob.size() : 1);
    memcpy(exact, blob.data(), blob.size());
    std::vector<og_mjpd_rec> recs((size_t)B + 1);
    std::vector<uint32_t> tabs((size_t)(B + 1) * sizeof(MjpdTab) / 4);
    int nsets = 0, H = 0, W = 0, sampling = 0, Ri = 0;
    if (og_jpegd_records_host(exact, offsets.data(), B, recs.data(), (uint8_t*)tabs.data(), B + 1, &nsets, &H, &W, &sampling, &Ri) != OG_OK) return 1;
    free(exact);
    printf("%u cases, %d table sets, form %dx%d sampling %d Ri %d; per status:", count, nsets, H, W, sampling, Ri);
    for (int s = 0; s <= kMjpdStatusMax; ++s) printf(" %d:%ld", s, seen[s]);
    printf("\n");
    return 0;
}
