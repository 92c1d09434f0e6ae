// The split entropy decoder's host twin under sanitizers: a stand-alone program around the host-only build of
// openglottal_amd/csrc/og_mjpd.inc and og_mjps.inc (the inline functions k_mjps_entropy calls, the lanes walked in a loop).
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/mjps_host_fuzz.cpp -o mjps_host_fuzz
//       (g++: add -static-libasan -static-libubsan, clang++: -static-libsan, so that the runtimes are part of the program)
//   python tools/mjps_fuzz_corpus.py corpus.bin && ./mjps_host_fuzz corpus.bin
//
// corpus.bin: u32 count, then per case u32 length and the bytes (little endian).  Every case is copied into a heap block of exactly
// its length and decoded into heap blocks of exactly H * W * 3 bytes, by og_jpegd_decode_host and by og_jpegs_decode_host at
// (sub, lanes) = (4, 2) and (4, 256): a read or a write one byte outside either is reported, and so is a status or a byte in which
// the split twin leaves the sequential one.  Prints the cases per status; exit code 0 unless a case breaks that contract.
#define OG_MJPD_HOST_ONLY
#include "../openglottal_amd/csrc/og_mjpd.inc"
#include "../openglottal_amd/csrc/og_mjps.inc"

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
    long long lanes = 0, windows = 0, decodes = 0;
    int rounds = 0;
    const int pairs[2][2] = {{4, 2}, {4, 256}};
    for (uint32_t i = 0; i < count; ++i) {
        if (at + 4 > all.size()) return 2;
        const uint32_t len = u32(at);
        at += 4;
        if (at + len > all.size()) return 2;
        uint8_t* jpeg = (uint8_t*)malloc(len ? len : 1);   // exactly its length (a zero-length case still needs an address)
        memcpy(jpeg, all.data() + at, len);
        at += len;
        og_jpegd_info info;
        if (og_jpegd_parse_host(jpeg, len, &info) != OG_OK) return 1;
        const size_t need = info.status ? 1 : (size_t)info.H * info.W * 3;
        uint8_t* want = (uint8_t*)malloc(need);
        int status = -1;
        if (og_jpegd_decode_host(jpeg, len, want, need, &status) != OG_OK) return 1;
        for (auto& pr : pairs) {
            uint8_t* out = (uint8_t*)malloc(need);
            int st = -1;
            int32_t stats[4];
            if (og_jpegs_decode_host(jpeg, len, pr[0], pr[1], out, need, &st, stats) != OG_OK) return 1;
            if (st != status || (status != 6 && memcmp(out, want, need) != 0)) {
                fprintf(stderr, "case %u at sub %d, %d lanes: status %d, the sequential twin's %d%s\n", i, pr[0], pr[1], st, status,
                        st == status ? ", other bytes" : "");
                return 1;
            }
            if (stats[2] > pr[1]) {
                fprintf(stderr, "case %u: %d rounds with %d lanes per window\n", i, stats[2], pr[1]);
                return 1;
            }
            lanes += stats[0];
            windows += stats[1];
            rounds = std::max(rounds, (int)stats[2]);
            decodes += stats[3];
            free(out);
        }
        if (status < 0 || status > kMjpdStatusMax) return 1;
        ++seen[status];
        free(want);
        free(jpeg);
    }
    printf("%u cases; lanes %lld windows %lld most rounds %d decodes %lld; per status:", count, lanes, windows, rounds, decodes);
    for (int s = 0; s <= kMjpdStatusMax; ++s) printf(" %d:%ld", s, seen[s]);
    printf("\n");
    return 0;
}
