// Stand-alone driver for the host half of the JPEG output path (fastmot_amd/csrc/jpegenc_host.hip), meant to be built with
// the host sanitizers and run on the CPU -- no GPU, no Python:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -c fastmot_amd/csrc/jpegenc_host.hip -o /tmp/jeh.o
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -c -x hip scripts/jpegenc_host_check.cpp -o /tmp/jec.o
//   /opt/rocm/llvm/bin/clang++ -fsanitize=address,undefined /tmp/jeh.o /tmp/jec.o -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib \
//         -o /tmp/jpegenc_host_check && /tmp/jpegenc_host_check
//
// (the sanitizers instrument host code only: -Xarch_host when compiling, a plain host link)
//
// It walks the inputs of tests/test_jpegenc_host.py: every quality and a spread of sizes through the table, header and
// bound functions; headers and whole files into buffers of EVERY capacity from 0 to the needed length, allocated at
// exactly that size so that a store past the capacity is a heap overflow the sanitizer reports; segment lists whose
// lengths do not fit the segment buffer; bad arguments.  Exit status 0 and "ok" when every call returned what it should.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/fastmot_hip.h"

void fm_set_error(const char*, ...) {}      // (ctx.hip's, which the library links)

#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            fprintf(stderr, "%s:%d failed: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                \
        }                                                            \
    } while (0)

int main() {
    const int sizes[][2] = {{1, 1}, {9, 17}, {16, 16}, {31, 33}, {48, 32}, {70, 130}, {1920, 1080}, {16384, 16384}};
    uint16_t qt[128];
    for (int q = -2; q <= 103; ++q) {
        const int rc = fm_jpeg_encode_tables(q, qt);
        CHECK((rc == 0) == (q >= 1 && q <= 100));
        if (!rc)
            for (int i = 0; i < 128; ++i) CHECK(qt[i] >= 1 && qt[i] <= 255);
    }
    CHECK(fm_jpeg_encode_tables(75, nullptr) != 0);
    uint32_t rng = 12345;
    for (auto& s : sizes) {
        const int w = s[0], h = s[1], rows = (h + 15) / 16;
        const size_t bound = fm_jpeg_encode_bound(w, h);
        CHECK(bound > 0);
        size_t need = 0;
        {
            std::vector<uint8_t> big(1024);
            CHECK(fm_jpeg_encode_header(w, h, 75, big.data(), big.size(), &need) == 0 && need > 0 && need <= big.size());
        }
        for (size_t cap = 0; cap <= need; ++cap) {          // a buffer of exactly `cap` bytes
            uint8_t* buf = (uint8_t*)malloc(cap ? cap : 1);
            size_t n = 0;
            const int rc = fm_jpeg_encode_header(w, h, 75, buf, cap, &n);
            CHECK(n == need && (rc == 0) == (cap == need));
            free(buf);
        }
        if (rows > 1100) continue;
        // segments of random lengths and bytes, 16-aligned one behind the other
        std::vector<uint32_t> lens(rows);
        size_t total = 0, sum = 0;
        for (int r = 0; r < rows; ++r) {
            rng = rng * 1664525u + 1013904223u;
            lens[r] = (rng >> 8) % 200;
            total += (lens[r] + 15) & ~15u;
            sum += lens[r];
        }
        std::vector<uint8_t> segs(total ? total : 1, 0xA5);
        const size_t file = need + sum + 2 * (size_t)(rows - 1) + 2;
        for (size_t cap : {(size_t)0, need, file - 1, file, file + 7}) {
            uint8_t* buf = (uint8_t*)malloc(cap ? cap : 1);
            size_t n = 0;
            const int rc = fm_jpeg_encode_assemble(w, h, 75, lens.data(), segs.data(), total, buf, cap, &n);
            CHECK(n == file && (rc == 0) == (cap >= file));
            if (!rc) CHECK(buf[0] == 0xFF && buf[1] == 0xD8 && buf[file - 2] == 0xFF && buf[file - 1] == 0xD9);
            free(buf);
        }
        // lengths that run past the segment buffer: refused, nothing read
        if (total >= 16) {
            std::vector<uint8_t> out(file);
            size_t n = 0;
            lens[0] = 0xFFFFFFF0u;
            CHECK(fm_jpeg_encode_assemble(w, h, 75, lens.data(), segs.data(), total, out.data(), out.size(), &n) != 0);
        }
    }
    size_t n = 0;
    uint8_t small[8];
    CHECK(fm_jpeg_encode_bound(0, 5) == 0 && fm_jpeg_encode_bound(5, 16385) == 0);
    CHECK(fm_jpeg_encode_header(0, 5, 75, small, sizeof small, &n) != 0);
    CHECK(fm_jpeg_encode_header(5, 5, 0, small, sizeof small, &n) != 0);
    CHECK(fm_jpeg_encode_header(5, 5, 101, small, sizeof small, &n) != 0);
    CHECK(fm_jpeg_encode_header(5, 5, 75, nullptr, 0, &n) != 0);
    puts("ok");
    return 0;
}
