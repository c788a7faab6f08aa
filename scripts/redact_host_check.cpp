// Stand-alone driver for the context-free half of the redaction path (fastmot_amd/csrc/redact_host.hip with
// redact_pixel.h: fm_redact_check and fm_redact_render_host), meant to be built with the host sanitizers and run on the
// CPU -- no GPU, no Python:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -c fastmot_amd/csrc/redact_host.hip -o /tmp/rdh.o
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -c -x hip scripts/redact_host_check.cpp -o /tmp/rdc.o
//   /opt/rocm/llvm/bin/clang++ -fsanitize=address,undefined /tmp/rdh.o /tmp/rdc.o -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib \
//         -o /tmp/redact_host_check && /tmp/redact_host_check
//
// Frames are heap blocks of exactly their size, so a load or store past them is a heap overflow the sanitizer reports,
// as is a read past the means of a region.  Valid lists of every mode and shape at frame sizes down to 1 x 1, regions
// inside, across and far outside the frame, with sides and coordinates at the limits and cells of 2 and 256; hostile
// lists, which must be refused with the frame untouched; n = 0.  Exit status 0 and "ok" when every call returned what it should.
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

static uint32_t rng_state = 2025;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }
static int between(int lo, int hi) { return lo + (int)((rnd() >> 8) % (uint32_t)(hi - lo + 1)); }

static fm_redact_region make(int x0, int y0, int x1, int y1, int mode, int shape, int cell) {
    fm_redact_region r;
    memset(&r, 0, sizeof r);
    r.x0 = x0, r.y0 = y0, r.x1 = x1, r.y1 = y1, r.mode = mode, r.shape = shape, r.cell = cell;
    r.b = (uint8_t)rnd(), r.g = (uint8_t)rnd(), r.r = (uint8_t)rnd();
    return r;
}

int main() {
    const int LIM = FM_OVERLAY_MAX_COORD, DIM = FM_SRC_MAX_DIM;
    const int sizes[][2] = {{1, 1}, {1, 37}, {37, 1}, {2, 3}, {37, 23}, {130, 50}};
    for (auto& s : sizes) {
        const int w = s[0], h = s[1];
        const size_t pitch = (size_t)w * 3, bytes = pitch * h;
        uint8_t* frame = (uint8_t*)malloc(bytes);
        uint8_t* copy = (uint8_t*)malloc(bytes);
        for (size_t i = 0; i < bytes; ++i) frame[i] = (uint8_t)rnd();

        // ---- valid lists
        std::vector<fm_redact_region> list;
        for (int i = 0; i < 300; ++i) {
            const int span = i % 3 == 0 ? 2 * (w + h) : (i % 3 == 1 ? 6 : 4000);
            const int x0 = between(-span, span + w), y0 = between(-span, span + h);
            const int cell = i % 7 == 0 ? 2 : (i % 7 == 1 ? 256 : between(2, 40));
            list.push_back(make(x0, y0, x0 + between(-2, span + w), y0 + between(-2, span + h), i % 3, (i / 3) % 2, cell));
        }
        for (int mode = 0; mode < 3; ++mode)
            for (int shape = 0; shape < 2; ++shape) {
                list.push_back(make(-DIM / 2, -DIM / 2, DIM / 2 - 1, DIM / 2 - 1, mode, shape, 256));     // the largest side, around the frame
                list.push_back(make(-LIM, -LIM, -LIM + DIM - 1, -LIM + DIM - 1, mode, shape, 2));          // far outside
                list.push_back(make(LIM - DIM + 1, LIM - DIM + 1, LIM, LIM, mode, shape, 3));
                list.push_back(make(w - 1, h - 1, w - 1, h - 1, mode, shape, 2));                         // the last pixel
                list.push_back(make(w - 1 - DIM + 1, h - 1 - DIM + 1, w - 1, h - 1, mode, shape, 255));   // anchored far up left
                list.push_back(make(LIM, LIM, -LIM, -LIM, mode, shape, 2));                                // empty
            }
        CHECK(fm_redact_check(list.data(), (int)list.size(), w, h) == 0);
        CHECK(fm_redact_render_host(frame, w, h, pitch, list.data(), (int)list.size()) == 0);
        // n = 0 with and without a pointer
        memcpy(copy, frame, bytes);
        CHECK(fm_redact_render_host(frame, w, h, pitch, nullptr, 0) == 0);
        CHECK(fm_redact_render_host(frame, w, h, pitch, list.data(), 0) == 0);
        CHECK(memcmp(copy, frame, bytes) == 0);

        // ---- hostile lists: refused, nothing written
        std::vector<fm_redact_region> bad = {
            make(0, 0, 5, 5, 3, 0, 4), make(0, 0, 5, 5, -1, 0, 4), make(0, 0, 5, 5, 0, 2, 4), make(0, 0, 5, 5, 0, -1, 4),
            make(0, 0, 5, 5, 0, 0, 1), make(0, 0, 5, 5, 0, 0, 257), make(0, 0, 5, 5, 2, 0, 0), make(0, 0, 5, 5, 0, 0, INT32_MIN),
            make(LIM + 1, 0, LIM + 1, 0, 0, 0, 4), make(0, -LIM - 1, 0, 0, 0, 0, 4), make(0, 0, INT32_MAX, 0, 0, 0, 4),
            make(INT32_MIN, 0, 0, 0, 0, 0, 4), make(0, 0, 0, INT32_MIN, 0, 0, 4), make(-1, 0, DIM - 1, 5, 0, 0, 4),
            make(0, -1, 5, DIM - 1, 2, 1, 4), make(INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX, 0, 1, 2)};
        fm_redact_region res = make(0, 0, 5, 5, 0, 0, 4);
        res.reserved = 1;
        bad.push_back(res);
        for (const fm_redact_region& b : bad) {
            std::vector<fm_redact_region> l = {make(0, 0, w, h, FM_REDACT_FILL, 0, 2), b};
            CHECK(fm_redact_check(l.data(), 2, w, h) != 0);
            CHECK(fm_redact_render_host(frame, w, h, pitch, l.data(), 2) != 0);
            CHECK(memcmp(copy, frame, bytes) == 0);
        }
        fm_redact_region one = make(0, 0, 5, 5, 0, 0, 4);
        CHECK(fm_redact_check(nullptr, 1, w, h) != 0);
        CHECK(fm_redact_check(&one, -1, w, h) != 0);
        CHECK(fm_redact_check(&one, FM_REDACT_MAX_REGIONS + 1, w, h) != 0);       // (refused before it is read)
        CHECK(fm_redact_check(&one, 1, 0, h) != 0 && fm_redact_check(&one, 1, w, DIM + 1) != 0);
        CHECK(fm_redact_render_host(nullptr, w, h, pitch, &one, 1) != 0);
        CHECK(fm_redact_render_host(frame, w, h, pitch - 1, &one, 1) != 0);
        CHECK(memcmp(copy, frame, bytes) == 0);
        free(frame), free(copy);
    }
    // the cap on the cells of a list depends on the frame: 2048 x 1024 cells on a frame that holds them, few on a small one
    {
        fm_redact_region big = make(0, 0, 4095, 2047, FM_REDACT_PIXELATE, 0, 2);
        CHECK(fm_redact_check(&big, 1, 4096, 2048) != 0 && fm_redact_check(&big, 1, 64, 64) == 0);
        big.mode = FM_REDACT_FILL;
        CHECK(fm_redact_check(&big, 1, 4096, 2048) == 0);
    }
    // a padded frame: the bytes between the rows stay as they are
    {
        const int w = 5, h = 4;
        const size_t pitch = 24;
        std::vector<uint8_t> frame(pitch * h, 0x5A);
        fm_redact_region r = make(-3, -3, 50, 50, FM_REDACT_FILL, 0, 2);
        r.b = r.g = r.r = 1;
        CHECK(fm_redact_render_host(frame.data(), w, h, pitch, &r, 1) == 0);
        for (int y = 0; y < h; ++y)
            for (size_t i = 0; i < pitch; ++i) CHECK(frame[y * pitch + i] == (i < (size_t)w * 3 ? 1 : 0x5A));
    }
    puts("ok");
    return 0;
}
