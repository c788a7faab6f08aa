// Stand-alone driver for the context-free half of the object-crop encoder (fastmot_amd/csrc/jpegenc_host.hip:
// fm_jpeg_encode_regions_plan / _bound / _assemble), meant to be built with the host sanitizers and run on the CPU -- no
// GPU, no Python:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -c fastmot_amd/csrc/jpegenc_host.hip -o /tmp/jeh.o
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -c -x hip scripts/objenc_host_check.cpp -o /tmp/oec.o
//   /opt/rocm/llvm/bin/clang++ -fsanitize=address,undefined /tmp/jeh.o /tmp/oec.o -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib \
//         -o /tmp/objenc_host_check && /tmp/objenc_host_check
//
// Segment lengths reach the assembler from device memory, so it is driven here with hostile ones: every buffer is a heap
// block of exactly its size, a read past the segments or a write past the output is a heap overflow the sanitizer
// reports.  Random lists at the limits, random and hostile lengths, capacities from 0 to the bound.  Exit status 0 and
// "ok" when every call returned what it should.
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

static uint32_t rng_state = 2026;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }
static int between(int lo, int hi) { return lo + (int)((rnd() >> 8) % (uint32_t)(hi - lo + 1)); }

int main() {
    fm_crop_totals tot;
    // refusals of the plan
    fm_crop_rect one = {0, 0, 15, 15};
    CHECK(fm_jpeg_encode_regions_plan(&one, -1, 1, nullptr, &tot) != 0);
    CHECK(fm_jpeg_encode_regions_plan(nullptr, 1, 1, nullptr, &tot) != 0);
    CHECK(fm_jpeg_encode_regions_plan(&one, 1, 3, nullptr, &tot) != 0);
    CHECK(fm_jpeg_encode_regions_plan(&one, 1, 1, nullptr, nullptr) != 0);
    CHECK(fm_jpeg_encode_regions_plan(nullptr, 0, 1, nullptr, &tot) == 0 && tot.rows == 0 && tot.bound == 0);
    fm_crop_rect bad[] = {{5, 0, 4, 3}, {0, 5, 3, 4}, {-1, 0, 3, 3}, {0, 0, 16384, 3}, {0, 0, 3, 0x7fffffff}, {INT32_MIN, 0, INT32_MAX, 0}};
    for (const fm_crop_rect& b : bad) CHECK(fm_jpeg_encode_regions_plan(&b, 1, 1, nullptr, &tot) != 0 && fm_jpeg_encode_regions_bound(&b, 1, 1) == 0);
    {
        std::vector<fm_crop_rect> many(FM_OBJENC_MAX_REGIONS + 1, one);
        CHECK(fm_jpeg_encode_regions_plan(many.data(), FM_OBJENC_MAX_REGIONS + 1, 1, nullptr, &tot) != 0);
        CHECK(fm_jpeg_encode_regions_plan(many.data(), FM_OBJENC_MAX_REGIONS, 1, nullptr, &tot) == 0 && tot.mcus == FM_OBJENC_MAX_REGIONS);
        fm_crop_rect huge = {0, 0, 16383, 16383};                // 2^20 MCUs
        CHECK(fm_jpeg_encode_regions_plan(&huge, 1, 1, nullptr, &tot) != 0);
        CHECK(fm_jpeg_encode_regions_plan(&huge, 1, 4, nullptr, &tot) != 0);
    }
    for (int round = 0; round < 300; ++round) {
        const int n = between(0, 12), shrink = 1 << between(0, 2);
        std::vector<fm_crop_rect> rects(n);
        for (fm_crop_rect& r : rects) {
            r.x0 = between(0, 500), r.y0 = between(0, 500);
            r.x1 = r.x0 + between(0, 1) * between(0, 300), r.y1 = r.y0 + between(0, 200);
        }
        fm_crop_plan* plans = (fm_crop_plan*)malloc(sizeof(fm_crop_plan) * (n ? n : 1));
        CHECK(fm_jpeg_encode_regions_plan(rects.data(), n, shrink, plans, &tot) == 0);
        CHECK(fm_jpeg_encode_regions_bound(rects.data(), n, shrink) == tot.bound);
        const int rows = tot.rows;
        uint32_t* lens = (uint32_t*)malloc(sizeof(uint32_t) * (rows ? rows : 1));
        size_t need = 0;
        for (int r = 0; r < rows; ++r) {
            lens[r] = (uint32_t)between(0, 90);
            need += ((size_t)lens[r] + 15) & ~(size_t)15;
        }
        // the segments as the device leaves them: exactly as many bytes as the padded lengths take
        uint8_t* segs = (uint8_t*)malloc(need ? need : 1);
        for (size_t i = 0; i < need; ++i) segs[i] = (uint8_t)rnd();
        const size_t bound = tot.bound ? (size_t)tot.bound : 1;
        size_t* offsets = (size_t*)malloc(sizeof(size_t) * (n + 1));
        uint8_t* out = (uint8_t*)malloc(bound);
        CHECK(fm_jpeg_encode_regions_assemble(plans, n, 75, lens, segs, need, out, bound, offsets) == 0);
        CHECK(offsets[0] == 0 && offsets[n] <= bound);
        for (int i = 0; i < n; ++i) {
            CHECK(offsets[i] < offsets[i + 1] && out[offsets[i]] == 0xFF && out[offsets[i] + 1] == 0xD8);
            CHECK(out[offsets[i + 1] - 2] == 0xFF && out[offsets[i + 1] - 1] == 0xD9);
        }
        const size_t total = offsets[n];
        free(out);
        // every smaller capacity: an error, nothing written past it (the block is exactly `cap` bytes)
        for (int k = 0; k < 4 && total > 0; ++k) {
            const size_t cap = k == 0 ? 0 : k == 1 ? total - 1 : (size_t)between(0, (int)total - 1);
            uint8_t* small = (uint8_t*)malloc(cap ? cap : 1);
            CHECK(fm_jpeg_encode_regions_assemble(plans, n, 75, lens, segs, need, small, cap, offsets) != 0);
            free(small);
        }
        out = (uint8_t*)malloc(bound);
        if (rows > 0) {
            // hostile lengths: one too long for what is left, huge ones, a segment buffer one byte short
            uint32_t* hostile = (uint32_t*)malloc(sizeof(uint32_t) * rows);
            for (int k = 0; k < 6; ++k) {
                memcpy(hostile, lens, sizeof(uint32_t) * rows);
                const int at = between(0, rows - 1);
                hostile[at] = k == 0 ? 0xFFFFFFFFu : k == 1 ? 0xFFFFFFF0u : k == 2 ? (uint32_t)need + 1 : k == 3 ? 1u << 31 : lens[at] + 16 * between(1, 4) + (uint32_t)need;
                CHECK(fm_jpeg_encode_regions_assemble(plans, n, 75, hostile, segs, need, out, bound, offsets) != 0);
            }
            if (need > 0 && lens[rows - 1] > 0)
                CHECK(fm_jpeg_encode_regions_assemble(plans, n, 75, lens, segs, need - 16, out, bound, offsets) != 0);
            free(hostile);
            // plans that do not number their rows without gaps, or state another grid than their size has
            fm_crop_plan keep = plans[n - 1];
            plans[n - 1].first_row += 1;
            CHECK(fm_jpeg_encode_regions_assemble(plans, n, 75, lens, segs, need, out, bound, offsets) != 0);
            plans[n - 1] = keep;
            plans[n - 1].mcus_y += 1;
            CHECK(fm_jpeg_encode_regions_assemble(plans, n, 75, lens, segs, need, out, bound, offsets) != 0);
            plans[n - 1] = keep;
            plans[n - 1].width = 0;
            CHECK(fm_jpeg_encode_regions_assemble(plans, n, 75, lens, segs, need, out, bound, offsets) != 0);
            plans[n - 1] = keep;
        }
        CHECK(fm_jpeg_encode_regions_assemble(plans, n, 0, lens, segs, need, out, bound, offsets) != 0);
        CHECK(fm_jpeg_encode_regions_assemble(plans, n, 75, lens, segs, need, out, bound, nullptr) != 0);
        free(out), free(offsets), free(segs), free(lens), free(plans);
    }
    puts("ok");
    return 0;
}
