// Stand-alone driver for the context-free half of the overlay path (fastmot_amd/csrc/overlay_host.hip with
// overlay_pixel.h: fm_overlay_check and fm_overlay_render_host), meant to be built with the host sanitizers and run on the
// CPU -- no GPU, no Python:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -c fastmot_amd/csrc/overlay_host.hip -o /tmp/ovh.o
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -c -x hip scripts/overlay_host_check.cpp -o /tmp/ovc.o
//   /opt/rocm/llvm/bin/clang++ -fsanitize=address,undefined /tmp/ovh.o /tmp/ovc.o -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib \
//         -o /tmp/overlay_host_check && /tmp/overlay_host_check
//
// (the sanitizers instrument host code only: -Xarch_host when compiling, a plain host link)
//
// Frames and mask blobs are heap blocks of exactly their size, so a load or store past them is a heap overflow the
// sanitizer reports.  Valid lists of every kind at frame sizes down to 1 x 1 and widths of 1, with coordinates inside, across
// and far outside the frame and at the limits; hostile lists -- mask rectangles past the blob, coordinates beyond the
// limits, unknown kinds, thicknesses, counts -- which must be refused with the frame untouched; n = 0.  Exit status 0
// and "ok" when every call returned what it should.
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

static uint32_t rng_state = 2024;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }
static int between(int lo, int hi) { return lo + (int)((rnd() >> 8) % (uint32_t)(hi - lo + 1)); }

static fm_overlay_cmd make(int kind, int x0, int y0, int x1, int y1, int t = 1, uint32_t off = 0) {
    fm_overlay_cmd c;
    memset(&c, 0, sizeof c);
    c.kind = kind, c.x0 = x0, c.y0 = y0, c.x1 = x1, c.y1 = y1;
    c.b = (uint8_t)rnd(), c.g = (uint8_t)rnd(), c.r = (uint8_t)rnd();
    c.thickness = (uint8_t)t, c.mask_off = off;
    return c;
}

int main() {
    const int LIM = FM_OVERLAY_MAX_COORD;
    const int sizes[][2] = {{1, 1}, {1, 37}, {37, 1}, {2, 3}, {67, 35}, {80, 48}, {200, 40}};
    for (auto& s : sizes) {
        const int w = s[0], h = s[1];
        const size_t pitch = (size_t)w * 3, bytes = pitch * h;
        uint8_t* frame = (uint8_t*)malloc(bytes);
        uint8_t* copy = (uint8_t*)malloc(bytes);
        for (size_t i = 0; i < bytes; ++i) frame[i] = (uint8_t)rnd();
        const int mw = 23, mh = 9;
        const size_t mask_bytes = (size_t)mw * mh;
        uint8_t* masks = (uint8_t*)malloc(mask_bytes);
        for (size_t i = 0; i < mask_bytes; ++i) masks[i] = (uint8_t)rnd();

        // ---- valid lists
        std::vector<fm_overlay_cmd> list;
        for (int i = 0; i < 400; ++i) {
            const int kind = i % 5, span = i % 3 == 0 ? 3 * (w + h) : (i % 3 == 1 ? 8 : LIM);
            const int x0 = between(-span, span + w), y0 = between(-span, span + h), x1 = between(-span, span + w), y1 = between(-span, span + h);
            if (kind == FM_OVL_MASK)
                list.push_back(make(kind, between(-mw - 2, w + 2), between(-mh - 2, h + 2), mw, mh));
            else if (kind == FM_OVL_RECT_FILL || kind == FM_OVL_RECT_OUTLINE)
                list.push_back(make(kind, x0 < x1 ? x0 : x1, y0 < y1 ? y0 : y1, x0 < x1 ? x1 : x0, y0 < y1 ? y1 : y0, 1 + i % 8));
            else
                list.push_back(make(kind, x0 > LIM ? LIM : x0, y0 > LIM ? LIM : y0, x1 > LIM ? LIM : x1, y1 > LIM ? LIM : y1));
        }
        for (auto& c : list) {                       // (between() can pass the limits by the frame's size)
            if (c.kind == FM_OVL_MASK) continue;
            for (int32_t* v : {&c.x0, &c.y0, &c.x1, &c.y1}) *v = *v > LIM ? LIM : (*v < -LIM ? -LIM : *v);
        }
        list.push_back(make(FM_OVL_LINE, -LIM, -LIM, LIM, LIM));
        list.push_back(make(FM_OVL_LINE, LIM, -LIM, -LIM, LIM - 1));
        list.push_back(make(FM_OVL_RECT_FILL, -LIM, -LIM, LIM, LIM));
        list.push_back(make(FM_OVL_RECT_OUTLINE, -LIM, -LIM, LIM, LIM, 8));
        list.push_back(make(FM_OVL_RECT_OUTLINE, 0, 0, 0, 0, 8));
        list.push_back(make(FM_OVL_DOT, LIM, -LIM, 0, 0));
        list.push_back(make(FM_OVL_MASK, LIM, LIM, mw, mh));
        list.push_back(make(FM_OVL_MASK, -LIM, 0, mw, mh));
        list.push_back(make(FM_OVL_MASK, 0, 0, 1, (int)mask_bytes));            // one column, the whole blob
        list.push_back(make(FM_OVL_MASK, 0, 0, (int)mask_bytes, 1));
        list.push_back(make(FM_OVL_MASK, 0, 0, 0, 0, 1, (uint32_t)mask_bytes));   // empty, at the very end
        list.push_back(make(FM_OVL_MASK, w - 1, h - 1, 1, 1, 1, (uint32_t)mask_bytes - 1));
        CHECK(fm_overlay_check(list.data(), (int)list.size(), masks, mask_bytes, w, h) == 0);
        CHECK(fm_overlay_render_host(frame, w, h, pitch, list.data(), (int)list.size(), masks, mask_bytes) == 0);
        // n = 0 with and without pointers
        memcpy(copy, frame, bytes);
        CHECK(fm_overlay_render_host(frame, w, h, pitch, nullptr, 0, nullptr, 0) == 0);
        CHECK(fm_overlay_render_host(frame, w, h, pitch, list.data(), 0, masks, mask_bytes) == 0);
        CHECK(memcmp(copy, frame, bytes) == 0);

        // ---- hostile lists: refused, nothing written
        std::vector<fm_overlay_cmd> bad_cmds = {
            make(5, 0, 0, 1, 1), make(-1, 0, 0, 1, 1), make(0x7fffffff, 0, 0, 1, 1),
            make(FM_OVL_RECT_OUTLINE, 0, 0, 5, 5, 0), make(FM_OVL_RECT_OUTLINE, 0, 0, 5, 5, 9), make(FM_OVL_RECT_OUTLINE, 0, 0, 5, 5, 255),
            make(FM_OVL_LINE, LIM + 1, 0, 0, 0), make(FM_OVL_LINE, 0, -LIM - 1, 0, 0), make(FM_OVL_LINE, 0, 0, INT32_MAX, 0),
            make(FM_OVL_LINE, 0, 0, 0, INT32_MIN), make(FM_OVL_DOT, INT32_MIN, 0, 0, 0), make(FM_OVL_RECT_FILL, 0, 0, LIM + 1, 0),
            make(FM_OVL_MASK, 0, 0, mw, mh, 1, 1), make(FM_OVL_MASK, 0, 0, mw, mh + 1), make(FM_OVL_MASK, 0, 0, 1, 1, 1, (uint32_t)mask_bytes),
            make(FM_OVL_MASK, 0, 0, 0, 0, 1, (uint32_t)mask_bytes + 1), make(FM_OVL_MASK, 0, 0, 1, 1, 1, 0xFFFFFFFFu),
            make(FM_OVL_MASK, 0, 0, -1, mh), make(FM_OVL_MASK, 0, 0, mw, -1), make(FM_OVL_MASK, 0, 0, LIM, LIM),
            make(FM_OVL_MASK, 0, 0, LIM + 1, 0), make(FM_OVL_MASK, 0, 0, 65536, 65536), make(FM_OVL_MASK, LIM + 1, 0, 1, 1)};
        for (const fm_overlay_cmd& b : bad_cmds) {
            std::vector<fm_overlay_cmd> l = {make(FM_OVL_RECT_FILL, 0, 0, w, h), b};
            CHECK(fm_overlay_check(l.data(), 2, masks, mask_bytes, w, h) != 0);
            CHECK(fm_overlay_render_host(frame, w, h, pitch, l.data(), 2, masks, mask_bytes) != 0);
            CHECK(memcmp(copy, frame, bytes) == 0);
        }
        fm_overlay_cmd m = make(FM_OVL_MASK, 0, 0, 1, 1);
        CHECK(fm_overlay_check(&m, 1, nullptr, 0, w, h) != 0);                    // a mask and no blob
        CHECK(fm_overlay_check(&m, 1, nullptr, mask_bytes, w, h) != 0);
        CHECK(fm_overlay_check(nullptr, 1, masks, mask_bytes, w, h) != 0);
        CHECK(fm_overlay_check(&m, -1, masks, mask_bytes, w, h) != 0);
        CHECK(fm_overlay_check(&m, FM_OVERLAY_MAX_CMDS + 1, masks, mask_bytes, w, h) != 0);      // (refused before it is read)
        CHECK(fm_overlay_check(&m, 1, masks, (size_t)FM_OVERLAY_MAX_MASK_BYTES + 1, w, h) != 0);
        CHECK(fm_overlay_check(&m, 1, masks, mask_bytes, 0, h) != 0 && fm_overlay_check(&m, 1, masks, mask_bytes, w, FM_SRC_MAX_DIM + 1) != 0);
        CHECK(fm_overlay_render_host(nullptr, w, h, pitch, &m, 1, masks, mask_bytes) != 0);
        CHECK(fm_overlay_render_host(frame, w, h, pitch - 1, &m, 1, masks, mask_bytes) != 0);
        CHECK(memcmp(copy, frame, bytes) == 0);
        free(frame), free(copy), free(masks);
    }
    // a padded frame: the bytes between the rows stay as they are
    {
        const int w = 5, h = 4;
        const size_t pitch = 24;
        std::vector<uint8_t> frame(pitch * h, 0x5A);
        fm_overlay_cmd c = make(FM_OVL_RECT_FILL, -3, -3, 50, 50);
        c.b = c.g = c.r = 1;
        CHECK(fm_overlay_render_host(frame.data(), w, h, pitch, &c, 1, nullptr, 0) == 0);
        for (int y = 0; y < h; ++y)
            for (size_t i = 0; i < pitch; ++i) CHECK(frame[y * pitch + i] == (i < (size_t)w * 3 ? 1 : 0x5A));
    }
    puts("ok");
    return 0;
}
