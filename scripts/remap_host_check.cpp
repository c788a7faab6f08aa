// Stand-alone driver for the context-free twin of the remap kernel (fastmot_amd/csrc/remap_host.hip with remap_pixel.h:
// fm_remap_bgr_host), meant to be built with the host sanitizers and run on the CPU -- no GPU, no Python:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -c fastmot_amd/csrc/remap_host.hip -o /tmp/rmh.o
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -c -x hip scripts/remap_host_check.cpp -o /tmp/rmc.o
//   /opt/rocm/llvm/bin/clang++ -fsanitize=address,undefined /tmp/rmh.o /tmp/rmc.o -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib \
//         -o /tmp/remap_host_check && /tmp/remap_host_check
//
// (the sanitizers instrument host code only: -Xarch_host when compiling, a plain host link)
//
// Sources, maps and destinations are heap blocks of exactly their size, so a tap that is dereferenced outside the image is
// a heap overflow the sanitizer reports: what the clamp-before-load rule of remap_pixel.h (which the kernel shares)
// exists to prevent.  Sizes down to 1 x 1; maps that hold every value of the range's ends and random ones over the whole
// range; each result compared with a plain float64 bilinear statement; maps one past either end of the range, null
// pointers and sizes out of range, which must be refused with the destination untouched.  Exit status 0 and "ok" when
// every call returned what it should.
#include <cmath>
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

// float64 bilinear value of the quantised coordinate, border per tap, rounded half up
static int reference(const uint8_t* src, int sw, int sh, int X, int Y, int c, const uint8_t* border) {
    const int ix = (int)std::floor(X / 32.), iy = (int)std::floor(Y / 32.);
    const double a = X / 32. - ix, b = Y / 32. - iy;
    auto tap = [&](int x, int y) -> double {
        return x >= 0 && x < sw && y >= 0 && y < sh ? src[((size_t)y * sw + x) * 3 + c] : border[c];
    };
    const double v = (1. - b) * ((1. - a) * tap(ix, iy) + a * tap(ix + 1, iy)) + b * ((1. - a) * tap(ix, iy + 1) + a * tap(ix + 1, iy + 1));
    return (int)std::floor(v + 0.5);
}

int main() {
    const int sizes[][4] = {{1, 1, 1, 1}, {1, 1, 9, 9}, {2, 2, 8, 1}, {3, 3, 14, 14}, {1, 37, 5, 40}, {37, 1, 40, 5}, {37, 29, 13, 7}, {37, 29, 64, 48},
                            {16384, 2, 24, 3}, {2, 16384, 3, 24}};
    const uint8_t border[3] = {7, 130, 255};
    for (const auto& sz : sizes) {
        const int sw = sz[0], sh = sz[1], dw = sz[2], dh = sz[3];
        const size_t ns = (size_t)sw * sh * 3, nd = (size_t)dw * dh;
        // heap blocks of exactly their size
        uint8_t* const src = (uint8_t*)malloc(ns);
        int32_t* const xy = (int32_t*)malloc(nd * 2 * sizeof(int32_t));
        uint8_t* const dst = (uint8_t*)malloc(nd * 3);
        CHECK(src && xy && dst);
        for (size_t i = 0; i < ns; ++i) src[i] = (rnd() >> 9) & 1 ? (uint8_t)(rnd() >> 8) : (uint8_t)(((rnd() >> 8) & 1) * 255);
        const int ends_x[] = {-64, -33, -32, -31, -1, 0, 31, 32, 32 * (sw - 1) - 1, 32 * (sw - 1), 32 * (sw - 1) + 1, 32 * sw - 1, 32 * sw, 32 * sw + 32};
        const int ends_y[] = {-64, -33, -32, -31, -1, 0, 31, 32, 32 * (sh - 1) - 1, 32 * (sh - 1), 32 * (sh - 1) + 1, 32 * sh - 1, 32 * sh, 32 * sh + 32};
        for (int round = 0; round < 6; ++round) {
            for (size_t i = 0; i < nd; ++i) {
                if (round & 1) {      // the ends of every interval, in every combination over the rounds
                    int x = ends_x[between(0, 13)], y = ends_y[between(0, 13)];
                    xy[2 * i] = x < -64 ? -64 : x, xy[2 * i + 1] = y < -64 ? -64 : y;
                } else {
                    xy[2 * i] = between(-64, 32 * (sw + 1)), xy[2 * i + 1] = between(-64, 32 * (sh + 1));
                }
            }
            memset(dst, 0x5a, nd * 3);
            CHECK(fm_remap_bgr_host(src, sw, sh, xy, dst, dw, dh, border) == 0);
            for (size_t i = 0; i < nd; ++i)
                for (int c = 0; c < 3; ++c) CHECK(dst[3 * i + c] == reference(src, sw, sh, xy[2 * i], xy[2 * i + 1], c, border));
        }
        // refused, with the destination untouched
        memset(dst, 0x5a, nd * 3);
        const int32_t keep_x = xy[2 * (nd - 1)], keep_y = xy[2 * (nd - 1) + 1];
        const int bad[][2] = {{-65, 0}, {32 * (sw + 1) + 1, 0}, {0, -65}, {0, 32 * (sh + 1) + 1}, {INT32_MIN, 0}, {INT32_MAX, INT32_MAX}};
        for (const auto& b : bad) {
            xy[2 * (nd - 1)] = b[0], xy[2 * (nd - 1) + 1] = b[1];
            CHECK(fm_remap_bgr_host(src, sw, sh, xy, dst, dw, dh, border) == -2);
        }
        xy[2 * (nd - 1)] = keep_x, xy[2 * (nd - 1) + 1] = keep_y;
        CHECK(fm_remap_bgr_host(nullptr, sw, sh, xy, dst, dw, dh, border) == -2);
        CHECK(fm_remap_bgr_host(src, sw, sh, nullptr, dst, dw, dh, border) == -2);
        CHECK(fm_remap_bgr_host(src, sw, sh, xy, nullptr, dw, dh, border) == -2);
        CHECK(fm_remap_bgr_host(src, sw, sh, xy, dst, dw, dh, nullptr) == -2);
        CHECK(fm_remap_bgr_host(src, 0, sh, xy, dst, dw, dh, border) == -2);
        CHECK(fm_remap_bgr_host(src, sw, -1, xy, dst, dw, dh, border) == -2);
        CHECK(fm_remap_bgr_host(src, 16385, sh, xy, dst, dw, dh, border) == -2);
        CHECK(fm_remap_bgr_host(src, sw, sh, xy, dst, 0, dh, border) == -2);
        CHECK(fm_remap_bgr_host(src, sw, sh, xy, dst, dw, 16385, border) == -2);
        for (size_t i = 0; i < nd * 3; ++i) CHECK(dst[i] == 0x5a);
        free(src), free(xy), free(dst);
    }
    printf("ok\n");
    return 0;
}
