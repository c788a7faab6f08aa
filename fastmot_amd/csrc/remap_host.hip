// The context-free twin of remap.hip: a correction map applied to host pixels with the functions of remap_pixel.h --
// the CPU statement of what the kernel computes, compiled from the same text.  Needs no context and no GPU and may run
// on any number of threads at once.  scripts/remap_host_check.cpp drives this file alone under the host sanitizers.
#include "common.h"
#include "remap_pixel.h"

namespace {
// the 8-byte word the kernel loads at a pixel, from the bytes that exist: the pixel, and its right neighbour when the row
// has one (host arrays carry no slack behind the last pixel)
inline uint64_t host_px2(const uint8_t* row, int cx, int sw) {
    const uint8_t* const p = row + (size_t)cx * 3;
    uint64_t q = (uint64_t)p[0] | (uint64_t)p[1] << 8 | (uint64_t)p[2] << 16;
    if (cx + 1 < sw) q |= (uint64_t)p[3] << 24 | (uint64_t)p[4] << 32 | (uint64_t)p[5] << 40;
    return q;
}
}  // namespace

extern "C" int fm_remap_bgr_host(const uint8_t* src, int sw, int sh, const int32_t* xy, uint8_t* dst, int dw, int dh,
                                 const uint8_t border[3]) {
    FM_CHECK_ARG(src && xy && dst && border);
    FM_CHECK_ARG(sw >= 1 && sh >= 1 && sw <= FM_SRC_MAX_DIM && sh <= FM_SRC_MAX_DIM);
    FM_CHECK_ARG(dw >= 1 && dh >= 1 && dw <= FM_SRC_MAX_DIM && dh <= FM_SRC_MAX_DIM);
    const size_t n = (size_t)dw * dh;
    for (size_t i = 0; i < n; ++i) FM_CHECK_ARG(fm_remap_entry_ok(xy[2 * i], xy[2 * i + 1], sw, sh));
    const uint32_t bc = (uint32_t)border[0] | (uint32_t)border[1] << 8 | (uint32_t)border[2] << 16;
    for (size_t i = 0; i < n; ++i) {
        const FmRemapTap t = fm_remap_tap(xy[2 * i], xy[2 * i + 1], sw, sh);
        const uint64_t q0 = host_px2(src + (size_t)t.cy0 * sw * 3, t.cx, sw);
        const uint64_t q1 = host_px2(src + (size_t)t.cy1 * sw * 3, t.cx, sw);
        const uint32_t px = fm_remap_blend(q0, q1, t, bc);
        dst[3 * i] = (uint8_t)px, dst[3 * i + 1] = (uint8_t)(px >> 8), dst[3 * i + 2] = (uint8_t)(px >> 16);
    }
    return 0;
}
