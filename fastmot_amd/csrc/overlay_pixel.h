// What one overlay command (fm_overlay_cmd, fastmot_hip.h) does to one pixel: the same text for the kernel of overlay.hip
// and for fm_overlay_render_host.  The rules are Pillow's ImageDraw (12.2.0) in integers; tests/overlay_ref.py states
// them in numpy and tests/test_overlay_host.py compares both with Pillow itself.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/fastmot_hip.h"

#define FM_OVL_HD __host__ __device__ __forceinline__

struct FmOvlBox {      // inclusive corners; empty when x1 < x0 or y1 < y0
    int x0, y0, x1, y1;
};

// Every pixel the command can touch lies inside this box (for an outline it is generous: a degenerate box spills up to
// `thickness` pixels past its corners).
FM_OVL_HD FmOvlBox fm_ovl_bbox(const fm_overlay_cmd& c) {
    switch (c.kind) {
    case FM_OVL_RECT_FILL: return {c.x0, c.y0, c.x1, c.y1};
    case FM_OVL_RECT_OUTLINE: {
        if (c.x1 < c.x0 || c.y1 < c.y0) return {0, 0, -1, -1};
        const int t = c.thickness;
        return {c.x0 - t, c.y0 - t, c.x1 + t, c.y1 + t};
    }
    case FM_OVL_LINE:
        return {c.x0 < c.x1 ? c.x0 : c.x1, c.y0 < c.y1 ? c.y0 : c.y1, c.x0 < c.x1 ? c.x1 : c.x0, c.y0 < c.y1 ? c.y1 : c.y0};
    case FM_OVL_DOT: return {c.x0 - 1, c.y0 - 1, c.x0 + 1, c.y0 + 1};
    case FM_OVL_MASK: return {c.x0, c.y0, c.x0 + c.x1 - 1, c.y0 + c.y1 - 1};
    default: return {0, 0, -1, -1};
    }
}

// `thickness` rings growing inward.  Rows y0 + i and y1 - i span [x0, x1]; the columns x0 + i and x1 - i are lines
// without their last point from y0 + t towards y1 - t + 1: downwards over y0 + t .. y1 - t when the box is at least
// 2 t high, otherwise upwards over y0 + t .. y1 - t + 2.
FM_OVL_HD bool fm_ovl_outline_covers(const fm_overlay_cmd& c, int x, int y) {
    if (c.x1 < c.x0 || c.y1 < c.y0) return false;
    const int t = c.thickness;
    if (x >= c.x0 && x <= c.x1 && ((y >= c.y0 && y < c.y0 + t) || (y <= c.y1 && y > c.y1 - t))) return true;
    if (!((x >= c.x0 && x < c.x0 + t) || (x <= c.x1 && x > c.x1 - t))) return false;
    return (y >= c.y0 + t && y <= c.y1 - t) || (y >= c.y1 - t + 2 && y <= c.y0 + t);
}

// Bresenham, both ends drawn, in closed form: i steps along the major axis from the start, the minor axis has moved
// (2 minor i + major) / (2 major) steps.  Coordinates up to 2^20 make the product 2^43: 64-bit, except for the segments
// short enough for 32 (every segment of a real scene).
FM_OVL_HD bool fm_ovl_line_covers(const fm_overlay_cmd& c, int x, int y) {
    const int dx = c.x1 < c.x0 ? c.x0 - c.x1 : c.x1 - c.x0, dy = c.y1 < c.y0 ? c.y0 - c.y1 : c.y1 - c.y0;
    const int xs = c.x1 < c.x0 ? -1 : 1, ys = c.y1 < c.y0 ? -1 : 1;
    const bool xmajor = dx > dy;
    const int major = xmajor ? dx : dy, minor = xmajor ? dy : dx;
    const int i = xmajor ? (x - c.x0) * xs : (y - c.y0) * ys;
    if (i < 0 || i > major) return false;
    int off = 0;
    if (major > 0) {
        if (major < 16384)
            off = (int)((2u * (unsigned)minor * (unsigned)i + (unsigned)major) / (2u * (unsigned)major));
        else
            off = (int)((2ull * (unsigned long long)minor * (unsigned long long)i + (unsigned long long)major) /
                        (2ull * (unsigned long long)major));
    }
    return xmajor ? y == c.y0 + ys * off : x == c.x0 + xs * off;
}

FM_OVL_HD unsigned fm_ovl_blend(unsigned m, unsigned ink, unsigned bg) {
    const unsigned t = m * ink + (255u - m) * bg + 128u;
    return (t + (t >> 8)) >> 8;
}

// Applies command c to the pixel at (x, y), whose channels are b, g, r.  masks: the blob FM_OVL_MASK commands index
// (fm_overlay_check has made sure that they stay inside it).
FM_OVL_HD void fm_ovl_apply(const fm_overlay_cmd& c, const uint8_t* masks, int x, int y, unsigned& b, unsigned& g, unsigned& r) {
    bool cover;
    switch (c.kind) {
    case FM_OVL_RECT_FILL: cover = x >= c.x0 && x <= c.x1 && y >= c.y0 && y <= c.y1; break;
    case FM_OVL_RECT_OUTLINE: cover = fm_ovl_outline_covers(c, x, y); break;
    case FM_OVL_LINE: cover = fm_ovl_line_covers(c, x, y); break;
    case FM_OVL_DOT: cover = (x == c.x0 && y >= c.y0 - 1 && y <= c.y0 + 1) || (y == c.y0 && x >= c.x0 - 1 && x <= c.x0 + 1); break;
    case FM_OVL_MASK: {
        const int mx = x - c.x0, my = y - c.y0;
        if (mx < 0 || mx >= c.x1 || my < 0 || my >= c.y1) return;
        const unsigned m = masks[(size_t)c.mask_off + (size_t)my * (size_t)c.x1 + (size_t)mx];
        b = fm_ovl_blend(m, c.b, b), g = fm_ovl_blend(m, c.g, g), r = fm_ovl_blend(m, c.r, r);
        return;
    }
    default: return;
    }
    if (cover) b = c.b, g = c.g, r = c.r;
}
