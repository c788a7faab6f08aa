// What one redaction region (fm_redact_region, fastmot_hip.h "Redaction of the frames that leave the GPU") does to one
// pixel: the same text for the tile pass of overlay.hip, the cell-mean kernel of redact.hip and fm_redact_render_host.
// Everything is integer and exact; tests/redact_ref.py states the same rules in numpy and Python integers.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/fastmot_hip.h"

#define FM_RED_HD __host__ __device__ __forceinline__

// The part of a region that exists on a W x H frame: its rectangle clipped to the frame (inclusive; empty when
// cx1 < cx0 or cy1 < cy0, and then the index ranges are empty as well) and the range of the cells that own at least one
// pixel of it.  The grid is anchored at the UNCLIPPED corner (x0, y0): cell i covers the columns x0 + i c .. x0 + (i + 1) c - 1.
struct FmRedGrid {
    int cx0, cy0, cx1, cy1;
    int imin, imax, jmin, jmax;
};

FM_RED_HD FmRedGrid fm_red_grid(const fm_redact_region& r, int W, int H) {
    FmRedGrid g;
    g.cx0 = r.x0 > 0 ? r.x0 : 0, g.cy0 = r.y0 > 0 ? r.y0 : 0;
    g.cx1 = r.x1 < W - 1 ? r.x1 : W - 1, g.cy1 = r.y1 < H - 1 ? r.y1 : H - 1;
    if (g.cx1 < g.cx0 || g.cy1 < g.cy0) {
        g.cx0 = g.cy0 = 0, g.cx1 = g.cy1 = -1;
        g.imin = g.jmin = 0, g.imax = g.jmax = -1;
        return g;
    }
    g.imin = (g.cx0 - r.x0) / r.cell, g.imax = (g.cx1 - r.x0) / r.cell;
    g.jmin = (g.cy0 - r.y0) / r.cell, g.jmax = (g.cy1 - r.y0) / r.cell;
    return g;
}

// FM_REDACT_FILL needs no means: such a region has no cells in the device buffer
FM_RED_HD long long fm_red_cells(const fm_redact_region& r, const FmRedGrid& g) {
    return r.mode == FM_REDACT_FILL ? 0ll : (long long)(g.imax - g.imin + 1) * (long long)(g.jmax - g.jmin + 1);
}

// The pixels of cell index k along one axis that lie inside the clipped range [lo, hi]: first one and count
FM_RED_HD int fm_red_cell_span(int origin, int cell, int k, int lo, int hi, int& first) {
    const int a = origin + k * cell, b = a + cell - 1;
    first = a > lo ? a : lo;
    return (b < hi ? b : hi) - first + 1;
}

// Rounded mean of `sum` over n >= 1 pixels
FM_RED_HD unsigned fm_red_mean(unsigned sum, unsigned n) { return (sum + n / 2u) / n; }

// Is (x, y) a pixel of the region's shape?  (The frame clip is the caller's.)
FM_RED_HD bool fm_red_covers(const fm_redact_region& r, int x, int y) {
    if (x < r.x0 || x > r.x1 || y < r.y0 || y > r.y1) return false;
    if (r.shape != FM_REDACT_ELLIPSE) return true;
    const long long a = (long long)r.x1 - r.x0 + 1, b = (long long)r.y1 - r.y0 + 1;
    const long long dx = 2ll * (x - r.x0) + 1 - a, dy = 2ll * (y - r.y0) + 1 - b;
    return dx * dx * b * b + dy * dy * a * a <= a * a * b * b;      // sides <= 2^14: every term below 2^57
}

// u = 2 (p - origin) + 1 - c along one axis -> the lower cell index floor(u / 2c) and the weight u - 2c i0 in 0..2c-1 of
// the upper one
FM_RED_HD void fm_red_lerp(int p, int origin, int c, int& i0, int& f) {
    const int u = 2 * (p - origin) + 1 - c, d = 2 * c;
    i0 = u >= 0 ? u / d : -((d - 1 - u) / d);
    f = u - d * i0;
}

FM_RED_HD int fm_red_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// The value of pixel (x, y), which fm_red_covers said the region covers, as B | G << 8 | R << 16.  means: the region's
// cells, one word each in that format, rows of (imax - imin + 1) starting at cell (imin, jmin); unused for FM_REDACT_FILL.
FM_RED_HD uint32_t fm_red_value(const fm_redact_region& r, const FmRedGrid& g, const uint32_t* means, int x, int y) {
    if (r.mode == FM_REDACT_FILL) return (uint32_t)r.b | (uint32_t)r.g << 8 | (uint32_t)r.r << 16;
    const int c = r.cell, ncx = g.imax - g.imin + 1;
    if (r.mode == FM_REDACT_PIXELATE) return means[(size_t)((y - r.y0) / c - g.jmin) * ncx + ((x - r.x0) / c - g.imin)];
    int i0, j0, fx, fy;
    fm_red_lerp(x, r.x0, c, i0, fx);
    fm_red_lerp(y, r.y0, c, j0, fy);
    const int ia = fm_red_clamp(i0, g.imin, g.imax) - g.imin, ib = fm_red_clamp(i0 + 1, g.imin, g.imax) - g.imin;
    const size_t ja = (size_t)(fm_red_clamp(j0, g.jmin, g.jmax) - g.jmin) * ncx, jb = (size_t)(fm_red_clamp(j0 + 1, g.jmin, g.jmax) - g.jmin) * ncx;
    const uint32_t m00 = means[ja + ia], m10 = means[ja + ib], m01 = means[jb + ia], m11 = means[jb + ib];
    const uint32_t d = 2u * c, gx = d - fx, gy = d - fy, half = 2u * c * c, den = 4u * c * c;
    const uint32_t w00 = gx * gy, w10 = fx * gy, w01 = gx * fy, w11 = (uint32_t)fx * fy;      // sum: 4 c^2 <= 2^18
    uint32_t out = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int s = 8 * ch;
        const uint32_t v = w00 * ((m00 >> s) & 255u) + w10 * ((m10 >> s) & 255u) + w01 * ((m01 >> s) & 255u) + w11 * ((m11 >> s) & 255u) + half;
        out |= (v / den) << s;                                                             // v < 2^27
    }
    return out;
}
