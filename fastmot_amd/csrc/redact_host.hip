// The context-free half of the redaction path (fastmot_hip.h "Redaction of the frames that leave the GPU"): the check
// every entry point runs on a region list first, and the list applied to host pixels with the functions of
// redact_pixel.h -- the CPU statement of what redact.hip and the tile pass of overlay.hip compute.  Neither needs a
// context or a GPU; both may run on any number of threads at once.
#include "common.h"
#include "redact_pixel.h"

static_assert(sizeof(fm_redact_region) == 32, "fm_redact_region is two 16-byte words");

extern "C" int fm_redact_check(const fm_redact_region* regions, int n, int width, int height) {
    FM_CHECK_ARG(n >= 0 && n <= FM_REDACT_MAX_REGIONS && (regions || n == 0));
    FM_CHECK_ARG(width >= 1 && height >= 1 && width <= FM_SRC_MAX_DIM && height <= FM_SRC_MAX_DIM);
    constexpr int LIM = FM_OVERLAY_MAX_COORD;
    long long cells = 0;
    for (int i = 0; i < n; ++i) {
        const fm_redact_region& r = regions[i];
        FM_CHECK_ARG(r.mode >= FM_REDACT_PIXELATE && r.mode <= FM_REDACT_FILL);
        FM_CHECK_ARG(r.shape == FM_REDACT_RECT || r.shape == FM_REDACT_ELLIPSE);
        FM_CHECK_ARG(r.cell >= 2 && r.cell <= 256 && r.reserved == 0);
        FM_CHECK_ARG(r.x0 >= -LIM && r.x0 <= LIM && r.y0 >= -LIM && r.y0 <= LIM);
        FM_CHECK_ARG(r.x1 >= -LIM && r.x1 <= LIM && r.y1 >= -LIM && r.y1 <= LIM);
        if (r.x1 < r.x0 || r.y1 < r.y0) continue;
        FM_CHECK_ARG(r.x1 - r.x0 < FM_SRC_MAX_DIM && r.y1 - r.y0 < FM_SRC_MAX_DIM);
        cells += fm_red_cells(r, fm_red_grid(r, width, height));
        FM_CHECK_ARG(cells <= FM_REDACT_MAX_CELLS);
    }
    return 0;
}

extern "C" int fm_redact_render_host(uint8_t* pixels, int width, int height, size_t pitch, const fm_redact_region* regions, int n) {
    if (int rc = fm_redact_check(regions, n, width, height)) return rc;
    FM_CHECK_ARG(pixels && pitch >= (size_t)width * 3);
    if (n == 0) return 0;
    const size_t row = (size_t)width * 3;
    std::vector<uint8_t> orig(row * height);                   // what every region reads
    for (int y = 0; y < height; ++y) memcpy(orig.data() + y * row, pixels + (size_t)y * pitch, row);
    std::vector<uint32_t> means;
    for (int k = 0; k < n; ++k) {
        const fm_redact_region& r = regions[k];
        const FmRedGrid g = fm_red_grid(r, width, height);
        if (g.cx1 < g.cx0 || g.cy1 < g.cy0) continue;
        const int ncx = g.imax - g.imin + 1;
        means.assign((size_t)fm_red_cells(r, g), 0u);
        if (!means.empty())
            for (int j = g.jmin; j <= g.jmax; ++j)
                for (int i = g.imin; i <= g.imax; ++i) {
                    int xa, ya;
                    const int nx = fm_red_cell_span(r.x0, r.cell, i, g.cx0, g.cx1, xa), ny = fm_red_cell_span(r.y0, r.cell, j, g.cy0, g.cy1, ya);
                    unsigned sum[3] = {0, 0, 0};
                    for (int y = ya; y < ya + ny; ++y)
                        for (int x = xa; x < xa + nx; ++x)
                            for (int ch = 0; ch < 3; ++ch) sum[ch] += orig[y * row + 3 * (size_t)x + ch];
                    const unsigned cnt = (unsigned)nx * (unsigned)ny;
                    means[(size_t)(j - g.jmin) * ncx + (i - g.imin)] =
                        fm_red_mean(sum[0], cnt) | fm_red_mean(sum[1], cnt) << 8 | fm_red_mean(sum[2], cnt) << 16;
                }
        for (int y = g.cy0; y <= g.cy1; ++y) {
            uint8_t* const out = pixels + (size_t)y * pitch;
            for (int x = g.cx0; x <= g.cx1; ++x) {
                if (!fm_red_covers(r, x, y)) continue;
                const uint32_t v = fm_red_value(r, g, means.data(), x, y);
                out[3 * x] = (uint8_t)v, out[3 * x + 1] = (uint8_t)(v >> 8), out[3 * x + 2] = (uint8_t)(v >> 16);
            }
        }
    }
    return 0;
}
