// The context-free half of the overlay path (fastmot_hip.h "Overlays ON the device frame"): the check every entry point
// runs on a command list first, and the list applied to host pixels with the functions of overlay_pixel.h -- the CPU
// statement of what the kernel of overlay.hip computes.  Neither needs a context or a GPU; both may run on any number of
// threads at once.  scripts/overlay_host_check.cpp drives this file alone under the host sanitizers.
#include "common.h"
#include "overlay_pixel.h"

extern "C" int fm_overlay_check(const fm_overlay_cmd* cmds, int n, const uint8_t* masks, size_t mask_bytes, int width, int height) {
    FM_CHECK_ARG(n >= 0 && n <= FM_OVERLAY_MAX_CMDS && (cmds || n == 0));
    FM_CHECK_ARG(mask_bytes <= FM_OVERLAY_MAX_MASK_BYTES && (masks || mask_bytes == 0));
    FM_CHECK_ARG(width >= 1 && height >= 1 && width <= FM_SRC_MAX_DIM && height <= FM_SRC_MAX_DIM);
    constexpr int LIM = FM_OVERLAY_MAX_COORD;
    for (int i = 0; i < n; ++i) {
        const fm_overlay_cmd& c = cmds[i];
        FM_CHECK_ARG(c.kind >= FM_OVL_RECT_FILL && c.kind <= FM_OVL_MASK);
        FM_CHECK_ARG(c.x0 >= -LIM && c.x0 <= LIM && c.y0 >= -LIM && c.y0 <= LIM);
        if (c.kind == FM_OVL_MASK) {
            FM_CHECK_ARG(c.x1 >= 0 && c.x1 <= LIM && c.y1 >= 0 && c.y1 <= LIM);
            const unsigned long long bytes = (unsigned long long)c.x1 * (unsigned long long)c.y1;
            FM_CHECK_ARG(c.mask_off <= mask_bytes && bytes <= mask_bytes - c.mask_off);
        } else {
            FM_CHECK_ARG(c.x1 >= -LIM && c.x1 <= LIM && c.y1 >= -LIM && c.y1 <= LIM);
        }
        if (c.kind == FM_OVL_RECT_OUTLINE) FM_CHECK_ARG(c.thickness >= 1 && c.thickness <= 8);
    }
    return 0;
}

extern "C" int fm_overlay_render_host(uint8_t* pixels, int width, int height, size_t pitch, const fm_overlay_cmd* cmds, int n,
                                      const uint8_t* masks, size_t mask_bytes) {
    if (int rc = fm_overlay_check(cmds, n, masks, mask_bytes, width, height)) return rc;
    FM_CHECK_ARG(pixels && pitch >= (size_t)width * 3);
    for (int i = 0; i < n; ++i) {
        const fm_overlay_cmd& c = cmds[i];
        const FmOvlBox bb = fm_ovl_bbox(c);
        const int x0 = bb.x0 > 0 ? bb.x0 : 0, y0 = bb.y0 > 0 ? bb.y0 : 0;
        const int x1 = bb.x1 < width - 1 ? bb.x1 : width - 1, y1 = bb.y1 < height - 1 ? bb.y1 : height - 1;
        for (int y = y0; y <= y1; ++y) {
            uint8_t* const row = pixels + (size_t)y * pitch;
            for (int x = x0; x <= x1; ++x) {
                unsigned b = row[3 * x], g = row[3 * x + 1], r = row[3 * x + 2];
                fm_ovl_apply(c, masks, x, y, b, g, r);
                row[3 * x] = (uint8_t)b, row[3 * x + 1] = (uint8_t)g, row[3 * x + 2] = (uint8_t)r;
            }
        }
    }
    return 0;
}
