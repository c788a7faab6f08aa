// Packed 4:2:2 (YUY2 / UYVY / YVYU) and packed RGB (any channel order, 3 or 4 bytes per pixel) -> packed BGR u8: the
// kernels behind fm_frame_upload_packed / fm_frame_upload_ahead_packed / fm_frame_ring_store_packed (frames.hip).
// Packed 4:2:2 is what UVC / V4L2 cameras and capture cards deliver, RGB what image libraries hand out, BGRx
// what `nvvidconv` / `appsink` do.  The frame arrives in device staging with its rows packed to their byte width
// (4 * ceil(W / 2), 3 W or 4 W) and leaves as the BGR frame every consumer reads.
//
// 4:2:2: one 4-byte macropixel carries Y0, Y1 and the U, V both pixels use; yuv_coef.h's arithmetic per pixel
// for the two limited-range matrices, and for the two full-range ones the same expression with a luma offset of 0 and a
// luma factor of 1 << 20, which is  y = Y << 20  (fastmot_amd/utils/packed.py states all of it in numpy, tests compare
// bit for bit).  Full range fits 32 bits as limited range does: 255 * 2^20 + 2^19 + 128 * 1945738 < 2^29.
// RGB: a byte permutation; a fourth byte is dropped -- hwc.hip's kernel with the row's bytes as its pitch.
//
// One thread owns 8 pixels of one row: 16 bytes (four macropixels) in, 24 BGR bytes out.  Threads are numbered along a
// row first, so a wavefront reads 1 KiB of contiguous bytes per row and writes 1536.  Macropixels lie 4-byte aligned
// whatever W is (the staging is hipMalloc'ed, the row width a multiple of 4), so by bgr_run.h's load_run a whole run is
// one 16-byte load where the row begins 16-byte aligned and narrower ones otherwise; stores are StoreRule::BY_ADDRESS.
// No address depends on a pixel.  A streaming kernel (5 bytes per pixel): no LDS, no reuse beyond a macropixel's chroma.
#include "common.h"
#include "bgr_run.h"
#include "yuv_coef.h"

namespace {

// src: H rows of rb = 4 * ceil(W / 2) bytes, 4-byte aligned.  ysh / ush / vsh: the bit a macropixel's Y0 / U / V begins
// at when it is read as one little-endian word (Y1 lies 16 bits above Y0); yoff: 16 (limited range) or 0.
__global__ __launch_bounds__(256) void packed422_to_bgr_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ bgr, int W, int H,
                                                               int rb, int ysh, int ush, int vsh, int yoff, Nv12Coef c) {
    int r, x0, n;
    if (!run_of(W, H, r, x0, n)) return;
    const int nm = (n + 1) >> 1;                           // macropixels under the run
    uint32_t m[4];
    load_run<4>(src + (size_t)r * rb + (size_t)x0 * 2, 4 * nm, nm == 4, m);

    uint32_t o[6] = {};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int cb, cg, cr;
        ycc_chroma(c, (int)((m[j] >> ush) & 0xffu) - 128, (int)((m[j] >> vsh) & 0xffu) - 128, cb, cg, cr);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            uint32_t b, g, d;
            ycc_px(c, (int)((m[j] >> (ysh + 16 * t)) & 0xffu), yoff, cb, cg, cr, b, g, d);
            put_px(o, 2 * j + t, b, g, d);
        }
    }
    store_run<StoreRule::BY_ADDRESS>(bgr + ((size_t)r * W + x0) * 3, n, o);
}

}  // namespace

// Converts the packed frame at `src` (h rows of fm_packed_row_bytes(w, format) bytes, 4-byte aligned) to w * h * 3 BGR
// bytes at `bgr`, on stream `s`.  The callers have checked the arguments.
int fm_packed_to_bgr(const uint8_t* src, uint8_t* bgr, int w, int h, int format, int matrix, hipStream_t s) {
    const size_t rb = fm_packed_row_bytes(w, format);
    FM_CHECK_ARG(src && bgr && w >= 1 && h >= 1 && w <= FM_SRC_MAX_DIM && h <= FM_SRC_MAX_DIM && rb && fm_packed_matrix_ok(matrix) &&
                 !((uintptr_t)src & 3));
    if (format < FM_PACKED_YUY2) return fm_hwc_to_bgr(src, (long long)rb, bgr, w, h, format, s);
    const long long threads = (long long)((w + 7) >> 3) * h;
    const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
    const bool full = matrix >= FM_PACKED_BT601_FULL;
    const Nv12Coef& c = full ? PACKED_FULL_COEF[matrix - FM_PACKED_BT601_FULL] : NV12_COEF[matrix];
    const int ysh = format == FM_PACKED_UYVY ? 8 : 0;
    const int ush = format == FM_PACKED_YUY2 ? 8 : format == FM_PACKED_UYVY ? 0 : 24;
    const int vsh = format == FM_PACKED_YUY2 ? 24 : format == FM_PACKED_UYVY ? 16 : 8;
    hipLaunchKernelGGL(packed422_to_bgr_kernel, grid, block, 0, s, src, bgr, w, h, (int)rb, ysh, ush, vsh, full ? 0 : 16, c);
    FM_HIP(hipGetLastError());
    return 0;
}
