// Packed BGR u8 [sh][sw][3] -> packed BGR u8 [dh][dw][3]: the frame-level resize behind fm_frame_upload_src /
// fm_frame_upload_ahead_src / fm_frame_ring_store_src (frames.hip).  A frame that arrives at capture
// resolution is copied (and, for NV12 / JPEG, converted) at that resolution and leaves this kernel as the W x H BGR
// frame that every consumer already reads, so nothing downstream knows the frame was ever larger.
//
// The arithmetic is cv2.resize's 8-bit INTER_LINEAR, integer and exact (fastmot_amd/videoio.py resize_bgr states it in
// numpy; tests compare bit for bit).  Per axis, for output index d (pixel_source.h lin_coef, shared with the ReID crop):
//     f = float((d + 0.5) * (ssize / dsize) - 0.5),  s = floor(f),  f -= s,  clamped: s < 0 -> (0, f = 0),
//     s >= ssize - 1 -> (ssize - 1, f = 0);   a0 = rint((1 - f) * 2048),  a1 = rint(f * 2048);   s' = min(s + 1, ssize - 1)
// and per channel, with p the source bytes at (row, column):
//     S0 = p[y][x] * ax0 + p[y][x'] * ax1,   S1 = p[y'][x] * ax0 + p[y'][x'] * ax1
//     v  = clamp((((ay0 * (S0 >> 4)) >> 16) + ((ay1 * (S1 >> 4)) >> 16) + 2) >> 2, 0, 255)
// An exact 2x decimation in BOTH axes (sw == 2 dw and sh == 2 dh) is cv2's INTER_AREA instead: the rounded 2 x 2 mean
// (a + b + c + d + 2) >> 2.  Every intermediate fits 32 bits: S <= 255 * 2048, ay * (S >> 4) <= 2048 * 32640 < 2^27.
//
// One thread owns 8 output pixels of a row: 2 x 8 unaligned 8-byte loads (a pixel and its right neighbour are 6
// consecutive bytes, pixel_source.h load_px2) and 24 BGR bytes out.  Threads are numbered along a row first, so a
// wavefront writes 1536 contiguous bytes (three 8-byte stores per thread, 24 bytes apart: the three together fill every
// cache line they touch) and reads two contiguous stretches of two source rows.  The vertical coefficients are computed
// once per thread, the horizontal ones once per pixel (8 float64 multiplies per 24 bytes stored).  A streaming
// kernel: no LDS; no address depends on a pixel's value.
#include "common.h"
#include "bgr_run.h"
#include "pixel_source.h"
#include "yuv_coef.h"      // clamp8

namespace {

// VEC: dw % 8 == 0 and an 8-byte aligned destination -- StoreRule::ALIGNED8.  Otherwise bytes (a pixel past the row's
// end is computed from the row's last column and not stored).
// AREA2: the 2 x 2 mean rule.
template <bool VEC, bool AREA2>
__global__ __launch_bounds__(256) void resize_bgr_kernel(const uint8_t* __restrict__ src, int sw, int sh,
                                                         uint8_t* __restrict__ dst, int dw, int dh) {
    int y, x0, n;
    if (!run_of(dw, dh, y, x0, n)) return;

    const ResizeCoef cy = lin_coef(y, (double)sh / dh, sh);
    const int ry0 = AREA2 ? 2 * y : cy.s, ry1 = AREA2 ? 2 * y + 1 : min(cy.s + 1, sh - 1);
    const uint8_t* const row0 = src + (size_t)ry0 * sw * 3;
    const uint8_t* const row1 = src + (size_t)ry1 * sw * 3;
    const double scale_x = (double)sw / dw;

    uint32_t o[6] = {};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int x = VEC ? x0 + i : min(x0 + i, dw - 1);      // (branch-free: all 16 loads of a thread in flight at once)
        const ResizeCoef cx = lin_coef(x, scale_x, sw);
        const int rx = AREA2 ? 2 * x : cx.s;
        const uint64_t q0 = load_px2(row0 + (size_t)rx * 3), q1 = load_px2(row1 + (size_t)rx * 3);
        // the right neighbour: the next 3 bytes, or the pixel itself at the clamped last column
        const int shift = (AREA2 || cx.s + 1 <= sw - 1) ? 24 : 0;
        uint32_t px[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int a0 = (int)((q0 >> (8 * c)) & 255), a1 = (int)((q0 >> (shift + 8 * c)) & 255);
            const int b0 = (int)((q1 >> (8 * c)) & 255), b1 = (int)((q1 >> (shift + 8 * c)) & 255);
            int v;
            if (AREA2) {
                v = (a0 + a1 + b0 + b1 + 2) >> 2;
            } else {
                const int S0 = a0 * cx.a0 + a1 * cx.a1;
                const int S1 = b0 * cx.a0 + b1 * cx.a1;
                v = (((cy.a0 * (S0 >> 4)) >> 16) + ((cy.a1 * (S1 >> 4)) >> 16) + 2) >> 2;
            }
            px[c] = clamp8(v);                          // clamped BEFORE it is narrowed and packed: yuv_coef.h sat8 says why
        }
        put_px(o, i, px[0], px[1], px[2]);
    }
    uint8_t* const out = dst + ((size_t)y * dw + x0) * 3;
    if (VEC) {
        store_run<StoreRule::ALIGNED8>(out, n, o);
    } else {
        // StoreRule::BYTES, with the row's end tested as the loop above tests it: with bgr_run.h's `k < 3 n` the compiler
        // issues the 16 loads in groups of four and the kernel measures 12 us for 11 (profiles/bgr_run_ab.txt)
#pragma unroll
        for (int k = 0; k < 24; ++k)
            if (x0 + k / 3 < dw) out[k] = (uint8_t)(o[k >> 2] >> ((k & 3) * 8));
    }
}

}  // namespace

// Resizes the sw x sh BGR frame at `src` to dw x dh at `dst` (exactly dw * dh * 3 bytes written), on stream `s`.  `src`
// has FM_FRAME_SLACK readable bytes behind its last pixel (the 8-byte load at the last pixel reaches 5 bytes past it).
int fm_resize_bgr(const uint8_t* src, int sw, int sh, uint8_t* dst, int dw, int dh, hipStream_t s) {
    FM_CHECK_ARG(src && dst && sw > 0 && sh > 0 && dw > 0 && dh > 0);
    const long long blocks = (long long)((dw + 7) >> 3) * dh;
    FM_CHECK_ARG(blocks < (1ll << 31) - 256);
    const dim3 grid((unsigned)((blocks + 255) / 256));
    const bool vec = dw % 8 == 0 && !((uintptr_t)dst & 7);
    const bool area2 = sw == 2 * dw && sh == 2 * dh;
#define FM_RESIZE_LAUNCH(V, A) hipLaunchKernelGGL((resize_bgr_kernel<V, A>), grid, dim3(256), 0, s, src, sw, sh, dst, dw, dh)
    if (vec && area2) FM_RESIZE_LAUNCH(true, true);
    else if (vec) FM_RESIZE_LAUNCH(true, false);
    else if (area2) FM_RESIZE_LAUNCH(false, true);
    else FM_RESIZE_LAUNCH(false, false);
#undef FM_RESIZE_LAUNCH
    FM_HIP(hipGetLastError());
    return 0;
}
