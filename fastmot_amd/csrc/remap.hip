// Packed BGR u8 [sh][sw][3] -> packed BGR u8 [dh][dw][3] through a per-pixel correction map: lens undistortion (or any
// fixed geometric correction) and the frame-level resize in ONE gather.  While a map is set (fm_frame_remap_set) this
// kernel takes the place of resize.hip's behind the described-source calls (frames.hip): the frame is
// copied / converted at capture resolution and leaves this kernel as the W x H BGR frame every consumer reads.
//
// The arithmetic is remap_pixel.h's (5 fractional bits, border per tap, one rounding), shared with fm_remap_bgr_host and
// stated in numpy by fastmot_amd/utils/lens.py remap_bgr; tests compare bit for bit.  It is deliberately not the
// resize's (11-bit separable coefficients): an identity-geometry map gives pixels near the resize's, not equal to them.
//
// Laid out like resize_bgr_kernel: one thread owns 8 consecutive output pixels of a row, threads are numbered along a
// row first.  A thread reads its 8 map entries (int32 pairs, 64 bytes: four 16-byte loads), then 2 x 8 unaligned 8-byte
// loads (a pixel and its right neighbour are 6 consecutive bytes, pixel_source.h load_px2), all issued before the first
// use, and stores 24 bytes (three aligned 8-byte stores).  Load positions are clamped into the image BEFORE the load
// and the border is selected afterwards (fm_remap_tap): no tap outside the image is ever dereferenced, whatever the map
// holds.  The 8-byte load at the source's last pixel reaches 5 bytes past it: FM_FRAME_SLACK, as for the resize.  A
// streaming kernel: no LDS; no address depends on a pixel's value.
#include "common.h"
#include "bgr_run.h"
#include "pixel_source.h"
#include "remap_pixel.h"

namespace {

// VEC: dw % 8 == 0, an 8-byte aligned destination and a 16-byte aligned map -- 16-byte map loads and
// StoreRule::ALIGNED8.  Otherwise 8-byte map loads and StoreRule::BYTES (a pixel past the row's end is computed from
// the row's last entry and not stored).
template <bool VEC>
__global__ __launch_bounds__(256) void remap_bgr_kernel(const uint8_t* __restrict__ src, int sw, int sh,
                                                        const int32_t* __restrict__ xy, uint8_t* __restrict__ dst, int dw,
                                                        int dh, uint32_t border) {
    int y, x0, n;
    if (!run_of(dw, dh, y, x0, n)) return;

    int32_t m[16];
    if (VEC) {
        const int4* const mp = reinterpret_cast<const int4*>(xy + ((size_t)y * dw + x0) * 2);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int4 v = mp[q];
            m[4 * q] = v.x, m[4 * q + 1] = v.y, m[4 * q + 2] = v.z, m[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int x = min(x0 + i, dw - 1);
            const int2 v = *reinterpret_cast<const int2*>(xy + ((size_t)y * dw + x) * 2);
            m[2 * i] = v.x, m[2 * i + 1] = v.y;
        }
    }

    FmRemapTap t[8];
    uint64_t q0[8], q1[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {      // (branch-free: all 16 loads of a thread in flight at once)
        t[i] = fm_remap_tap(m[2 * i], m[2 * i + 1], sw, sh);
        q0[i] = load_px2(src + ((size_t)t[i].cy0 * sw + t[i].cx) * 3);
        q1[i] = load_px2(src + ((size_t)t[i].cy1 * sw + t[i].cx) * 3);
    }

    uint32_t o[6] = {};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t px = fm_remap_blend(q0[i], q1[i], t[i], border);
        put_px(o, i, px & 255u, (px >> 8) & 255u, (px >> 16) & 255u);
    }
    store_run<VEC ? StoreRule::ALIGNED8 : StoreRule::BYTES>(dst + ((size_t)y * dw + x0) * 3, n, o);
}

}  // namespace

// Writes the dw x dh BGR frame at `dst` (exactly dw * dh * 3 bytes) from the sw x sh BGR frame at `src` through the map
// `xy` ([dh][dw][2] int32 on the device, 8-byte aligned), on stream `s`.  border: b | g << 8 | r << 16.  `src` has
// FM_FRAME_SLACK readable bytes behind its last pixel.  Entries outside remap_pixel.h's range are memory-safe (the taps
// clamp) but are not what fm_frame_remap_set lets through.
int fm_remap_bgr(const uint8_t* src, int sw, int sh, const int32_t* xy, uint8_t* dst, int dw, int dh, uint32_t border, hipStream_t s) {
    FM_CHECK_ARG(src && xy && dst && sw > 0 && sh > 0 && dw > 0 && dh > 0 && sw <= FM_SRC_MAX_DIM && sh <= FM_SRC_MAX_DIM);
    FM_CHECK_ARG(!((uintptr_t)xy & 7));
    const long long blocks = (long long)((dw + 7) >> 3) * dh;
    FM_CHECK_ARG(blocks < (1ll << 31) - 256);
    const dim3 grid((unsigned)((blocks + 255) / 256));
    const bool vec = dw % 8 == 0 && !((uintptr_t)dst & 7) && !((uintptr_t)xy & 15);
    if (vec) hipLaunchKernelGGL((remap_bgr_kernel<true>), grid, dim3(256), 0, s, src, sw, sh, xy, dst, dw, dh, border);
    else hipLaunchKernelGGL((remap_bgr_kernel<false>), grid, dim3(256), 0, s, src, sw, sh, xy, dst, dw, dh, border);
    FM_HIP(hipGetLastError());
    return 0;
}
