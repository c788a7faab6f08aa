// Interleaved RGB in any of six channel orders, 3 or 4 bytes per pixel -> packed BGR u8: a byte permutation, a fourth byte
// dropped.  One kernel behind both ways such a frame arrives: staged from the host with its rows packed (packed.hip,
// pitch = the row's bytes) and where a producer left it in device memory (devsrc.hip, any pitch, any first byte).
// fastmot_amd/utils/packed.py and utils/devarray.py state it in numpy; tests compare bit for bit.
//
// One thread owns 8 pixels of a row: 24 or 32 bytes in, 24 BGR bytes out; a wavefront reads 1.5 or 2 KiB of contiguous
// bytes and writes 1536.  Nothing but the address itself is known about a run, so loads and stores are chosen per thread
// by bgr_run.h's rules (load_run, StoreRule::BY_ADDRESS).  A streaming kernel (6 or 7 bytes per pixel): no LDS, no reuse.
#include "common.h"
#include "bgr_run.h"

namespace {

// src: H rows of BPP * W bytes, `pitch` bytes apart.  rsh / gsh / bsh: the bit R / G / B begins at in a pixel read as one
// little-endian word.
template <int BPP>
__global__ __launch_bounds__(256) void hwc_to_bgr_kernel(const uint8_t* __restrict__ src, long long pitch, uint8_t* __restrict__ bgr, int W,
                                                         int H, int rsh, int gsh, int bsh) {
    int r, x0, n;
    if (!run_of(W, H, r, x0, n)) return;
    uint32_t w[2 * BPP];                                   // 8 pixels: 24 or 32 bytes
    load_run<2 * BPP>(src + (long long)r * pitch + (long long)x0 * BPP, n * BPP, n == 8, w);
    uint32_t o[6] = {};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t px = BPP == 4 ? w[i] : px24(w, i);
        put_px(o, i, (px >> bsh) & 0xffu, (px >> gsh) & 0xffu, (px >> rsh) & 0xffu);
    }
    store_run<StoreRule::BY_ADDRESS>(bgr + ((size_t)r * W + x0) * 3, n, o);
}

}  // namespace

int fm_hwc_to_bgr(const uint8_t* src, long long pitch, uint8_t* bgr, int w, int h, int format, hipStream_t s) {
    FM_CHECK_ARG(src && bgr && w >= 1 && h >= 1 && w <= FM_SRC_MAX_DIM && h <= FM_SRC_MAX_DIM && format >= FM_PACKED_RGB &&
                 format <= FM_PACKED_XBGR);
    // byte offsets of R, G, B in a pixel of FM_PACKED_RGB, _BGR, _RGBX, _BGRX, _XRGB, _XBGR
    static const int OFF[6][3] = {{0, 1, 2}, {2, 1, 0}, {0, 1, 2}, {2, 1, 0}, {1, 2, 3}, {3, 2, 1}};
    const int* const off = OFF[format];
    const unsigned threads = (unsigned)((w + 7) >> 3) * (unsigned)h;
    const dim3 grid((threads + 255) / 256), block(256);
    if (format <= FM_PACKED_BGR)
        hipLaunchKernelGGL(hwc_to_bgr_kernel<3>, grid, block, 0, s, src, pitch, bgr, w, h, 8 * off[0], 8 * off[1], 8 * off[2]);
    else
        hipLaunchKernelGGL(hwc_to_bgr_kernel<4>, grid, block, 0, s, src, pitch, bgr, w, h, 8 * off[0], 8 * off[1], 8 * off[2]);
    FM_HIP(hipGetLastError());
    return 0;
}
