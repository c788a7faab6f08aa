// NV12 -> packed BGR u8: the conversion behind fm_frame_upload_nv12 / fm_frame_upload_ahead_nv12 /
// fm_frame_ring_store_nv12 (frames.hip).  The frame arrives as 1.5 bytes per pixel in a device staging
// buffer (Y plane W x H, then the interleaved UV plane W x H/2, both packed to rows of W bytes) and leaves as the BGR
// frame that every consumer already reads (pixel_source.h, the ReID crop, the KLT gray conversion), so nothing
// downstream knows where the frame came from.
//
// The arithmetic is integer and exact (fastmot_amd/utils/nv12.py states it in numpy; tests compare bit for bit):
//     y = max(Y - 16, 0) * CY,  u = U - 128,  v = V - 128,  h = 1 << 19
//     R = sat8((y + h + CVR v) >> 20)   G = sat8((y + h + CVG v + CUG u) >> 20)   B = sat8((y + h + CUB u) >> 20)
// with an arithmetic shift and the chroma sample of a 2 x 2 block used for its four pixels.  Every intermediate fits
// 32 bits: 239 * 1220945 + 127 * 2215014 + h < 2^31.
//
// One thread owns 8 pixels x 2 rows: 2 x 8 Y bytes and 8 UV bytes in, 2 x 24 BGR bytes out.  Threads are numbered along
// a row first, so a wavefront reads 512 contiguous Y bytes per row and writes 1536 contiguous BGR bytes per row.  The one
// kernel serves the staged frame (both pitches W) and a decoder's surface in device memory (devsrc.hip: a pitch per
// plane, planes that begin anywhere), so nothing but the address itself is known about a run: loads and stores are
// chosen per thread by bgr_run.h's rules (load_run, StoreRule::BY_ADDRESS) -- for a frame whose width is a multiple
// of 8, staged and written at 8-byte aligned addresses, every thread takes the 8-byte ones.  A streaming kernel at 4.5
// bytes per pixel: no LDS, no reuse beyond the chroma pair a thread holds in registers.
#include "common.h"
#include "bgr_run.h"
#include "yuv_coef.h"

namespace {

// yp: H rows of W luma bytes, sy apart; uvp: H / 2 rows of W interleaved U, V bytes, suv apart; W and H even (so a chroma
// pair is never split).
__global__ __launch_bounds__(256) void nv12_to_bgr_kernel(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ uvp, long long sy,
                                                          long long suv, uint8_t* __restrict__ bgr, int W, int H, Nv12Coef c) {
    int by, x0, n;
    if (!run_of(W, H >> 1, by, x0, n)) return;
    uint32_t yw[2][2], uvw[2];
    const uint8_t* const y0 = yp + (long long)(2 * by) * sy + x0;
    load_run<2>(y0, n, n == 8, yw[0]);
    load_run<2>(y0 + sy, n, n == 8, yw[1]);
    load_run<2>(uvp + (long long)by * suv + x0, n, n == 8, uvw);

    uint32_t o[2][6] = {};
#pragma unroll
    for (int p = 0; p < 4; ++p) {                           // chroma pair p: pixels 2p, 2p + 1 of both rows
        int cb, cg, cr;
        ycc_chroma(c, (int)run_byte(uvw, 2 * p) - 128, (int)run_byte(uvw, 2 * p + 1) - 128, cb, cg, cr);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int i = 2 * p + j;
                uint32_t b, g, d;
                ycc_px(c, (int)run_byte(yw[r], i), 16, cb, cg, cr, b, g, d);
                put_px(o[r], i, b, g, d);
            }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) store_run<StoreRule::BY_ADDRESS>(bgr + ((size_t)(2 * by + r) * W + x0) * 3, n, o[r]);
}

}  // namespace

// Converts the NV12 frame whose Y rows lie `sy` bytes apart from `y` and whose UV rows `suv` bytes apart from `uv` (device
// memory, any alignment) to w * h * 3 BGR bytes at `bgr`, on stream `s`.  w and h even, matrix FM_NV12_BT601 / FM_NV12_BT709.
int fm_nv12_planes_to_bgr(const uint8_t* y, const uint8_t* uv, long long sy, long long suv, uint8_t* bgr, int w, int h, int matrix,
                          hipStream_t s) {
    FM_CHECK_ARG(y && uv && bgr && w > 0 && h > 0 && !(w & 1) && !(h & 1) && (matrix == FM_NV12_BT601 || matrix == FM_NV12_BT709));
    const long long blocks = (long long)((w + 7) >> 3) * (h >> 1);
    FM_CHECK_ARG(blocks < (1ll << 31) - 256);
    const dim3 grid((unsigned)((blocks + 255) / 256));
    hipLaunchKernelGGL(nv12_to_bgr_kernel, grid, dim3(256), 0, s, y, uv, sy, suv, bgr, w, h, NV12_COEF[matrix]);
    FM_HIP(hipGetLastError());
    return 0;
}

// Converts the packed NV12 frame at `nv12` (Y: w * h bytes, then UV: w * h / 2 bytes) to w * h * 3 BGR bytes at `bgr`,
// on stream `s`.  w and h even, matrix FM_NV12_BT601 / FM_NV12_BT709 (the callers have checked).
int fm_nv12_to_bgr(const uint8_t* nv12, uint8_t* bgr, int w, int h, int matrix, hipStream_t s) {
    FM_CHECK_ARG(nv12 && w > 0 && h > 0);
    return fm_nv12_planes_to_bgr(nv12, nv12 + (size_t)w * h, w, w, bgr, w, h, matrix, s);
}
