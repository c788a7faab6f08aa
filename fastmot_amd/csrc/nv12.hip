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
// a row first, so a wavefront reads 512 contiguous Y bytes per row and writes 1536 contiguous BGR bytes per row (three
// 8-byte stores per thread, 24 bytes apart: the three together fill every cache line they touch).  A streaming
// kernel at 4.5 bytes per pixel: no LDS, no reuse beyond the chroma pair a thread holds in registers.
#include "common.h"
#include "yuv_coef.h"      // Nv12Coef, NV12_COEF, NV12_SHIFT, sat8 (shared with yuv.hip)

namespace {

// VEC: W % 8 == 0 -- every access is an aligned 8-byte load / store.  Otherwise bytes, with the row's end checked per
// pixel pair (W is even, so a chroma pair is never split).
template <bool VEC>
__global__ __launch_bounds__(256) void nv12_to_bgr_kernel(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ uvp,
                                                          uint8_t* __restrict__ bgr, int W, int H, Nv12Coef c) {
    const int nbx = (W + 7) >> 3;
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= nbx * (H >> 1)) return;
    const int by = id / nbx, bx = id - by * nbx;
    const int x0 = bx * 8;
    const size_t row0 = (size_t)(2 * by) * W + x0;          // first Y byte of the block; the BGR block starts at 3 * row0
    const uint8_t* const uvrow = uvp + (size_t)by * W + x0;

    uint32_t yw[2][2] = {}, uvw[2] = {};                    // bytes i of the block: word i >> 2, bits 8 * (i & 3)
    if (VEC) {
        const uint2 a = *reinterpret_cast<const uint2*>(yp + row0);
        const uint2 b = *reinterpret_cast<const uint2*>(yp + row0 + W);
        const uint2 q = *reinterpret_cast<const uint2*>(uvrow);
        yw[0][0] = a.x, yw[0][1] = a.y, yw[1][0] = b.x, yw[1][1] = b.y, uvw[0] = q.x, uvw[1] = q.y;
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (x0 + i < W) {
                const int sh = (i & 3) * 8;
                yw[0][i >> 2] |= (uint32_t)yp[row0 + i] << sh;
                yw[1][i >> 2] |= (uint32_t)yp[row0 + W + i] << sh;
                uvw[i >> 2] |= (uint32_t)uvrow[i] << sh;
            }
    }
#define NV12_BYTE(w, i) ((int)(((w)[(i) >> 2] >> (((i) & 3) * 8)) & 0xffu))

    uint32_t o[2][6] = {};
    constexpr int half = 1 << (NV12_SHIFT - 1);
#pragma unroll
    for (int p = 0; p < 4; ++p) {                           // chroma pair p: pixels 2p, 2p + 1 of both rows
        const int u = NV12_BYTE(uvw, 2 * p) - 128, v = NV12_BYTE(uvw, 2 * p + 1) - 128;
        const int cb = half + c.cub * u, cg = half + c.cvg * v + c.cug * u, cr = half + c.cvr * v;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int i = 2 * p + j;
                const int y = max(NV12_BYTE(yw[r], i) - 16, 0) * c.cy;
                const uint32_t px[3] = {sat8(y + cb), sat8(y + cg), sat8(y + cr)};
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const int k = 3 * i + ch;               // byte of the 24-byte row segment
                    o[r][k >> 2] |= px[ch] << ((k & 3) * 8);
                }
            }
    }

#pragma unroll
    for (int r = 0; r < 2; ++r) {
        uint8_t* const out = bgr + 3 * (row0 + (size_t)r * W);
        if (VEC) {
#pragma unroll
            for (int q = 0; q < 3; ++q) reinterpret_cast<uint2*>(out)[q] = make_uint2(o[r][2 * q], o[r][2 * q + 1]);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (x0 + i < W) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const int k = 3 * i + ch;
                        out[k] = (uint8_t)(o[r][k >> 2] >> ((k & 3) * 8));
                    }
                }
        }
    }
}
#undef NV12_BYTE

}  // namespace

// Converts the packed NV12 frame at `nv12` (Y: w * h bytes, then UV: w * h / 2 bytes) to w * h * 3 BGR bytes at `bgr`,
// on stream `s`.  w and h even, matrix FM_NV12_BT601 / FM_NV12_BT709 (the callers have checked); `nv12` and `bgr`
// 8-byte aligned (hipMalloc'ed buffers and whole frames of the ring are).
int fm_nv12_to_bgr(const uint8_t* nv12, uint8_t* bgr, int w, int h, int matrix, hipStream_t s) {
    FM_CHECK_ARG(nv12 && bgr && w > 0 && h > 0 && !(w & 1) && !(h & 1) && (matrix == FM_NV12_BT601 || matrix == FM_NV12_BT709));
    const long long blocks = (long long)((w + 7) >> 3) * (h >> 1);
    FM_CHECK_ARG(blocks < (1ll << 31) - 256);
    const uint8_t* const uv = nv12 + (size_t)w * h;
    const dim3 grid((unsigned)((blocks + 255) / 256));
    if (w % 8 == 0)
        hipLaunchKernelGGL(nv12_to_bgr_kernel<true>, grid, dim3(256), 0, s, nv12, uv, bgr, w, h, NV12_COEF[matrix]);
    else
        hipLaunchKernelGGL(nv12_to_bgr_kernel<false>, grid, dim3(256), 0, s, nv12, uv, bgr, w, h, NV12_COEF[matrix]);
    FM_HIP(hipGetLastError());
    return 0;
}
