// Packed 4:2:2 (YUY2 / UYVY / YVYU) and packed RGB (any channel order, 3 or 4 bytes per pixel) -> packed BGR u8: the
// kernels behind fm_frame_upload_packed / fm_frame_upload_ahead_packed / fm_frame_ring_store_packed (frames.hip).
// Packed 4:2:2 is what UVC / V4L2 cameras and capture cards deliver, RGB what image libraries hand out, BGRx
// what `nvvidconv` / `appsink` do.  The frame arrives in device staging with its rows packed to their byte width
// (4 * ceil(W / 2), 3 W or 4 W) and leaves as the BGR frame every consumer reads.
//
// 4:2:2: one 4-byte macropixel carries Y0, Y1 and the U, V both pixels use; nv12.hip's arithmetic per pixel (yuv_coef.h)
// for the two limited-range matrices, and for the two full-range ones the same expression with a luma offset of 0 and a
// luma factor of 1 << 20, which is  y = Y << 20  (fastmot_amd/utils/packed.py states all of it in numpy, tests compare
// bit for bit).  Full range fits 32 bits as limited range does: 255 * 2^20 + 2^19 + 128 * 1945738 < 2^29.
// RGB: a byte permutation; a fourth byte is dropped.
//
// One thread owns 8 pixels of one row: 16 (4:2:2), 24 or 32 (RGB) bytes in, 24 BGR bytes out.  Threads are numbered
// along a row first, so a wavefront reads 1 (1.5, 2) KiB of contiguous bytes per row and writes 1536.  Loads: macropixels
// and 4-byte pixels lie 4-byte aligned whatever W is (the staging is hipMalloc'ed, the row width a multiple of 4), so
// a whole run is one (two) 16-byte loads where the row begins 16-byte aligned and 4-byte loads otherwise; 3-byte pixels
// take yuv.hip's load_run rule: 8-byte loads, 4-byte loads or bytes by the run's address (a 24-byte run is 16-byte
// aligned in every other thread only: a 16 + 8 split would issue more load instructions per wavefront, not fewer).
// Stores: three 8-byte stores where the run is whole and its first byte 8-byte aligned, six 4-byte stores where it is
// 4-byte aligned, bytes otherwise -- decided per thread from the address, which depends on 3 W, the row and the frame's
// base only, so odd widths cost just the rows and the ragged last thread they touch.  No address depends on a pixel.
//
// Both are streaming kernels (5, 6 or 7 bytes per pixel): no LDS, no reuse beyond a macropixel's chroma in registers.
#include "common.h"
#include "yuv_coef.h"

namespace {

// FM_PACKED_BT601_FULL / FM_PACKED_BT709_FULL: round(coef * 2^20) of 1.402, 1.772, -0.344136, -0.714136 and of
// 1.5748, 1.8556, -0.187324, -0.468124 (CVR, CUB, CUG, CVG); the luma factor 1 << 20 goes with a luma offset of 0
constexpr Nv12Coef PACKED_FULL_COEF[2] = {
    {1 << NV12_SHIFT, 1470104, 1858077, -360853, -748826},
    {1 << NV12_SHIFT, 1651297, 1945738, -196423, -490864},
};

// the 3 n <= 24 BGR bytes of a thread's run (byte k: word k >> 2, bits 8 * (k & 3)) to `out`
__device__ __forceinline__ void store_run(uint8_t* __restrict__ out, int n, const uint32_t (&o)[6]) {
    if (n == 8 && !((uintptr_t)out & 7)) {
#pragma unroll
        for (int q = 0; q < 3; ++q) reinterpret_cast<uint2*>(out)[q] = make_uint2(o[2 * q], o[2 * q + 1]);
    } else if (n == 8 && !((uintptr_t)out & 3)) {
#pragma unroll
        for (int q = 0; q < 6; ++q) reinterpret_cast<uint32_t*>(out)[q] = o[q];
    } else {
#pragma unroll
        for (int k = 0; k < 24; ++k)
            if (k < 3 * n) out[k] = (uint8_t)(o[k >> 2] >> ((k & 3) * 8));
    }
}

__device__ __forceinline__ void put_px(uint32_t (&o)[6], int i, uint32_t b, uint32_t g, uint32_t r) {
    const uint32_t px[3] = {b, g, r};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int k = 3 * i + ch;                          // byte of the 24-byte row segment
        o[k >> 2] |= px[ch] << ((k & 3) * 8);
    }
}

// src: H rows of rb = 4 * ceil(W / 2) bytes, 4-byte aligned.  ysh / ush / vsh: the bit a macropixel's Y0 / U / V begins
// at when it is read as one little-endian word (Y1 lies 16 bits above Y0); yoff: 16 (limited range) or 0.
__global__ __launch_bounds__(256) void packed422_to_bgr_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ bgr, int W, int H,
                                                               int rb, int ysh, int ush, int vsh, int yoff, Nv12Coef c) {
    const int nbx = (W + 7) >> 3;
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long long)nbx * H) return;
    const int r = (int)(id / nbx), x0 = (int)(id - (long long)r * nbx) * 8;
    const int n = min(8, W - x0);                          // pixels of this thread's run
    const int nm = (n + 1) >> 1;                           // macropixels under it
    const uint8_t* const p = src + (size_t)r * rb + (size_t)x0 * 2;

    uint32_t m[4] = {0, 0, 0, 0};
    if (nm == 4 && !((uintptr_t)p & 15)) {
        const uint4 a = *reinterpret_cast<const uint4*>(p);
        m[0] = a.x, m[1] = a.y, m[2] = a.z, m[3] = a.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nm) m[j] = reinterpret_cast<const uint32_t*>(p)[j];
    }

    uint32_t o[6] = {};
    constexpr int half = 1 << (NV12_SHIFT - 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int u = (int)((m[j] >> ush) & 0xffu) - 128, v = (int)((m[j] >> vsh) & 0xffu) - 128;
        const int cb = half + c.cub * u, cg = half + c.cvg * v + c.cug * u, cr = half + c.cvr * v;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int y = max((int)((m[j] >> (ysh + 16 * t)) & 0xffu) - yoff, 0) * c.cy;
            put_px(o, 2 * j + t, sat8(y + cb), sat8(y + cg), sat8(y + cr));
        }
    }
    store_run(bgr + ((size_t)r * W + x0) * 3, n, o);
}

// src: H rows of rb = BPP * W bytes.  rsh / gsh / bsh: the bit R / G / B begins at in a pixel read as one little-endian word.
template <int BPP>
__global__ __launch_bounds__(256) void packed_rgb_to_bgr_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ bgr, int W, int H,
                                                                int rb, int rsh, int gsh, int bsh) {
    const int nbx = (W + 7) >> 3;
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long long)nbx * H) return;
    const int r = (int)(id / nbx), x0 = (int)(id - (long long)r * nbx) * 8;
    const int n = min(8, W - x0);
    const uint8_t* const p = src + (size_t)r * rb + (size_t)x0 * BPP;

    uint32_t px[8] = {};
    if (BPP == 4) {                                        // (p is 4-byte aligned)
        if (n == 8 && !((uintptr_t)p & 15)) {
            const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
            px[0] = a.x, px[1] = a.y, px[2] = a.z, px[3] = a.w, px[4] = b.x, px[5] = b.y, px[6] = b.z, px[7] = b.w;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (i < n) px[i] = reinterpret_cast<const uint32_t*>(p)[i];
        }
    } else {
        uint32_t w[6] = {};
        if (n == 8 && !((uintptr_t)p & 7)) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint2 a = reinterpret_cast<const uint2*>(p)[q];
                w[2 * q] = a.x, w[2 * q + 1] = a.y;
            }
        } else if (n == 8 && !((uintptr_t)p & 3)) {
#pragma unroll
            for (int q = 0; q < 6; ++q) w[q] = reinterpret_cast<const uint32_t*>(p)[q];
        } else {
#pragma unroll
            for (int k = 0; k < 24; ++k)
                if (k < 3 * n) w[k >> 2] |= (uint32_t)p[k] << ((k & 3) * 8);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {                      // pixel i: the 24 bits from bit 24 i of the run
            const int word = (24 * i) >> 5, sh = (24 * i) & 31;
            px[i] = w[word] >> sh;
            if (sh > 8) px[i] |= w[word + 1] << (32 - sh);
        }
    }

    uint32_t o[6] = {};
#pragma unroll
    for (int i = 0; i < 8; ++i) put_px(o, i, (px[i] >> bsh) & 0xffu, (px[i] >> gsh) & 0xffu, (px[i] >> rsh) & 0xffu);
    store_run(bgr + ((size_t)r * W + x0) * 3, n, o);
}

}  // namespace

// Converts the packed frame at `src` (h rows of fm_packed_row_bytes(w, format) bytes, 4-byte aligned) to w * h * 3 BGR
// bytes at `bgr`, on stream `s`.  The callers have checked the arguments.
int fm_packed_to_bgr(const uint8_t* src, uint8_t* bgr, int w, int h, int format, int matrix, hipStream_t s) {
    const size_t rb = fm_packed_row_bytes(w, format);
    FM_CHECK_ARG(src && bgr && w >= 1 && h >= 1 && w <= FM_SRC_MAX_DIM && h <= FM_SRC_MAX_DIM && rb && fm_packed_matrix_ok(matrix) &&
                 !((uintptr_t)src & 3));
    const long long threads = (long long)((w + 7) >> 3) * h;
    const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
    if (format >= FM_PACKED_YUY2) {
        const bool full = matrix >= FM_PACKED_BT601_FULL;
        const Nv12Coef& c = full ? PACKED_FULL_COEF[matrix - FM_PACKED_BT601_FULL] : NV12_COEF[matrix];
        const int ysh = format == FM_PACKED_UYVY ? 8 : 0;
        const int ush = format == FM_PACKED_YUY2 ? 8 : format == FM_PACKED_UYVY ? 0 : 24;
        const int vsh = format == FM_PACKED_YUY2 ? 24 : format == FM_PACKED_UYVY ? 16 : 8;
        hipLaunchKernelGGL(packed422_to_bgr_kernel, grid, block, 0, s, src, bgr, w, h, (int)rb, ysh, ush, vsh, full ? 0 : 16, c);
    } else {
        // byte offsets of R, G, B in a pixel
        static const int OFF[6][3] = {{0, 1, 2}, {2, 1, 0}, {0, 1, 2}, {2, 1, 0}, {1, 2, 3}, {3, 2, 1}};
        const int* const off = OFF[format];
        if (format <= FM_PACKED_BGR)
            hipLaunchKernelGGL(packed_rgb_to_bgr_kernel<3>, grid, block, 0, s, src, bgr, w, h, (int)rb, 8 * off[0], 8 * off[1], 8 * off[2]);
        else
            hipLaunchKernelGGL(packed_rgb_to_bgr_kernel<4>, grid, block, 0, s, src, bgr, w, h, (int)rb, 8 * off[0], 8 * off[1], 8 * off[2]);
    }
    FM_HIP(hipGetLastError());
    return 0;
}
