// Frames that lie in device memory already -> packed BGR u8: the kernels behind fm_frame_upload_device /
// fm_frame_upload_ahead_device / fm_frame_ring_store_device (frames.hip), and fm_frame_device_check, the
// host-only part of their argument check.  There is no staging and no copy: a kernel reads the producer's memory where
// it lies -- a torch / CuPy tensor or a view of one, a decoder's NV12 surface -- and writes the BGR frame every consumer
// reads (fastmot_amd/utils/devarray.py to_bgr states the four conversions in numpy, tests compare bit for bit):
//   HWC u8, 3 or 4 bytes per pixel: packed.hip's byte permutation (six channel orders)
//   CHW u8: three planes, a channel permutation
//   CHW f16 / f32: v = (float)x * scale (one float32 multiply; the library is built with -ffp-contract=off and nothing
//       stands next to it that could fuse), rintf (half to even), NaN -> 0, clamp to 0..255
//   NV12: nv12.hip's integer arithmetic (yuv_coef.h), a pitch per plane
//
// The source is somebody else's memory: its planes begin at any element and their rows lie any pitch apart, so nothing
// but the element size is known about an address.  One thread owns 8 pixels of a row (NV12: of two rows), as in
// packed.hip and nv12.hip -- a wavefront reads 512 B .. 2 KiB of contiguous bytes per row and plane and writes 1536 --
// and decides per run, from the run's address, how it loads: one or two 16-byte loads, 8-byte loads, 4-byte loads,
// 2-byte loads or bytes.  For a contiguous tensor from an allocator the wide path is taken by every thread but the
// ragged last of a row; for a view at an odd offset every thread takes elements, and the bytes a wavefront asks for are
// contiguous all the same.  Stores follow packed.hip's rule (8-byte, 4-byte or bytes by the address of the run's first byte).
// No address depends on a pixel; every load lies inside the row the description names (a vector load only where the
// run is whole), which fm_frame_*_device have checked against the allocation.
//
// Streaming kernels (4.5 to 15 bytes per pixel): no LDS, no reuse.
#include <hip/hip_fp16.h>
#include "common.h"
#include "yuv_coef.h"      // Nv12Coef, NV12_COEF, NV12_SHIFT, sat8 (shared with nv12.hip, yuv.hip, packed.hip)

namespace {

// the 3 n <= 24 BGR bytes of a thread's run (byte k: word k >> 2, bits 8 * (k & 3)) to `out`: packed.hip's store rule
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

// NW words of a run of `bytes` <= 4 NW bytes at p (byte k: word k >> 2, bits 8 * (k & 3)); `whole`: the run has all
// its 4 NW bytes, and only then is anything wider than a byte loaded
template <int NW>
__device__ __forceinline__ void load_run(const uint8_t* __restrict__ p, int bytes, bool whole, uint32_t (&w)[NW]) {
#pragma unroll
    for (int q = 0; q < NW; ++q) w[q] = 0;
    if (NW % 4 == 0 && whole && !((uintptr_t)p & 15)) {
#pragma unroll
        for (int q = 0; q < NW / 4; ++q) {
            const uint4 a = reinterpret_cast<const uint4*>(p)[q];
            w[4 * q] = a.x, w[4 * q + 1] = a.y, w[4 * q + 2] = a.z, w[4 * q + 3] = a.w;
        }
    } else if (whole && !((uintptr_t)p & 7)) {
#pragma unroll
        for (int q = 0; q < NW / 2; ++q) {
            const uint2 a = reinterpret_cast<const uint2*>(p)[q];
            w[2 * q] = a.x, w[2 * q + 1] = a.y;
        }
    } else if (whole && !((uintptr_t)p & 3)) {
#pragma unroll
        for (int q = 0; q < NW; ++q) w[q] = reinterpret_cast<const uint32_t*>(p)[q];
    } else if (whole && !((uintptr_t)p & 1)) {
#pragma unroll
        for (int q = 0; q < 2 * NW; ++q) w[q >> 1] |= (uint32_t)reinterpret_cast<const uint16_t*>(p)[q] << ((q & 1) * 16);
    } else {
#pragma unroll
        for (int k = 0; k < 4 * NW; ++k)
            if (k < bytes) w[k >> 2] |= (uint32_t)p[k] << ((k & 3) * 8);
    }
}
#define DEV_BYTE(w, i) (((w)[(i) >> 2] >> (((i) & 3) * 8)) & 0xffu)

// thread id -> row r, first pixel x0 and pixel count n of its run; false for the threads past the frame.  (W and rows are
// at most FM_SRC_MAX_DIM: 2^11 runs a row, 2^25 threads, so 32 bits do -- a 64-bit division is a subroutine.)
__device__ __forceinline__ bool run_of(int W, int rows, int& r, int& x0, int& n) {
    const unsigned nbx = (unsigned)(W + 7) >> 3;
    const unsigned id = blockIdx.x * 256u + threadIdx.x;
    if (id >= nbx * (unsigned)rows) return false;
    r = (int)(id / nbx);
    x0 = (int)(id - (unsigned)r * nbx) * 8;
    n = min(8, W - x0);
    return true;
}

// src: H rows of BPP * W bytes, `pitch` bytes apart.  rsh / gsh / bsh: the bit R / G / B begins at in a pixel read as one
// little-endian word.
template <int BPP>
__global__ __launch_bounds__(256) void dev_hwc_to_bgr_kernel(const uint8_t* __restrict__ src, long long pitch, uint8_t* __restrict__ bgr,
                                                             int W, int H, int rsh, int gsh, int bsh) {
    int r, x0, n;
    if (!run_of(W, H, r, x0, n)) return;
    uint32_t w[2 * BPP];                                   // 8 pixels: 24 or 32 bytes
    load_run<2 * BPP>(src + (long long)r * pitch + (long long)x0 * BPP, n * BPP, n == 8, w);
    uint32_t o[6] = {};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint32_t px;
        if (BPP == 4) {
            px = w[i];
        } else {                                           // pixel i: the 24 bits from bit 24 i of the run
            const int word = (24 * i) >> 5, sh = (24 * i) & 31;
            px = w[word] >> sh;
            if (sh > 8) px |= w[word + 1] << (32 - sh);
        }
        put_px(o, i, (px >> bsh) & 0xffu, (px >> gsh) & 0xffu, (px >> rsh) & 0xffu);
    }
    store_run(bgr + ((size_t)r * W + x0) * 3, n, o);
}

// pb / pg / pr: the B, G and R planes, H rows of W bytes, sb / sg / sr bytes apart
__global__ __launch_bounds__(256) void dev_chw_u8_to_bgr_kernel(const uint8_t* __restrict__ pb, const uint8_t* __restrict__ pg,
                                                                const uint8_t* __restrict__ pr, long long sb, long long sg, long long sr,
                                                                uint8_t* __restrict__ bgr, int W, int H) {
    int r, x0, n;
    if (!run_of(W, H, r, x0, n)) return;
    uint32_t b[2], g[2], d[2];
    load_run<2>(pb + (long long)r * sb + x0, n, n == 8, b);
    load_run<2>(pg + (long long)r * sg + x0, n, n == 8, g);
    load_run<2>(pr + (long long)r * sr + x0, n, n == 8, d);
    uint32_t o[6] = {};
#pragma unroll
    for (int i = 0; i < 8; ++i) put_px(o, i, DEV_BYTE(b, i), DEV_BYTE(g, i), DEV_BYTE(d, i));
    store_run(bgr + ((size_t)r * W + x0) * 3, n, o);
}

// one float sample -> its byte: a float32 multiply, round half to even, NaN -> 0 (every comparison with it is false),
// clamp
__device__ __forceinline__ uint32_t quantise(float x, float scale) {
    const float v = rintf(x * scale);
    return v >= 0.f ? (v <= 255.f ? (uint32_t)v : 255u) : 0u;
}

// the n <= 8 samples of a run at p as bytes (sample i: word i >> 2, bits 8 * (i & 3))
__device__ __forceinline__ void load_quantised(const float* __restrict__ p, int n, float scale, uint32_t (&q)[2]) {
    uint32_t w[8];
    load_run<8>(reinterpret_cast<const uint8_t*>(p), 4 * n, n == 8, w);      // (p is 4-byte aligned: never the byte path's shifts across samples)
    q[0] = q[1] = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i >> 2] |= quantise(__uint_as_float(w[i]), scale) << ((i & 3) * 8);
}
__device__ __forceinline__ void load_quantised(const __half* __restrict__ p, int n, float scale, uint32_t (&q)[2]) {
    uint32_t w[4];
    load_run<4>(reinterpret_cast<const uint8_t*>(p), 2 * n, n == 8, w);
    q[0] = q[1] = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float x = __half2float(__ushort_as_half((unsigned short)((w[i >> 1] >> ((i & 1) * 16)) & 0xffffu)));
        q[i >> 2] |= quantise(x, scale) << ((i & 3) * 8);
    }
}

// pb / pg / pr: the B, G and R planes, H rows of W samples of T (__half or float), sb / sg / sr BYTES apart
template <typename T>
__global__ __launch_bounds__(256) void dev_chw_float_to_bgr_kernel(const uint8_t* __restrict__ pb, const uint8_t* __restrict__ pg,
                                                                   const uint8_t* __restrict__ pr, long long sb, long long sg, long long sr,
                                                                   uint8_t* __restrict__ bgr, int W, int H, float scale) {
    int r, x0, n;
    if (!run_of(W, H, r, x0, n)) return;
    uint32_t b[2], g[2], d[2];
    load_quantised(reinterpret_cast<const T*>(pb + (long long)r * sb) + x0, n, scale, b);
    load_quantised(reinterpret_cast<const T*>(pg + (long long)r * sg) + x0, n, scale, g);
    load_quantised(reinterpret_cast<const T*>(pr + (long long)r * sr) + x0, n, scale, d);
    uint32_t o[6] = {};
#pragma unroll
    for (int i = 0; i < 8; ++i) put_px(o, i, DEV_BYTE(b, i), DEV_BYTE(g, i), DEV_BYTE(d, i));
    store_run(bgr + ((size_t)r * W + x0) * 3, n, o);
}

// yp: H rows of W luma bytes, sy apart; uvp: H / 2 rows of W interleaved U, V bytes, suv apart; W and H even.  One thread:
// 8 pixels of two rows and the chroma row they share -- nv12.hip's block and, per pixel, its arithmetic.
__global__ __launch_bounds__(256) void dev_nv12_to_bgr_kernel(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ uvp, long long sy,
                                                              long long suv, uint8_t* __restrict__ bgr, int W, int H, Nv12Coef c) {
    int by, x0, n;
    if (!run_of(W, H >> 1, by, x0, n)) return;
    uint32_t yw[2][2], uvw[2];
    const uint8_t* const y0 = yp + (long long)(2 * by) * sy + x0;
    load_run<2>(y0, n, n == 8, yw[0]);
    load_run<2>(y0 + sy, n, n == 8, yw[1]);
    load_run<2>(uvp + (long long)by * suv + x0, n, n == 8, uvw);

    uint32_t o[2][6] = {};
    constexpr int half = 1 << (NV12_SHIFT - 1);
#pragma unroll
    for (int p = 0; p < 4; ++p) {                           // chroma pair p: pixels 2p, 2p + 1 of both rows
        const int u = (int)DEV_BYTE(uvw, 2 * p) - 128, v = (int)DEV_BYTE(uvw, 2 * p + 1) - 128;
        const int cb = half + c.cub * u, cg = half + c.cvg * v + c.cug * u, cr = half + c.cvr * v;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int i = 2 * p + j;
                const int y = max((int)DEV_BYTE(yw[r], i) - 16, 0) * c.cy;
                put_px(o[r], i, sat8(y + cb), sat8(y + cg), sat8(y + cr));
            }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) store_run(bgr + ((size_t)(2 * by + r) * W + x0) * 3, n, o[r]);
}
#undef DEV_BYTE

}  // namespace

// The geometry of a device frame's description: everything that can be said without asking the runtime about the
// pointers (the entry points in frames.hip do that next).  Host code only.
extern "C" int fm_frame_device_check(const struct fm_frame_device* f) {
    FM_CHECK_ARG(f != nullptr);
    FM_CHECK_ARG(f->width >= 1 && f->height >= 1 && f->width <= FM_SRC_MAX_DIM && f->height <= FM_SRC_MAX_DIM);
    FM_CHECK_ARG(f->layout == FM_DEV_HWC || f->layout == FM_DEV_CHW || f->layout == FM_DEV_NV12);
    FM_CHECK_ARG(f->dtype == FM_DEV_U8 || (f->layout == FM_DEV_CHW && (f->dtype == FM_DEV_F16 || f->dtype == FM_DEV_F32)));
    if (f->layout == FM_DEV_HWC) FM_CHECK_ARG(f->format >= FM_PACKED_RGB && f->format <= FM_PACKED_XBGR);
    if (f->layout == FM_DEV_CHW) FM_CHECK_ARG(f->format == FM_DEV_ORDER_RGB || f->format == FM_DEV_ORDER_BGR);
    if (f->layout == FM_DEV_NV12) {
        FM_CHECK_ARG(f->format == 0 && (f->matrix == FM_NV12_BT601 || f->matrix == FM_NV12_BT709));
        FM_CHECK_ARG(!(f->width & 1) && !(f->height & 1));
    }
    if (f->dtype != FM_DEV_U8) FM_CHECK_ARG(f->scale == 1.0f || f->scale == 255.0f);
    FM_CHECK_ARG(!(f->flags & ~FM_DEV_READY));
    const int np = fm_dev_planes(f->layout), es = fm_dev_elem_bytes(f->dtype);
    const long long rb = (long long)fm_dev_row_bytes(f);
    for (int p = 0; p < 3; ++p) {
        if (p >= np) {
            FM_CHECK_ARG(f->plane[p] == nullptr);
            continue;
        }
        FM_CHECK_ARG(f->plane[p] != nullptr);
        FM_CHECK_ARG(f->pitch[p] >= rb && f->pitch[p] <= (1ll << 40));
        FM_CHECK_ARG(!((uintptr_t)f->plane[p] % es) && !(f->pitch[p] % es));
    }
    return 0;
}

// Converts the device frame `f` to f->width * f->height * 3 BGR bytes at `bgr` on stream `s`.  The callers have checked
// the description (fm_frame_device_check) and the memory behind it.
int fm_device_to_bgr(const struct fm_frame_device* f, uint8_t* bgr, hipStream_t s) {
    FM_CHECK_ARG(bgr);
    int rc = fm_frame_device_check(f);
    if (rc) return rc;
    const int w = f->width, h = f->height;
    const long long threads = (long long)((w + 7) >> 3) * (f->layout == FM_DEV_NV12 ? h >> 1 : h);
    const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
    const uint8_t* const p0 = static_cast<const uint8_t*>(f->plane[0]);
    if (f->layout == FM_DEV_HWC) {
        // byte offsets of R, G, B in a pixel (packed.hip)
        static const int OFF[6][3] = {{0, 1, 2}, {2, 1, 0}, {0, 1, 2}, {2, 1, 0}, {1, 2, 3}, {3, 2, 1}};
        const int* const off = OFF[f->format];
        if (f->format <= FM_PACKED_BGR)
            hipLaunchKernelGGL(dev_hwc_to_bgr_kernel<3>, grid, block, 0, s, p0, (long long)f->pitch[0], bgr, w, h, 8 * off[0], 8 * off[1], 8 * off[2]);
        else
            hipLaunchKernelGGL(dev_hwc_to_bgr_kernel<4>, grid, block, 0, s, p0, (long long)f->pitch[0], bgr, w, h, 8 * off[0], 8 * off[1], 8 * off[2]);
    } else if (f->layout == FM_DEV_CHW) {
        const int ib = f->format == FM_DEV_ORDER_RGB ? 2 : 0, ir = 2 - ib;      // the planes that hold B and R
        const uint8_t* const pb = static_cast<const uint8_t*>(f->plane[ib]);
        const uint8_t* const pg = static_cast<const uint8_t*>(f->plane[1]);
        const uint8_t* const pr = static_cast<const uint8_t*>(f->plane[ir]);
        const long long sb = f->pitch[ib], sg = f->pitch[1], sr = f->pitch[ir];
        if (f->dtype == FM_DEV_U8)
            hipLaunchKernelGGL(dev_chw_u8_to_bgr_kernel, grid, block, 0, s, pb, pg, pr, sb, sg, sr, bgr, w, h);
        else if (f->dtype == FM_DEV_F16)
            hipLaunchKernelGGL(dev_chw_float_to_bgr_kernel<__half>, grid, block, 0, s, pb, pg, pr, sb, sg, sr, bgr, w, h, f->scale);
        else
            hipLaunchKernelGGL(dev_chw_float_to_bgr_kernel<float>, grid, block, 0, s, pb, pg, pr, sb, sg, sr, bgr, w, h, f->scale);
    } else {
        hipLaunchKernelGGL(dev_nv12_to_bgr_kernel, grid, block, 0, s, p0, static_cast<const uint8_t*>(f->plane[1]), (long long)f->pitch[0],
                           (long long)f->pitch[1], bgr, w, h, NV12_COEF[f->matrix]);
    }
    FM_HIP(hipGetLastError());
    return 0;
}
