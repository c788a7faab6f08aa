// Frames that lie in device memory already -> packed BGR u8: the kernels behind fm_frame_upload_device /
// fm_frame_upload_ahead_device / fm_frame_ring_store_device (frames.hip), and fm_frame_device_check, the
// host-only part of their argument check.  There is no staging and no copy: a kernel reads the producer's memory where
// it lies -- a torch / CuPy tensor or a view of one, a decoder's NV12 surface -- and writes the BGR frame every consumer
// reads (fastmot_amd/utils/devarray.py to_bgr states the four conversions in numpy, tests compare bit for bit):
//   HWC u8, 3 or 4 bytes per pixel: a byte permutation (six channel orders) -- hwc.hip's kernel, shared with packed.hip
//   CHW u8: three planes, a channel permutation
//   CHW f16 / f32: v = (float)x * scale (one float32 multiply; the library is built with -ffp-contract=off and nothing
//       stands next to it that could fuse), rintf (half to even), NaN -> 0, clamp to 0..255
//   NV12: nv12.hip's kernel, a pitch per plane
//
// The source is somebody else's memory: its planes begin at any element and their rows lie any pitch apart, so nothing
// but the element size is known about an address.  One thread owns 8 pixels of a row (NV12: of two rows) -- a
// wavefront reads 512 B .. 2 KiB of contiguous bytes per row and plane and writes 1536 -- and decides per run, from the
// run's address, how it loads (bgr_run.h load_run: one or two 16-byte loads, 8-byte loads, 4-byte loads, 2-byte loads
// or bytes).  For a contiguous tensor from an allocator the wide path is taken by every thread but the
// ragged last of a row; for a view at an odd offset every thread takes elements, and the bytes a wavefront asks for are
// contiguous all the same.  Stores are bgr_run.h's StoreRule::BY_ADDRESS.
// No address depends on a pixel; every load lies inside the row the description names (a vector load only where the
// run is whole), which fm_frame_*_device have checked against the allocation.
//
// Streaming kernels (4.5 to 15 bytes per pixel): no LDS, no reuse.
#include <hip/hip_fp16.h>
#include "common.h"
#include "bgr_run.h"

namespace {

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
    for (int i = 0; i < 8; ++i) put_px(o, i, run_byte(b, i), run_byte(g, i), run_byte(d, i));
    store_run<StoreRule::BY_ADDRESS>(bgr + ((size_t)r * W + x0) * 3, n, o);
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
    for (int i = 0; i < 8; ++i) put_byte(q, i, quantise(__uint_as_float(w[i]), scale));
}
__device__ __forceinline__ void load_quantised(const __half* __restrict__ p, int n, float scale, uint32_t (&q)[2]) {
    uint32_t w[4];
    load_run<4>(reinterpret_cast<const uint8_t*>(p), 2 * n, n == 8, w);
    q[0] = q[1] = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float x = __half2float(__ushort_as_half((unsigned short)run_word16(w, i)));
        put_byte(q, i, quantise(x, scale));
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
    for (int i = 0; i < 8; ++i) put_px(o, i, run_byte(b, i), run_byte(g, i), run_byte(d, i));
    store_run<StoreRule::BY_ADDRESS>(bgr + ((size_t)r * W + x0) * 3, n, o);
}

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
    const uint8_t* const p0 = static_cast<const uint8_t*>(f->plane[0]);
    if (f->layout == FM_DEV_HWC) return fm_hwc_to_bgr(p0, (long long)f->pitch[0], bgr, w, h, f->format, s);
    if (f->layout == FM_DEV_NV12)
        return fm_nv12_planes_to_bgr(p0, static_cast<const uint8_t*>(f->plane[1]), (long long)f->pitch[0], (long long)f->pitch[1], bgr, w, h,
                                     f->matrix, s);
    const long long threads = (long long)((w + 7) >> 3) * h;
    const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
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
    FM_HIP(hipGetLastError());
    return 0;
}
