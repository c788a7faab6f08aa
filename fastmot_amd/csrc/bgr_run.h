// The 8-pixel BGR run: what every frame converter ends in (nv12.hip, yuv.hip, packed.hip, hwc.hip, deep.hip, devsrc.hip,
// bayer.hip, jpeg.hip, resize.hip, remap.hip).  A thread owns n <= 8 horizontally adjacent pixels of a row, packs their
// 3 n <= 24 BGR bytes into six 32-bit words and stores them; most read their source as runs of bytes too.  A run in
// registers is always little-endian: byte k of it is bits 8 * (k & 3) of word k >> 2.
//
// Threads are numbered along a row first (run_of), 256 a workgroup, so a wavefront reads and writes contiguous bytes;
// no address depends on a pixel's value.
#pragma once
#include "common.h"

// thread id -> row r, first pixel x0 and pixel count n of its run; false for the threads past the frame.  `rows`: rows of
// runs -- row pairs for the kernels whose threads own two rows.  (W and rows are at most FM_SRC_MAX_DIM: 2^11 runs a row,
// 2^25 threads -- or the launcher has checked runs * rows < 2^31 --, so 32 bits do: a 64-bit division is a subroutine.)
__device__ __forceinline__ bool run_of(int W, int rows, int& r, int& x0, int& n) {
    const unsigned nbx = (unsigned)(W + 7) >> 3;
    const unsigned id = blockIdx.x * 256u + threadIdx.x;
    if (id >= nbx * (unsigned)rows) return false;
    r = (int)(id / nbx);
    x0 = (int)(id - (unsigned)r * nbx) * 8;
    n = min(8, W - x0);
    return true;
}

// v (0 .. 255) into byte k of a run that holds zeros there; byte i / 16-bit word i of a run
template <int NW>
__device__ __forceinline__ void put_byte(uint32_t (&w)[NW], int k, uint32_t v) { w[k >> 2] |= v << ((k & 3) * 8); }
template <int NW>
__device__ __forceinline__ uint32_t run_byte(const uint32_t (&w)[NW], int i) { return (w[i >> 2] >> ((i & 3) * 8)) & 0xffu; }
template <int NW>
__device__ __forceinline__ uint32_t run_word16(const uint32_t (&w)[NW], int i) { return (w[i >> 1] >> ((i & 1) * 16)) & 0xffffu; }

// pixel i of a run of 3-byte pixels: the 24 bits from bit 24 i of the run (bits 24 .. 31 of the result are the next
// pixel's, or absent)
template <int NW>
__device__ __forceinline__ uint32_t px24(const uint32_t (&w)[NW], int i) {
    const int word = (24 * i) >> 5, sh = (24 * i) & 31;
    uint32_t px = w[word] >> sh;
    if (sh > 8) px |= w[word + 1] << (32 - sh);
    return px;
}

// pixel i's B, G, R (each 0 .. 255) into bytes 3 i .. 3 i + 2 of the run `o`, which began as zeros
__device__ __forceinline__ void put_px(uint32_t (&o)[6], int i, uint32_t b, uint32_t g, uint32_t r) {
    const uint32_t px[3] = {b, g, r};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) put_byte(o, 3 * i + ch, px[ch]);
}

// How a kernel stores its runs.  ALIGNED8: the launcher has seen W % 8 == 0 and an 8-byte aligned frame -- every run is
// whole and 8-byte aligned: three 8-byte stores, 24 bytes apart (the three together fill every cache line they touch).
// BY_ADDRESS: decided per thread -- three 8-byte stores where the run is whole and its first byte 8-byte aligned, six
// 4-byte stores where it is 4-byte aligned, bytes otherwise; the address depends on 3 W, the row and the frame's base
// only, so odd widths cost just the rows and the ragged last thread they touch.  BYTES: the first 3 n bytes, one by one.
enum class StoreRule { ALIGNED8, BY_ADDRESS, BYTES };

// the 3 n <= 24 BGR bytes of the run `o` to `out`; never a byte outside [out, out + 3 n)
template <StoreRule RULE>
__device__ __forceinline__ void store_run(uint8_t* __restrict__ out, int n, const uint32_t (&o)[6]) {
    if (RULE == StoreRule::ALIGNED8 || (RULE == StoreRule::BY_ADDRESS && n == 8 && !((uintptr_t)out & 7))) {
#pragma unroll
        for (int q = 0; q < 3; ++q) reinterpret_cast<uint2*>(out)[q] = make_uint2(o[2 * q], o[2 * q + 1]);
    } else if (RULE == StoreRule::BY_ADDRESS && n == 8 && !((uintptr_t)out & 3)) {
#pragma unroll
        for (int q = 0; q < 6; ++q) reinterpret_cast<uint32_t*>(out)[q] = o[q];
    } else {
#pragma unroll
        for (int k = 0; k < 24; ++k)
            if (k < 3 * n) out[k] = (uint8_t)(o[k >> 2] >> ((k & 3) * 8));
    }
}

// NW words of a run of `bytes` <= 4 NW bytes at p, the bytes past the run zero.  `whole`: the run has all its 4 NW bytes,
// and only then is anything wider than a byte loaded -- 16-, 8-, 4- or 2-byte loads by the address; never a byte outside
// [p, p + bytes).
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
    } else if (NW % 2 == 0 && whole && !((uintptr_t)p & 7)) {
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
            if (k < bytes) put_byte(w, k, p[k]);
    }
}
