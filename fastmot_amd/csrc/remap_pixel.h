// What a correction map does for one pixel of the frame: the same text for the kernel of remap.hip and for
// fm_remap_bgr_host (remap_host.hip).  fastmot_amd/utils/lens.py remap_bgr states it in numpy; tests compare all three
// bit for bit.
//
// A map entry is a source coordinate in fixed point with FM_REMAP_BITS = 5 fractional bits, X = rint(32 x), Y = rint(32 y),
// X in [-64, 32 (sw + 1)], Y in [-64, 32 (sh + 1)].  With ix = X >> 5 (arithmetic), fx = X & 31 and the same for y, the
// four taps are (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1); a tap outside [0, sw) x [0, sh) contributes the
// border colour's channel, chosen PER TAP, and per channel
//     v = ((32 - fy) ((32 - fx) p00 + fx p01) + fy ((32 - fx) p10 + fx p11) + 512) >> 10
// which is exact in 32 bits (at most 255 * 1024 + 512), needs no clamp, and equals the float64 bilinear value of the
// quantised coordinate rounded half up.
//
// Memory safety lives here, not with whoever made the map: fm_remap_tap answers CLAMPED load positions for ANY two
// int32, so the pixels are loaded from inside the image first and the border is selected afterwards.
#pragma once
#include <cstddef>
#include <cstdint>

#define FM_REMAP_HD __host__ __device__ __forceinline__
#define FM_REMAP_BITS 5
#define FM_REMAP_MIN (-64)        // two whole pixels left of / above the image: all four taps outside

// the range a map entry must lie in for a sw x sh source (fm_frame_remap_set / fm_remap_bgr_host refuse any other)
FM_REMAP_HD bool fm_remap_entry_ok(int32_t X, int32_t Y, int sw, int sh) {
    return X >= FM_REMAP_MIN && X <= 32 * (sw + 1) && Y >= FM_REMAP_MIN && Y <= 32 * (sh + 1);
}

struct FmRemapTap {
    int cx, cy0, cy1;      // where to load: column of the left tap and the two rows, clamped into the image
    int fx, fy;            // weights of the right column / the lower row, 0..31
    int shift;             // bit position of the right tap's pixel in the 8-byte word loaded at column cx: 24, or 0 when
                           // the right tap IS column cx (ix = -1, the left tap is outside)
    bool x0, x1, y0, y1;   // tap column ix / ix + 1 and tap row iy / iy + 1 inside the image
};

FM_REMAP_HD FmRemapTap fm_remap_tap(int32_t X, int32_t Y, int sw, int sh) {
    const int ix = X >> FM_REMAP_BITS, iy = Y >> FM_REMAP_BITS;       // (|ix|, |iy| <= 2^26: ix + 1 cannot overflow)
    FmRemapTap t;
    t.fx = X & 31, t.fy = Y & 31;
    t.x0 = ix >= 0 && ix < sw, t.x1 = ix >= -1 && ix < sw - 1;
    t.y0 = iy >= 0 && iy < sh, t.y1 = iy >= -1 && iy < sh - 1;
    t.cx = ix < 0 ? 0 : ix > sw - 1 ? sw - 1 : ix;
    t.cy0 = iy < 0 ? 0 : iy > sh - 1 ? sh - 1 : iy;
    t.cy1 = iy + 1 < 0 ? 0 : iy + 1 > sh - 1 ? sh - 1 : iy + 1;
    t.shift = ix >= 0 ? 24 : 0;      // (x1 && ix >= 0 implies cx = ix < sw - 1: the word's second pixel is column ix + 1)
    return t;
}

// q0 / q1: the pixels at (cx, cy0) / (cx, cy1) in bits 0..23 and their right neighbours in bits 24..47 (little endian: 6
// consecutive bytes of a row; the neighbour's bits are not looked at unless tap column ix + 1 = cx + 1 is inside).
// border: b | g << 8 | r << 16.  Returns the pixel the same way.
FM_REMAP_HD uint32_t fm_remap_blend(uint64_t q0, uint64_t q1, const FmRemapTap& t, uint32_t border) {
    const int wx1 = t.fx, wx0 = 32 - t.fx, wy1 = t.fy, wy0 = 32 - t.fy;
    const bool in00 = t.x0 && t.y0, in01 = t.x1 && t.y0, in10 = t.x0 && t.y1, in11 = t.x1 && t.y1;
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int bc = (int)((border >> (8 * c)) & 255);
        const int p00 = in00 ? (int)((q0 >> (8 * c)) & 255) : bc, p01 = in01 ? (int)((q0 >> (t.shift + 8 * c)) & 255) : bc;
        const int p10 = in10 ? (int)((q1 >> (8 * c)) & 255) : bc, p11 = in11 ? (int)((q1 >> (t.shift + 8 * c)) & 255) : bc;
        const int v = (wy0 * (wx0 * p00 + wx1 * p01) + wy1 * (wx0 * p10 + wx1 * p11) + 512) >> 10;
        out |= (uint32_t)v << (8 * c);
    }
    return out;
}
