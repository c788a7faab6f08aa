// The YCbCr -> BGR arithmetic of every converter that has one (nv12.hip, yuv.hip, packed.hip, deep.hip): the matrices of
// include/fastmot_hip.h in 20-bit fixed point, a pixel in 32-bit and in 64-bit (deep) form, and the saturating narrowing
// (also resize.hip's and jpeg.hip's, which have arithmetic of their own before it).
#pragma once
#include <cstdint>

struct Nv12Coef { int cy, cvr, cub, cug, cvg; };

constexpr int NV12_SHIFT = 20;
constexpr Nv12Coef NV12_COEF[2] = {
    {1220542, 1673527, 2116026, -409993, -852492},   // FM_NV12_BT601: OpenCV's COLOR_YUV2BGR_NV12 constants
    {1220945, 1879825, 2215014, -223607, -558796},   // FM_NV12_BT709: limited range, round(coef * 2^20)
};
// FM_PACKED_BT601_FULL / FM_PACKED_BT709_FULL: round(coef * 2^20) of 1.402, 1.772, -0.344136, -0.714136 and of
// 1.5748, 1.8556, -0.187324, -0.468124 (CVR, CUB, CUG, CVG); the luma factor 1 << 20 goes with a luma offset of 0
constexpr Nv12Coef PACKED_FULL_COEF[2] = {
    {1 << NV12_SHIFT, 1470104, 1858077, -360853, -748826},
    {1 << NV12_SHIFT, 1651297, 1945738, -196423, -490864},
};
// FM_DEEP_BT601 / _BT709: the constants above.  FM_DEEP_BT2020: non-constant luminance, Kr = 0.2627, Kb = 0.0593,
// round(c * 2^20) of 255 / 219, 2 (1 - Kr) 255 / 224, 2 (1 - Kb) 255 / 224, -2 (1 - Kb) Kb / Kg 255 / 224, -2 (1 - Kr) Kr / Kg 255 / 224
constexpr Nv12Coef DEEP_COEF[3] = {NV12_COEF[0], NV12_COEF[1], {1220945, 1760217, 2245811, -196426, -682019}};

// sat8(v >> 20), written as a clamp of v followed by the shift (the same value for every int v).  In the order
// shift - clamp - pack, the hipcc of ROCm 7.2 fuses two results into one v_ashr_pk_u8_i32 and ORs the other bytes of the output
// word onto it as if that instruction cleared bits 31:16 of its destination; on the MI355X it leaves them as they
// were, and bytes 2 and 3 of every output word came out ORed with stale register contents.
__device__ __forceinline__ uint32_t sat8(int v) { return (uint32_t)min(max(v, 0), (256 << NV12_SHIFT) - 1) >> NV12_SHIFT; }
// the clamp of a value that needs no shift; one that does goes through sat8, or clamps before it shifts (the comment above)
__device__ __forceinline__ uint32_t clamp8(int v) { return (uint32_t)min(max(v, 0), 255); }

// The limited-range pixel:  y = max(Y - yoff, 0) * CY,  u = U - 128,  v = V - 128,  h = 1 << 19,
//     B = sat8((y + h + CUB u) >> 20)   G = sat8((y + h + CVG v + CUG u) >> 20)   R = sat8((y + h + CVR v) >> 20)
// (full range: yoff = 0 and CY = 1 << 20).  ycc_chroma: the three sums without y, once per chroma sample; ycc_px: a pixel
// from them.  Every intermediate fits 32 bits: 239 * 1220945 + 127 * 2215014 + h < 2^31.
__device__ __forceinline__ void ycc_chroma(const Nv12Coef& c, int u, int v, int& cb, int& cg, int& cr) {
    constexpr int half = 1 << (NV12_SHIFT - 1);
    cb = half + c.cub * u, cg = half + c.cvg * v + c.cug * u, cr = half + c.cvr * v;
}
__device__ __forceinline__ void ycc_px(const Nv12Coef& c, int Y, int yoff, int cb, int cg, int cr, uint32_t& b, uint32_t& g, uint32_t& r) {
    const int y = max(Y - yoff, 0) * c.cy;
    b = sat8(y + cb), g = sat8(y + cg), r = sat8(y + cr);
}

// The same for samples of 8 + s bits (u, v and yoff at that depth, h = 1 << (19 + s)): the sums reach 2^37.2 at s = 8, so
// they are 64-bit, one mad per term.  A sum is below 2^(29.2 + s) in magnitude, so (sum >> s) fits an int and
// sat8(sum >> (20 + s)) = sat8((int)(sum >> s) >> 20) exactly: the 64-bit part ends with one shift and sat8 does the rest.
__device__ __forceinline__ void ycc_chroma(const Nv12Coef& c, int u, int v, int s, long long& cb, long long& cg, long long& cr) {
    const long long half = 1ll << (NV12_SHIFT - 1 + s);
    cb = half + (long long)c.cub * u, cg = half + (long long)c.cvg * v + (long long)c.cug * u, cr = half + (long long)c.cvr * v;
}
__device__ __forceinline__ void ycc_px(const Nv12Coef& c, int Y, int yoff, int s, long long cb, long long cg, long long cr, uint32_t& b,
                                       uint32_t& g, uint32_t& r) {
    const long long y = (long long)max(Y - yoff, 0) * c.cy;
    b = sat8((int)((y + cb) >> s)), g = sat8((int)((y + cg) >> s)), r = sat8((int)((y + cr) >> s));
}
