// The limited-range YCbCr -> BGR arithmetic shared by nv12.hip (interleaved chroma) and yuv.hip (planar chroma): the
// two matrices of include/fastmot_hip.h (FM_NV12_BT601 / FM_NV12_BT709) in 20-bit fixed point, and the saturating shift.
#pragma once
#include <cstdint>

struct Nv12Coef { int cy, cvr, cub, cug, cvg; };

constexpr int NV12_SHIFT = 20;
constexpr Nv12Coef NV12_COEF[2] = {
    {1220542, 1673527, 2116026, -409993, -852492},   // FM_NV12_BT601: OpenCV's COLOR_YUV2BGR_NV12 constants
    {1220945, 1879825, 2215014, -223607, -558796},   // FM_NV12_BT709: limited range, round(coef * 2^20)
};

// sat8(v >> 20), written as a clamp of v followed by the shift (the same value for every int v).  In the order
// shift - clamp - pack, the hipcc of ROCm 7.2 fuses two results into one v_ashr_pk_u8_i32 and ORs the other bytes of the output
// word onto it as if that instruction cleared bits 31:16 of its destination; on the MI355X it leaves them as they
// were, and bytes 2 and 3 of every output word came out ORed with stale register contents.
__device__ __forceinline__ uint32_t sat8(int v) { return (uint32_t)min(max(v, 0), (256 << NV12_SHIFT) - 1) >> NV12_SHIFT; }
