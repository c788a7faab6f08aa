// fast-reid's Non_local block (AGW / SBS ReID models; Wang et al. 2018 in its dot-product form with ONE inner channel, as
// fastreid/layers/non_local.py builds it) over an NHWC fp16 channel view in one launch (FM_OP_NONLOCAL; models/onnx_graph.py):
//   theta_i = wt . x_i + bt,  phi_i = wp . x_i + bp,  g_i = wg . x_i + bg          three dot products over C per pixel
//   s       = (1 / HW) sum_i phi_i g_i                                             one scalar per sample
//   z[i, c] = x[i, c] + (a[c] * (theta_i * s) + b[c])                              a, b: the 1 -> C conv W with its BatchNorm folded
// to a NEW tensor.  With one inner channel matmul(matmul(theta, phi) / HW, g) is theta_i * s: the HW x HW matrix never exists.
// Everything between the fp16 load of x and the ONE fp16 store of z is fp32 and lives in registers or LDS.
//
// A workgroup of NL_T threads (half of that for C > 512) owns one sample: the first output element needs s, s needs the
// whole map, and workgroups of a launch can only meet through memory.  Lanes over the 8-channel groups of a pixel: LPP = min(64, the power of two >= C / 8)
// lanes share a pixel, lane l of them holds groups l, l + LPP, ...  (C = 512: a wave instruction reads one pixel's 1024
// consecutive bytes; C < 512: 64 / LPP pixels per instruction; C > 512: up to four loads per pixel; lanes whose group is past
// C / 8 -- C / 8 = 3 on four lanes -- load nothing and add zeros).  Wave w of W takes the pixel rows w, w + W, ... of 64 / LPP
// pixels each.
// Pass 1: a lane's partial dot products, folded over the LPP lanes of the pixel by xor shuffles (all of them hold the sum);
//         theta_i goes to LDS, phi_i * g_i is added to the slot's running sum in pixel order.  With a whole wave per pixel
//         (256 < C <= 512) the 3 x 8 sums of a batch of 8 pixels share one butterfly, which leaves each pixel's three sums
//         with 8 of the lanes: 30 shuffles per batch instead of 144.
// Fold:   the 64 / LPP slots of a wave by xor shuffles, the waves through LDS in wave order: every thread holds the same
//         bits of s.  The order of summation depends on (C, HW) alone -- not on the batch or the sample's index.
// Pass 2: the same lanes re-read the same bytes of x (L2) and store z.
// One workgroup per sample leaves most of the chip idle at the batches a tracker runs, and the passes are bound by what one
// CU keeps in flight.  So a sample may get K = gridDim.y workgroups that never meet: each runs pass 1 and the fold over the
// WHOLE map for itself -- the same loads in the same order, hence the same bits of s and theta -- and pass 2 over every K-th
// batch of pixel rows only.  What is stored does not depend on K.
// Parameters: a lane with one group (C <= 512) keeps its 24 weights and 16 affine values in registers; with more groups
// the five vectors are staged in LDS once.
#include "net.h"

namespace {

constexpr int NL_T = 1024;                   // 16 wavefronts; 8 where a lane has several groups (their weights pass through registers)
constexpr int NL_MAX_HW = 4096;              // theta of one map in LDS: 16 KB
constexpr int NL_MAX_C = 2048;               // the five parameter vectors in LDS: 40 KB
constexpr int NL_U1 = 8;                     // 16-byte loads a lane has in flight: pixel rows, where it has one group per pixel
constexpr int NL_UG = 4;                     // ... its groups of one pixel otherwise
constexpr int NL_SPLIT = 4;                  // at most this many workgroups share a sample's pass 2
static_assert(NL_MAX_C / 8 <= 64 * NL_UG, "a lane's groups of one pixel are one batch of loads");

__device__ __forceinline__ void load8(const float* p, float* f) {
    const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
    f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w; f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
}

// v[0 .. 2 H) -> v[0 .. H): a lane keeps the lower half (upper: the upper half) and adds its partner's share of it
template <int H>
__device__ __forceinline__ void halve(float* v, bool upper, int off) {
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const float keep = upper ? v[i + H] : v[i], send = upper ? v[i] : v[i + H];
        v[i] = keep + __shfl_xor(send, off);
    }
}

// ONE: every lane has at most one channel group (C / 8 <= LPP)
template <int LPP, bool ONE>
__global__ __launch_bounds__(ONE ? NL_T : NL_T / 2) void nonlocal_kernel(const f16* __restrict__ in, int in_cs, int in_coff, f16* __restrict__ out,
                                                        int out_cs, int out_coff, int HW, int C, const float* __restrict__ w3,
                                                        const float* __restrict__ bias3, const float* __restrict__ wa,
                                                        const float* __restrict__ wb) {
    constexpr int T = ONE ? NL_T : NL_T / 2, U = ONE ? NL_U1 : NL_UG;
    constexpr bool WIDE = ONE && LPP == 64;                  // 256 < C <= 512: a whole wave per pixel, 8 pixels per batch of loads
    static_assert(!WIDE || U == 8, "the butterfly below hands out 8 pixels over 3 bits of the lane");
    __shared__ float theta[NL_MAX_HW];
    __shared__ float red[T / 64];
    __shared__ float par[ONE ? 8 : 5 * NL_MAX_C];            // theta, phi, g weights, a, b: C floats each
    constexpr int PPW = 64 / LPP;                            // pixels of one wave instruction
    constexpr int STEP = T / 64 * PPW;                       // pixel step of a wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = lane % LPP, slot = lane / LPP;
    const int ng = C / 8;
    const f16* src = in + (size_t)blockIdx.x * HW * in_cs + in_coff;
    f16* dst = out + (size_t)blockIdx.x * HW * out_cs + out_coff;
    const float bt = bias3[0], bp = bias3[1], bg = bias3[2];

    float wt[8] = {0, 0, 0, 0, 0, 0, 0, 0}, wp[8] = {0, 0, 0, 0, 0, 0, 0, 0}, wg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (ONE) {
        if (l < ng) {                                        // (a lane without a group multiplies zeros by zeros)
            load8(w3 + l * 8, wt);
            load8(w3 + C + l * 8, wp);
            load8(w3 + 2 * C + l * 8, wg);
        }
    } else {
        for (int i = tid; i < 3 * C; i += T) par[i] = w3[i];
        for (int i = tid; i < C; i += T) {
            par[3 * C + i] = wa[i];
            par[4 * C + i] = wb[i];
        }
        __syncthreads();
    }

    // ---- 1. the three dot products of every pixel; theta to LDS, phi * g into the slot's sum.  U loads are issued before
    //         the first is used: U pixel rows (ONE), or the up to U groups of one pixel
    float part = 0.f;
    const uint4 zero{0, 0, 0, 0};
    auto pixel_done = [&](float t, float p, float g, int px) {
#pragma unroll
        for (int off = LPP / 2; off >= 1; off >>= 1) {
            t += __shfl_xor(t, off);
            p += __shfl_xor(p, off);
            g += __shfl_xor(g, off);
        }
        if (px < HW) {
            if (l == 0) theta[px] = t + bt;
            part += (p + bp) * (g + bg);
        }
    };
    for (int base = wave * PPW; base < HW; base += ONE ? STEP * U : STEP) {   // (wave-uniform: every lane reaches the shuffles)
        uint4 raw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int px = base + slot + (ONE ? u * STEP : 0), cg = l + (ONE ? 0 : u * LPP);
            raw[u] = px < HW && cg < ng ? *reinterpret_cast<const uint4*>(src + (size_t)px * in_cs + cg * 8) : zero;
        }
        float t = 0.f, p = 0.f, g = 0.f;
        float acc[WIDE ? 3 * U : 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float v[8];
            unpack8(raw[u], v);
            if constexpr (!ONE) {                            // (past C / 8: zeros times whatever the LDS row holds)
                const int cg = min(l + u * LPP, ng - 1);
                load8(par + cg * 8, wt);
                load8(par + C + cg * 8, wp);
                load8(par + 2 * C + cg * 8, wg);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                t = fmaf(wt[e], v[e], t);
                p = fmaf(wp[e], v[e], p);
                g = fmaf(wg[e], v[e], g);
            }
            if constexpr (WIDE) {
                acc[3 * u] = t;
                acc[3 * u + 1] = p;
                acc[3 * u + 2] = g;
                t = p = g = 0.f;
            } else if constexpr (ONE) {
                pixel_done(t, p, g, base + slot + u * STEP);
                t = p = g = 0.f;
            }
        }
        if constexpr (WIDE) {
            // the 24 sums of the batch's 8 pixels over the 64 lanes as ONE butterfly: at each of the first three steps a lane
            // keeps one half of its values and hands the other to its partner (12 + 6 + 3 shuffles), then the three values
            // of ONE pixel -- pixel u = bits 5, 4, 3 of the lane -- take the last three steps (9): 30 shuffles where 8
            // pixel_done calls take 144.  The launch spent more than half its time in those (profiles/reid_nonlocal.txt)
            halve<12>(acc, lane & 32, 32);
            halve<6>(acc, lane & 16, 16);
            halve<3>(acc, lane & 8, 8);
#pragma unroll
            for (int off = 4; off >= 1; off >>= 1)
#pragma unroll
                for (int i = 0; i < 3; ++i) acc[i] += __shfl_xor(acc[i], off);
            const int px = base + (lane >> 3) * STEP;
            if (px < HW) {
                if ((lane & 7) == 0) theta[px] = acc[0] + bt;
                part += (acc[1] + bp) * (acc[2] + bg);
            }
        }
        if constexpr (!ONE) pixel_done(t, p, g, base + slot);
    }
    // ---- the sample's scalar: slots of a wave (WIDE: the eight pixel positions of a batch), then the waves in order
#pragma unroll
    for (int off = 32; off >= (WIDE ? 8 : LPP); off >>= 1) part += __shfl_xor(part, off);
    if (lane == 0) red[wave] = part;
    __syncthreads();                                         // (theta of every pixel is in LDS as well)
    float s = 0.f;
#pragma unroll
    for (int wv = 0; wv < T / 64; ++wv) s += red[wv];
    s = s / (float)HW;

    // ---- 2. z = x + (a * (theta * s) + b), one rounding to fp16
    float a[8], b[8];
    if constexpr (ONE) {
        if (l >= ng) return;
        load8(wa + l * 8, a);
        load8(wb + l * 8, b);
    }
    constexpr int BATCH = ONE ? STEP * U : STEP;             // pixels of one batch of loads of the workgroup
    for (int base = blockIdx.y * BATCH + wave * PPW + slot; base < HW; base += gridDim.y * BATCH) {
        uint4 raw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int px = base + (ONE ? u * STEP : 0), cg = l + (ONE ? 0 : u * LPP);
            raw[u] = px < HW && cg < ng ? *reinterpret_cast<const uint4*>(src + (size_t)px * in_cs + cg * 8) : zero;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int px = base + (ONE ? u * STEP : 0), cg = l + (ONE ? 0 : u * LPP);
            if (px < HW && cg < ng) {
                const float y = theta[px] * s;
                float v[8];
                unpack8(raw[u], v);
                if constexpr (!ONE) {
                    load8(par + 3 * C + cg * 8, a);
                    load8(par + 4 * C + cg * 8, b);
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += fmaf(a[e], y, b[e]);
                *reinterpret_cast<uint4*>(dst + (size_t)px * out_cs + cg * 8) = pack8(v);
            }
        }
    }
}

}  // namespace

// the one rule behind Graph.nonlocal_supported (models/graph.py) and the launch check below
bool nonlocal_supported(int C, int hw) { return C >= 8 && C <= NL_MAX_C && C % 8 == 0 && hw >= 1 && hw <= NL_MAX_HW; }
extern "C" int fm_nonlocal_supported(int c, int hw) { return nonlocal_supported(c, hw) ? 1 : 0; }

// w3 = f32 [3][C] (theta, phi, g), bias3 = their three biases, wa / wb = f32 [C]
int launch_nonlocal(const f16* in, int in_cs, int in_coff, f16* out, int out_cs, int out_coff, int N, int HW, int C, const float* w3,
                    const float* bias3, const float* wa, const float* wb, hipStream_t s) {
    FM_CHECK_ARG(in && out && in != out && w3 && bias3 && wa && wb && N >= 1 && N <= 65535 && nonlocal_supported(C, HW));
    FM_CHECK_ARG(in_cs % 8 == 0 && out_cs % 8 == 0 && in_coff >= 0 && out_coff >= 0 && in_coff % 8 == 0 && out_coff % 8 == 0 &&
                 in_coff + C <= in_cs && out_coff + C <= out_cs);
    const int ng = C / 8;
    // workgroups per sample: while the launch stays under the chip's 256 CUs and every one of them has a batch of pass 2
    const int lpp = ng > 32 ? 64 : ng > 16 ? 32 : ng > 8 ? 16 : ng > 4 ? 8 : ng > 2 ? 4 : ng > 1 ? 2 : 1;
    const int batch_px = ng > 64 ? NL_T / 2 / 64 : NL_T / 64 * (64 / lpp) * NL_U1;
    int split = 1;
    while (split < NL_SPLIT && (long)N * split * 2 <= 256 && split * 2 * batch_px <= HW) split *= 2;
#define FM_NL_LAUNCH(LPP, ONE)                                                                                                   \
    hipLaunchKernelGGL((nonlocal_kernel<LPP, ONE>), dim3(N, split), dim3(ONE ? NL_T : NL_T / 2), 0, s, in, in_cs, in_coff, out, out_cs, out_coff, HW, C, w3, \
                       bias3, wa, wb)
    if (ng > 64) FM_NL_LAUNCH(64, false);
    else if (ng > 32) FM_NL_LAUNCH(64, true);
    else if (ng > 16) FM_NL_LAUNCH(32, true);
    else if (ng > 8) FM_NL_LAUNCH(16, true);
    else if (ng > 4) FM_NL_LAUNCH(8, true);
    else if (ng > 2) FM_NL_LAUNCH(4, true);
    else if (ng > 1) FM_NL_LAUNCH(2, true);
    else FM_NL_LAUNCH(1, true);
#undef FM_NL_LAUNCH
    FM_HIP(hipGetLastError());
    return 0;
}
