// Instance normalisation of an NHWC fp16 channel view in one launch (FM_OP_INSTNORM; models/onnx_graph.py: the IN half of an
// IBN-a layer, the IN behind a residual sum or the stem of an IBN-b model):
//   channels [0, cn) of the view: per sample and channel over the HW pixels, biased variance,
//       y = act((x - mean) * (1 / sqrt(var + eps)) * gamma[c] + beta[c]),  rounded to fp16 once, on the store
//   channels [cn, C): y = act(x)          (the BatchNorm half of IBN-a is folded into the conv in front; its ReLU waits here)
// to a NEW tensor.  Optionally (template flag RES; the unfused tail of an OSNet-AIN block, relu(IN(conv3(x2)) + identity)) a
// residual view of C channels is added to every channel behind the affine and in front of the activation; a layer without
// it runs the instantiation without a single instruction for it.  All statistics in fp32; the variance is the sum of CENTRED squares from a second pass over the same
// values (E[x^2] - mean^2 in fp32 loses every digit of a channel with mean 100 and std 0.1).
//
// Lanes over (pixel, channel group): a workgroup of IN_T threads owns one sample and G consecutive 8-channel groups,
// G in {1, 2, 4, 8}.  Thread t holds group t % G of pixels t / G, t / G + IN_T / G, ...: the G lanes of one pixel read
// G x 16 consecutive bytes, so one wave instruction touches 64 / G pixels with G x 16 bytes each, channel-stride apart.
// A thread sums its pixels in order, a wavefront folds the lanes of equal group by xor shuffles (32 .. G), the 8 waves
// meet in LDS and every thread adds the 8 partials in wave order: all threads hold the same mean / rstd bits.
// Register path (HW * G <= IN_T * IN_R): the pixels are loaded ONCE as 16-byte vectors and stay in registers across the two
// statistics passes and the apply.  Larger maps (128 x 64 behind an IN stem) take the same code with every pass re-reading
// the view (L2 / Infinity Cache): same arithmetic, same order of summation per lane.
#include "net.h"

namespace {

constexpr int IN_T = 512;                    // 8 wavefronts
constexpr int IN_R = 8;                      // 16-byte vectors a thread keeps (register path)

template <int G>
__device__ __forceinline__ void fold8(float* a, float (*red)[8][8], int wave, int lane, int cg) {
#pragma unroll
    for (int off = 32; off >= G; off >>= 1)
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += __shfl_xor(a[e], off);
    if (lane < G)
#pragma unroll
        for (int e = 0; e < 8; ++e) red[wave][cg][e] = a[e];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float t = 0.f;
#pragma unroll
        for (int wv = 0; wv < IN_T / 64; ++wv) t += red[wv][cg][e];
        a[e] = t;
    }
}

template <int G, bool REG, bool RES>
__global__ __launch_bounds__(IN_T) void instnorm_kernel(const f16* __restrict__ in, int in_cs, int in_coff, f16* __restrict__ out,
                                                        int out_cs, int out_coff, int HW, int C, int cn,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float eps, int act, const f16* __restrict__ res, int res_cs, int res_coff) {
    __shared__ float red[2][IN_T / 64][8][8];
    constexpr int PS = IN_T / G;                             // pixel step of a thread
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cg = tid % G, slot = tid / G;
    const int c0 = (blockIdx.x * G + cg) * 8;                // first channel of this thread's group, inside the view
    const bool live = c0 < C, norm = c0 < cn;                // (a ragged last block: lanes without a group load and store nothing)
    const f16* src = in + (size_t)blockIdx.y * HW * in_cs + in_coff + c0;
    f16* dst = out + (size_t)blockIdx.y * HW * out_cs + out_coff + c0;

    uint4 x[REG ? IN_R : 1];
    if constexpr (REG) {
#pragma unroll
        for (int r = 0; r < IN_R; ++r) {
            const int px = slot + r * PS;
            x[r] = live && px < HW ? *reinterpret_cast<const uint4*>(src + (size_t)px * in_cs) : uint4{0, 0, 0, 0};
        }
    }
    float mean[8], rstd[8];
    // (uniform per workgroup unless cn falls inside its G groups: then the pass-through lanes fold zeros along)
    if (blockIdx.x * G * 8 < cn) {
        // ---- 1. mean: fp32 sum, a divide
        float a[8] = {0, 0, 0, 0, 0, 0, 0, 0}, v[8];
        if constexpr (REG) {
#pragma unroll
            for (int r = 0; r < IN_R; ++r) {                 // (pixels past HW hold zeros)
                unpack8(x[r], v);
#pragma unroll
                for (int e = 0; e < 8; ++e) a[e] += v[e];
            }
        } else if (norm) {
            for (int px = slot; px < HW; px += PS) {
                unpack8(*reinterpret_cast<const uint4*>(src + (size_t)px * in_cs), v);
#pragma unroll
                for (int e = 0; e < 8; ++e) a[e] += v[e];
            }
        }
        fold8<G>(a, red[0], wave, lane, cg);
#pragma unroll
        for (int e = 0; e < 8; ++e) mean[e] = a[e] / (float)HW;
        // ---- 2. biased variance: the sum of centred squares over the same values
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = 0.f;
        if constexpr (REG) {
#pragma unroll
            for (int r = 0; r < IN_R; ++r)
                if (slot + r * PS < HW) {
                    unpack8(x[r], v);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float d = v[e] - mean[e];
                        a[e] += d * d;
                    }
                }
        } else if (norm) {
            for (int px = slot; px < HW; px += PS) {
                unpack8(*reinterpret_cast<const uint4*>(src + (size_t)px * in_cs), v);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = v[e] - mean[e];
                    a[e] += d * d;
                }
            }
        }
        fold8<G>(a, red[1], wave, lane, cg);
#pragma unroll
        for (int e = 0; e < 8; ++e) rstd[e] = 1.0f / sqrtf(a[e] / (float)HW + eps);
    }
    if (!live) return;
    // ---- 3. apply, activation, one rounding to fp16
    float g[8], b[8];
    if (norm) {
        const float4 g0 = *reinterpret_cast<const float4*>(gamma + c0), g1 = *reinterpret_cast<const float4*>(gamma + c0 + 4);
        const float4 b0 = *reinterpret_cast<const float4*>(beta + c0), b1 = *reinterpret_cast<const float4*>(beta + c0 + 4);
        g[0] = g0.x; g[1] = g0.y; g[2] = g0.z; g[3] = g0.w; g[4] = g1.x; g[5] = g1.y; g[6] = g1.z; g[7] = g1.w;
        b[0] = b0.x; b[1] = b0.y; b[2] = b0.z; b[3] = b0.w; b[4] = b1.x; b[5] = b1.y; b[6] = b1.z; b[7] = b1.w;
    }
    auto apply = [&](const uint4& raw, int px) {
        float v[8];
        unpack8(raw, v);
        if (norm)
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (v[e] - mean[e]) * rstd[e] * g[e] + b[e];
        if constexpr (RES) {                                 // the residual view: behind the affine, in front of the activation
            float r[8];
            unpack8(*reinterpret_cast<const uint4*>(res + ((size_t)blockIdx.y * HW + px) * res_cs + res_coff + c0), r);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += r[e];
        }
        if (act == ACT_RELU)
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = act_relu(v[e]);
        *reinterpret_cast<uint4*>(dst + (size_t)px * out_cs) = pack8(v);
    };
    if constexpr (REG) {
#pragma unroll
        for (int r = 0; r < IN_R; ++r)
            if (slot + r * PS < HW) apply(x[r], slot + r * PS);
    } else {
        for (int px = slot; px < HW; px += PS) apply(*reinterpret_cast<const uint4*>(src + (size_t)px * in_cs), px);
    }
}

template <int G>
void launch_g(bool reg, dim3 grid, hipStream_t s, const f16* in, int in_cs, int in_coff, f16* out, int out_cs, int out_coff, int HW,
              int C, int cn, const float* gamma, const float* beta, float eps, int act, const f16* res, int res_cs, int res_coff) {
#define FM_IN_LAUNCH(REG, RES)                                                                                                  \
    hipLaunchKernelGGL((instnorm_kernel<G, REG, RES>), grid, dim3(IN_T), 0, s, in, in_cs, in_coff, out, out_cs, out_coff, HW, C, cn, \
                       gamma, beta, eps, act, res, res_cs, res_coff)
    if (res) {
        if (reg) FM_IN_LAUNCH(true, true); else FM_IN_LAUNCH(false, true);
    } else {
        if (reg) FM_IN_LAUNCH(true, false); else FM_IN_LAUNCH(false, false);
    }
#undef FM_IN_LAUNCH
}

}  // namespace

// pixels one workgroup keeps in registers with G channel groups per pixel
int instnorm_reg_pixels(int G) { return IN_T * IN_R / G; }

// The channel groups a workgroup owns: as many as sit side by side in memory (the bytes one wave instruction finds
// together), halved while the map does not fit the registers (a map that fits with no G keeps the widest: it re-reads),
// and halved down to 2 while the grid would leave most of the chip's 256 CUs without a workgroup.
int instnorm_groups(int N, int HW, int C) {
    const int ng = C / 8;
    int wide = 8;
    while (wide > 1 && wide / 2 >= ng) wide >>= 1;
    int G = wide;
    while (G > 1 && HW > instnorm_reg_pixels(G)) G >>= 1;
    if (HW > instnorm_reg_pixels(G)) G = wide;
    while (G > 2 && (long)N * ((ng + G - 1) / G) < 128) G >>= 1;
    return G;
}

// res: nullptr, or a view of C channels (res_cs, res_coff) added to every channel behind the affine, in front of the activation
int launch_instnorm(const f16* in, int in_cs, int in_coff, f16* out, int out_cs, int out_coff, int N, int HW, int C, int cn,
                    const float* gamma, const float* beta, float eps, int act, hipStream_t s, const f16* res, int res_cs,
                    int res_coff) {
    FM_CHECK_ARG(in && out && gamma && beta && N >= 1 && N <= 65535 && HW >= 1 && C >= 8 && C % 8 == 0 && cn >= 8 && cn % 8 == 0 && cn <= C);
    FM_CHECK_ARG(in_cs % 8 == 0 && out_cs % 8 == 0 && in_coff >= 0 && out_coff >= 0 && in_coff % 8 == 0 && out_coff % 8 == 0 &&
                 in_coff + C <= in_cs && out_coff + C <= out_cs);
    FM_CHECK_ARG((act == ACT_LINEAR || act == ACT_RELU) && eps >= 0.f && eps < 1.f);
    FM_CHECK_ARG(!res || (res_cs % 8 == 0 && res_coff >= 0 && res_coff % 8 == 0 && res_coff + C <= res_cs));
    const int G = instnorm_groups(N, HW, C);
    const bool reg = HW <= instnorm_reg_pixels(G);
    const dim3 grid((C / 8 + G - 1) / G, N);
    switch (G) {
        case 8: launch_g<8>(reg, grid, s, in, in_cs, in_coff, out, out_cs, out_coff, HW, C, cn, gamma, beta, eps, act, res, res_cs, res_coff); break;
        case 4: launch_g<4>(reg, grid, s, in, in_cs, in_coff, out, out_cs, out_coff, HW, C, cn, gamma, beta, eps, act, res, res_cs, res_coff); break;
        case 2: launch_g<2>(reg, grid, s, in, in_cs, in_coff, out, out_cs, out_coff, HW, C, cn, gamma, beta, eps, act, res, res_cs, res_coff); break;
        default: launch_g<1>(reg, grid, s, in, in_cs, in_coff, out, out_cs, out_coff, HW, C, cn, gamma, beta, eps, act, res, res_cs, res_coff); break;
    }
    FM_HIP(hipGetLastError());
    return 0;
}
