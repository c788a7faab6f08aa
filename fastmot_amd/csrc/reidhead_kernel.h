// The kernel of FM_OP_POOLHEAD (reidhead.hip has the description), a template over the pooling mode so that its two users
// are separate translation units: reidhead.hip instantiates the average pool with the flags of the whole library, and
// reidhead_gem.hip the two GeM modes without the SLP vectoriser (build.py FILE_FLAGS) -- powf / cbrtf bring double-float
// arithmetic that the vectoriser pairs into packed fp32 with a cross-half op_sel, the form tests/test_isa_lint.py refuses.
#pragma once
#include "net.h"

namespace {

constexpr int PH_T = 512;                    // 8 wavefronts
constexpr int PH_R = 8;                      // output rows a wavefront works on at once
constexpr int PH_MAX = 4096;                 // largest C and D
constexpr size_t PH_LDS_MAX = 64 * 1024;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

enum { GEM_NONE = 0, GEM_CUBE = 1, GEM_POW = 2 };

template <int GEM>
__global__ __launch_bounds__(PH_T) void poolhead_kernel(const f16* __restrict__ in, int in_cs, int in_coff, int HW, int C, int D,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        const f16* __restrict__ w, const float* __restrict__ b, int relu,
                                                        float* __restrict__ out, float* __restrict__ mirror, float gem_p, float gem_eps) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c8n = C >> 3;
    const int groups = c8n < PH_T ? PH_T / c8n : 1;          // pixel groups that share a column of 8 channels
    float* part = sm;                                        // [groups][C]
    float* pooled = part + groups * C;
    float* feat = w ? pooled + C : pooled;                   // (no FC: the pooled vector is the feature, D == C)
    float* red = feat + D;

    // ---- 1. global average pool: 16-byte loads, fp32 sums; pixel group g takes pixels g, g + groups, ...
    const f16* base = in + (size_t)n * HW * in_cs + in_coff;
    for (int it = tid; it < groups * c8n; it += PH_T) {
        const int pg = it / c8n, cg = it - pg * c8n;
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int px = pg; px < HW; px += groups) {
            float v[8];
            unpack8(*reinterpret_cast<const uint4*>(base + (size_t)px * in_cs + cg * 8), v);
            if constexpr (GEM != GEM_NONE) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float t = fmaxf(v[e], gem_eps);
                    v[e] = GEM == GEM_CUBE ? t * t * t : powf(t, gem_p);
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += v[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) part[pg * C + cg * 8 + e] = acc[e];
    }
    __syncthreads();
    // ---- 2. mean, then the BN neck as one multiply and one add per channel
    for (int c = tid; c < C; c += PH_T) {
        float s = 0.f;
        for (int g = 0; g < groups; ++g) s += part[g * C + c];
        float m = s / (float)HW;
        if constexpr (GEM == GEM_CUBE) m = cbrtf(m);
        if constexpr (GEM == GEM_POW) m = powf(m, 1.0f / gem_p);
        if (scale) m = m * scale[c] + shift[c];
        pooled[c] = m;
    }
    __syncthreads();
    // ---- 3. FC: one wavefront per output row, PH_R rows at a time -- their weight loads are independent, so PH_R x 16 B per
    // lane are in flight per step (one row at a time is a chain of load -> wait -> 8 FMAs: latency bound)
    if (w) {
        for (int d0 = wave * PH_R; d0 < D; d0 += (PH_T / 64) * PH_R) {
            float s[PH_R];
            const f16* wr[PH_R];
#pragma unroll
            for (int r = 0; r < PH_R; ++r) {
                s[r] = 0.f;
                wr[r] = w + (size_t)min(d0 + r, D - 1) * C;        // (rows past D: the last row again, not stored)
            }
            for (int c = lane * 8; c < C; c += 64 * 8) {
                uint4 wv[PH_R];
#pragma unroll
                for (int r = 0; r < PH_R; ++r) wv[r] = *reinterpret_cast<const uint4*>(wr[r] + c);
                const float4 g0 = *reinterpret_cast<const float4*>(pooled + c);
                const float4 g1 = *reinterpret_cast<const float4*>(pooled + c + 4);
#pragma unroll
                for (int r = 0; r < PH_R; ++r) {
                    // (v_fma_mix_f32 extends the half inside the FMA: the value of convert + fmaf; as inline assembly it also
                    // keeps the SLP vectoriser from pairing two rows into packed fp32 with a cross-half op_sel, the form
                    // tests/test_isa_lint.py refuses)
                    float a = s[r];
                    a = fma_mix_h<0>(wv[r].x, g0.x, a); a = fma_mix_h<1>(wv[r].x, g0.y, a);
                    a = fma_mix_h<0>(wv[r].y, g0.z, a); a = fma_mix_h<1>(wv[r].y, g0.w, a);
                    a = fma_mix_h<0>(wv[r].z, g1.x, a); a = fma_mix_h<1>(wv[r].z, g1.y, a);
                    a = fma_mix_h<0>(wv[r].w, g1.z, a); a = fma_mix_h<1>(wv[r].w, g1.w, a);
                    s[r] = a;
                }
            }
#pragma unroll
            for (int r = 0; r < PH_R; ++r) {
                const float t = wave_sum(s[r]) + b[min(d0 + r, D - 1)];
                if (lane == 0 && d0 + r < D) feat[d0 + r] = relu ? act_relu(t) : t;
            }
        }
        __syncthreads();
    }
    // ---- 4. L2 normalise, 5. the row to the embedding matrix and its host mirror
    float nrm = 0.f;
    for (int d = tid; d < D; d += PH_T) nrm = fmaf(feat[d], feat[d], nrm);
    nrm = wave_sum(nrm);
    if (lane == 0) red[wave] = nrm;
    __syncthreads();
    float total = 0.f;
#pragma unroll
    for (int i = 0; i < PH_T / 64; ++i) total += red[i];
    const float inv = 1.f / sqrtf(total);
    for (int d = tid; d < D; d += PH_T) {
        const float v = feat[d] * inv;
        out[(size_t)n * D + d] = v;
        if (mirror) mirror[(size_t)n * D + d] = v;
    }
}

}  // namespace
