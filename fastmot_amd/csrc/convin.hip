// The tail of an OSNet-IBN / OSNet-AIN block in one launch (FM_OP_CONVIN): pointwise conv, instance normalisation, residual, ReLU
//   v = W x + b (+ res, FM_RES_BEFORE_NORM)                                   fp32 accumulators, never stored
//   y = act((v - mean_nc) * (1 / sqrt(var_nc + eps)) * gamma + beta (+ res, FM_RES_BEFORE_ACT))      one fp16 store
// with mean / var per sample and channel over the HW pixels of v (biased variance).  Unfused this is a conv that stores v as
// fp16 and FM_OP_INSTNORM that reads it back (Graph.convin with use_convin off).
//
// The statistics of a (sample, channel) need the whole map before the first output, so a workgroup of NW wavefronts owns one
// sample and ONE tile of 32 output channels and keeps the whole map's accumulators in registers: wave w holds the T pixel
// tiles w, w + NW, .. of 32 pixels each as T accumulators of mfma_f32_32x32x16_f16 (lane = pixel, 16 registers = channels
// (r & 3) + 8 (r >> 2) + 4 (lane >> 5)); T * NW * 32 >= HW, at most 4 x 16 x 32 = 2048 pixels (64 accumulator registers of the
// 128 a wave has at 4 waves per SIMD).  Weights are the A operand in MFMA fragment order (Graph._pack_frag) straight from L2 as
// in sepconv.hip; pixels are the B operand, one 16-byte NHWC load per lane and K step without LDS staging: every pixel tile
// has exactly one reader.  K % 16 == 8: the upper half of the last K step is zero on both sides.
// Statistics in fp32, in one fixed order: a lane adds its T tiles, 32 lanes fold by xor shuffles (16 .. 1), the waves meet in
// LDS, thread c adds channel c's NW partials in wave order and every thread reads the totals back -- the same mean / rstd
// bits in all of them.  Two passes over the registers, the mean first and then CENTRED squares (instnorm.hip says why).
// Lanes of pixels beyond HW in a ragged last tile add nothing to either sum; the divisor is HW.  (T, NW) depend on HW alone,
// so a sample's bits do not depend on the batch.
#include "net.h"

namespace {

struct ConvInParams {
    const f16* in;  int in_cs, in_coff;
    f16* out;       int out_cs, out_coff;
    const f16* res; int res_cs, res_coff, res_mode;
    const f16* w;           // [ceil32(cout) / 32][ceil16(K) / 16][64][8] fp16
    const float* bias;      // f32 [ceil32(cout)], likewise gamma / beta
    const float* gamma;
    const float* beta;
    int HW, K, cout, act;
    float eps;
};

constexpr int CI_RES_BEFORE_NORM = 3;      // FM_RES_BEFORE_NORM (fastmot_hip.h)

// the 16 channel sums of a lane -> the workgroup's totals, the same bits in every thread
template <int NW>
__device__ __forceinline__ void fold_channels(float* s, float (*red)[32], float* tot, int wave, int frow, int fh) {
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] += __shfl_xor(s[r], off);
    if (frow == 0)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wave][(r & 3) + 8 * (r >> 2) + 4 * fh] = s[r];
    __syncthreads();
    if (threadIdx.x < 32) {                                  // thread c adds channel c's partials in wave order
        float t = 0.f;
#pragma unroll
        for (int wv = 0; wv < NW; ++wv) t += red[wv][threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = tot[(r & 3) + 8 * (r >> 2) + 4 * fh];
}

template <int T, int NW>
__global__ __launch_bounds__(NW * 64) void convin_kernel(const ConvInParams p) {
    __shared__ float red[2][NW][32], tot[2][32];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, fh = lane >> 5;
    const int ct = blockIdx.x;
    const size_t n = blockIdx.y;
    const int k16 = (p.K + 15) >> 4;
    const int n_tiles = (p.HW + 31) >> 5;

    f32x16 acc[T];
    int pix[T];                                              // this lane's pixel of tile j, clamped into the map
    bool valid[T];
#pragma unroll
    for (int j = 0; j < T; ++j) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        const int px = (j * NW + wave) * 32 + frow;
        valid[j] = px < p.HW;
        pix[j] = min(px, p.HW - 1);
    }
    // ---- 1. the conv: K steps in ascending order into the same accumulators
    const f16* src = p.in + n * p.HW * p.in_cs + p.in_coff + fh * 8;
    const f16* wrow = p.w + ((size_t)ct * k16 * 64 + lane) * 8;
    // (tile by tile, and per tile the accesses to one pixel's row back to back: a 16-byte K step, or an 8-byte channel group, is
    // a fraction of a cache line, and a line that waits for its other fractions behind the rest of the map is fetched again)
#pragma unroll
    for (int j = 0; j < T; ++j) {
        if ((j * NW + wave) >= n_tiles) continue;            // (wave-uniform: a tile beyond the map stays zero)
        const f16* row = src + (size_t)pix[j] * p.in_cs;
#pragma unroll 4
        for (int ks = 0; ks < k16; ++ks) {
            const f16x8 fa = *reinterpret_cast<const f16x8*>(wrow + (size_t)ks * 512);
            f16x8 fb = {0, 0, 0, 0, 0, 0, 0, 0};
            if (ks * 16 + fh * 8 < p.K) fb = *reinterpret_cast<const f16x8*>(row + ks * 16);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa, fb, acc[j], 0, 0, 0);
        }
    }
    // ---- 2. bias (and the residual that is part of the normalised value)
    const f16* rsrc = p.res_mode != RES_NONE ? p.res + n * p.HW * p.res_cs + p.res_coff + ct * 32 + fh * 4 : nullptr;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        f16x4 rv[4] = {};
        if (p.res_mode == CI_RES_BEFORE_NORM)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (ct * 32 + g * 8 + fh * 4 < p.cout) rv[g] = *reinterpret_cast<const f16x4*>(rsrc + (size_t)pix[j] * p.res_cs + g * 8);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 bv = *reinterpret_cast<const float4*>(p.bias + ct * 32 + g * 8 + fh * 4);
            acc[j][4 * g + 0] += bv.x; acc[j][4 * g + 1] += bv.y; acc[j][4 * g + 2] += bv.z; acc[j][4 * g + 3] += bv.w;
            if (p.res_mode == CI_RES_BEFORE_NORM)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j][4 * g + e] += (float)rv[g][e];
        }
    }
    // ---- 3. mean: fp32 sum, a divide
    float mean[16], s[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int j = 0; j < T; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] += valid[j] ? acc[j][r] : 0.f;
    fold_channels<NW>(s, red[0], tot[0], wave, frow, fh);
#pragma unroll
    for (int r = 0; r < 16; ++r) mean[r] = s[r] / (float)p.HW;
    // ---- 4. biased variance: the sum of centred squares over the same values
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int j = 0; j < T; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float d = acc[j][r] - mean[r];
            s[r] += valid[j] ? d * d : 0.f;
        }
    fold_channels<NW>(s, red[1], tot[1], wave, frow, fh);
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 1.0f / sqrtf(s[r] / (float)p.HW + p.eps);      // rstd
    // ---- 5. apply, residual, activation, one rounding to fp16
    f16* dst = p.out + n * p.HW * p.out_cs + p.out_coff + ct * 32 + fh * 4;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        if (!valid[j]) continue;
        f16x4 rv[4] = {};
        if (p.res_mode == RES_BEFORE_ACT)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (ct * 32 + g * 8 + fh * 4 < p.cout) rv[g] = *reinterpret_cast<const f16x4*>(rsrc + (size_t)pix[j] * p.res_cs + g * 8);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int co = ct * 32 + g * 8 + fh * 4;
            if (co >= p.cout) continue;                      // (cout % 8 == 0: a 4-channel group is all in or all out)
            const float4 gv = *reinterpret_cast<const float4*>(p.gamma + co), bv = *reinterpret_cast<const float4*>(p.beta + co);
            const float ga[4] = {gv.x, gv.y, gv.z, gv.w}, be[4] = {bv.x, bv.y, bv.z, bv.w};
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (acc[j][4 * g + e] - mean[4 * g + e]) * s[4 * g + e] * ga[e] + be[e];
            if (p.res_mode == RES_BEFORE_ACT)
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += (float)rv[g][e];
            if (p.act == ACT_RELU)
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = act_relu(v[e]);
            f16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (f16)v[e];
            *reinterpret_cast<f16x4*>(dst + (size_t)pix[j] * p.out_cs + g * 8) = o;
        }
    }
}

template <int T, int NW>
int launch_ci(const ConvInParams& p, int N, hipStream_t s) {
    const dim3 grid((unsigned)((p.cout + 31) / 32), (unsigned)N), block(NW * 64);
    hipLaunchKernelGGL((convin_kernel<T, NW>), grid, block, 0, s, p);
    FM_HIP(hipGetLastError());
    return 0;
}

}  // namespace

constexpr int CONVIN_MAX_HW = 2048;        // 16 waves x 4 pixel tiles x 32 pixels

// the one rule behind Graph.convin_supported (models/graph.py) and the launch check below
bool convin_supported(int K, int cout, int hw) {
    return K >= 8 && K <= 4096 && K % 8 == 0 && cout >= 8 && cout <= 4096 && cout % 8 == 0 && hw >= 1 && hw <= CONVIN_MAX_HW;
}
extern "C" int fm_convin_supported(int K, int cout, int hw) { return convin_supported(K, cout, hw) ? 1 : 0; }

// w: [ceil32(cout)/32][ceil16(K)/16][64][8] fp16 (Graph._pack_frag); bias / gamma / beta: f32 [ceil32(cout)].  The tile shape
// is chosen on one sample's pixel count only.
int launch_convin(const f16* in, int in_cs, int in_coff, f16* out, int out_cs, int out_coff, const f16* res, int res_cs, int res_coff,
                  int res_mode, const f16* w, const float* bias, const float* gamma, const float* beta, int N, int HW, int K,
                  int cout, float eps, int act, hipStream_t s) {
    FM_CHECK_ARG(in && out && w && bias && gamma && beta && N >= 1 && N <= 65535 && convin_supported(K, cout, HW));
    FM_CHECK_ARG(in_cs % 8 == 0 && in_coff % 8 == 0 && in_coff >= 0 && in_coff + K <= in_cs && out_cs % 8 == 0 && out_coff % 8 == 0 &&
                 out_coff >= 0 && out_coff + cout <= out_cs);
    FM_CHECK_ARG(res_mode == RES_NONE || ((res_mode == RES_BEFORE_ACT || res_mode == CI_RES_BEFORE_NORM) && res && res_cs % 8 == 0 &&
                                          res_coff % 8 == 0 && res_coff >= 0 && res_coff + cout <= res_cs));
    FM_CHECK_ARG((act == ACT_LINEAR || act == ACT_RELU) && eps >= 0.f && eps < 1.f);
    ConvInParams p{};
    p.in = in; p.in_cs = in_cs; p.in_coff = in_coff;
    p.out = out; p.out_cs = out_cs; p.out_coff = out_coff;
    p.res = res; p.res_cs = res_cs; p.res_coff = res_coff; p.res_mode = res_mode;
    p.w = w; p.bias = bias; p.gamma = gamma; p.beta = beta;
    p.HW = HW; p.K = K; p.cout = cout; p.act = act; p.eps = eps;
    const int n_tiles = (HW + 31) / 32;
    if (n_tiles <= 4) return launch_ci<1, 4>(p, N, s);
    if (n_tiles <= 16) return launch_ci<1, 16>(p, N, s);
    if (n_tiles <= 32) return launch_ci<2, 16>(p, N, s);
    return launch_ci<4, 16>(p, N, s);
}
