// The ResNet stem with its max pool as ONE launch (FM_OP_STEMPOOL; emitted by models/onnx_graph.py only): 7x7 stride-2
// pad-3 conv 3 -> cout (cout <= 64, BN folded, ReLU), then the 3x3 stride-2 max pool in either padding form (pads 1, or
// pads 0 with ceil_mode).  In the mould of stemconv.hip / stem2.hip:
//   * a workgroup (4 waves) owns a tile of 7 x 7 POOLED outputs = 15 x 15 conv outputs (computed as a 16 x 16 tile whose
//     origin is conv row 2 py0 - ppad), for which it stages the 37 x 37 x 4-channel input patch in LDS -- from the input
//     tensor, or computed from the frame while staging (pixel_source.h, StemSrc kind 2: the extractor's crops), so that
//     neither a crop kernel nor an input tensor exists;
//   * the conv is stem_conv_kernel<7, 2>'s: D[cout][pixel] = sum_k W[cout][k] X[pixel][k], k = (kh, kw, c4), K = 196 padded
//     to 208 = 13 steps of v_mfma_f32_32x32x16_f16, the B operand = 2 taps x 4 channels read from the patch, the A operand
//     (32 couts) in registers; 64 couts are two passes over the same patch.  Same K order, same instruction sequence: for
//     cout <= 32 the conv tile equals FM_OP_STEMCONV's output bit for bit;
//   * bias + ReLU, ROUNDED TO FP16 -- what the unfused conv would have stored -- into an LDS tile [256][cout + 8]; conv
//     positions outside the conv map are stored as -inf, so that the pool ignores them (every window holds a valid tap);
//   * after one barrier, thread (pooled pixel, 8 channels) takes the max of its 9 taps from LDS and stores 16 bytes.
// The 128 x 64 x 64 conv output of ResNet-50 at 256 x 128 (52 MB at 50 crops) is never stored.  A conv output is computed
// by every pooled tile whose windows touch it: 256 / 196 = 1.31 x the conv work.
// LDS: patch 37 x 37 x 8 B = 10.7 KB, crop-normalisation table 1.5 KB, conv tile 256 x 72 x 2 B = 36 KB (cout 64): 48.2 KB.
#include "pixel_source.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int SP_PT = 7;                      // pooled tile side
constexpr int SP_KS = 7, SP_TAPS = 49, SP_KP = 208, SP_NKS = 13;
constexpr int SP_PW = 15 * 2 + SP_KS;         // 37: patch side

template <int SRC, int NCH>
__global__ __launch_bounds__(256) void stem_pool_kernel(const StemSrc src, const f16* __restrict__ in, int in_cs, int in_coff,
                                                        f16* __restrict__ out, int out_cs, int out_coff,
                                                        const f16* __restrict__ w, const float* __restrict__ bias,
                                                        int H, int W, int Hc, int Wc, int Hp, int Wp, int ppad, int cout_store) {
    constexpr int CTS = NCH * 32 + 8;         // conv tile row stride in halfs (16 B of padding)
    __shared__ __attribute__((aligned(16))) uint2 patch[SP_PW * SP_PW];
    __shared__ __attribute__((aligned(16))) f16 ct[256 * CTS];
    __shared__ f16 norm_lut[SRC == 2 ? 3 * 256 : 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int px0 = blockIdx.x * SP_PT, py0 = blockIdx.y * SP_PT;       // pooled tile origin
    const int cx0 = 2 * px0 - ppad, cy0 = 2 * py0 - ppad;               // conv tile origin (may be -1)
    const long n = blockIdx.z;
    const f16* img = in + n * (long)H * W * in_cs + in_coff;
    if constexpr (SRC == 2) {
        norm_lut[0 * 256 + tid] = crop_normalise(tid, 0);
        norm_lut[1 * 256 + tid] = crop_normalise(tid, 1);
        norm_lut[2 * 256 + tid] = crop_normalise(tid, 2);
        __syncthreads();
    }
    constexpr int NIT = (SP_PW * SP_PW + 255) / 256;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int i = tid + it * 256, ic = min(i, SP_PW * SP_PW - 1);
        const int iy = cy0 * 2 - 3 + ic / SP_PW, ix = cx0 * 2 - 3 + ic % SP_PW;
        const bool inside = iy >= 0 && iy < H && ix >= 0 && ix < W;
        const int cy = min(max(iy, 0), H - 1), cx = min(max(ix, 0), W - 1);
        uint2 v;
        if constexpr (SRC == 0) {
            v = *reinterpret_cast<const uint2*>(img + ((long)cy * W + cx) * in_cs);
        } else {
            int bgr[3];
            union { f16 h[4]; uint2 u; } pk;
            pk.u = make_uint2(0u, 0u);
            if (crop_u8_pixel(src.frame[0], src.fw, src.fh, src.boxes + n * 4, cx, cy, W, H, bgr)) {
                pk.h[0] = norm_lut[0 * 256 + bgr[2]]; pk.h[1] = norm_lut[1 * 256 + bgr[1]]; pk.h[2] = norm_lut[2 * 256 + bgr[0]];
            }
            v = pk.u;
        }
        if (!inside) v = make_uint2(0u, 0u);
        if (i < SP_PW * SP_PW) patch[i] = v;
    }
    __syncthreads();
    const int frow = lane & 31, fh = lane >> 5;
    const f16 ninf = -__builtin_inff16();
#pragma unroll 1
    for (int ch = 0; ch < NCH; ++ch) {
        f16x8 afr[SP_NKS];
#pragma unroll
        for (int ks = 0; ks < SP_NKS; ++ks)
            afr[ks] = *reinterpret_cast<const f16x8*>(w + (long)(ch * 32 + frow) * SP_KP + ks * 16 + fh * 8);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int mt = wave * 2 + t;                 // 8 tiles of 32 conv pixels = 2 rows of the 16 x 16 tile each
            const int ty = mt * 2 + (frow >> 4), tx = frow & 15;
            const int base = (ty * 2) * SP_PW + tx * 2;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < SP_NKS; ++ks) {
                const int t0 = fh ? 4 * ks + 2 : 4 * ks;
                const int tA = t0 < SP_TAPS ? t0 : SP_TAPS - 1, tB = t0 + 1 < SP_TAPS ? t0 + 1 : SP_TAPS - 1;   // (taps >= 49: zero weights)
                const uint2 a = patch[base + (tA / SP_KS) * SP_PW + tA % SP_KS];
                const uint2 b = patch[base + (tB / SP_KS) * SP_PW + tB % SP_KS];
                uint4 v = make_uint4(a.x, a.y, b.x, b.y);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(afr[ks], *reinterpret_cast<f16x8*>(&v), acc, 0, 0, 0);
            }
            const int cy = cy0 + ty, cx = cx0 + tx;
            const bool valid = cy >= 0 && cy < Hc && cx >= 0 && cx < Wc;
            f16* dst = ct + (ty * 16 + tx) * CTS + ch * 32;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = 8 * g + 4 * fh;
                const float4 bv = *reinterpret_cast<const float4*>(bias + ch * 32 + co);
                float a4[4] = {acc[4 * g + 0] + bv.x, acc[4 * g + 1] + bv.y, acc[4 * g + 2] + bv.z, acc[4 * g + 3] + bv.w};
                f16x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = valid ? (f16)act_relu(a4[e]) : ninf;
                *reinterpret_cast<f16x4*>(dst + co) = o;
            }
        }
    }
    __syncthreads();
    // pooled pixel (qy, qx) of the tile reads conv tile rows 2 qy .. 2 qy + 2 (<= 14), columns likewise
    const int c8 = cout_store >> 3;
    for (int it = tid; it < SP_PT * SP_PT * c8; it += 256) {
        const int pp = it / c8, cg = it - pp * c8;
        const int qy = pp / SP_PT, qx = pp - qy * SP_PT;
        const int gy = py0 + qy, gx = px0 + qx;
        if (gy >= Hp || gx >= Wp) continue;
        float m[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = -__builtin_inff();
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                float v[8];
                unpack8(*reinterpret_cast<const uint4*>(ct + ((2 * qy + dy) * 16 + 2 * qx + dx) * CTS + cg * 8), v);
#pragma unroll
                for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], v[e]);
            }
        *reinterpret_cast<uint4*>(out + ((n * Hp + gy) * (long)Wp + gx) * out_cs + out_coff + cg * 8) = pack8(m);
    }
}

template <int SRC>
int launch_kind(const StemSrc& src, const f16* in, int in_cs, int in_coff, f16* out, int out_cs, int out_coff, const f16* w,
                const float* bias, int N, int H, int W, int Hc, int Wc, int Hp, int Wp, int ppad, int cout, hipStream_t s) {
    const dim3 grid((Wp + SP_PT - 1) / SP_PT, (Hp + SP_PT - 1) / SP_PT, N), block(256);
    const int cs = (cout + 7) & ~7;
    if (cout <= 32)
        hipLaunchKernelGGL((stem_pool_kernel<SRC, 1>), grid, block, 0, s, src, in, in_cs, in_coff, out, out_cs, out_coff, w, bias,
                           H, W, Hc, Wc, Hp, Wp, ppad, cs);
    else
        hipLaunchKernelGGL((stem_pool_kernel<SRC, 2>), grid, block, 0, s, src, in, in_cs, in_coff, out, out_cs, out_coff, w, bias,
                           H, W, Hc, Wc, Hp, Wp, ppad, cs);
    FM_HIP(hipGetLastError());
    return 0;
}

}  // namespace

bool stempool_supported(int cout, int ppad) { return cout >= 8 && cout <= 64 && cout % 8 == 0 && (ppad == 0 || ppad == 1); }

// w: fp16 [ceil32(cout)][208], K order (kh, kw, c) with c < 4; bias f32 [ceil32(cout)].  (Hc, Wc): the conv map, (Hp, Wp):
// the pooled map; ppad 1: pool pads 1 on every side, 0: pads (0, 1) (ceil_mode).  src.kind 0 (tensor) or 2 (crops).
int launch_stempool_src(const StemSrc& src, const f16* in, int in_cs, int in_coff, f16* out, int out_cs, int out_coff,
                        const f16* w, const float* bias, int N, int H, int W, int Hc, int Wc, int Hp, int Wp, int ppad,
                        int cout, hipStream_t s) {
    FM_CHECK_ARG(stempool_supported(cout, ppad) && N >= 1 && N <= 65535 && H >= 1 && W >= 1 && out && w && bias);
    FM_CHECK_ARG(in_cs % 4 == 0 && in_coff % 4 == 0 && out_cs % 8 == 0 && out_coff % 8 == 0 && out_coff + ((cout + 7) & ~7) <= out_cs);
    FM_CHECK_ARG(Hc == (H + 6 - 7) / 2 + 1 && Wc == (W + 6 - 7) / 2 + 1 && Hc >= 1 && Wc >= 1);
    FM_CHECK_ARG(Hp == (Hc + ppad + 1 - 3) / 2 + 1 && Wp == (Wc + ppad + 1 - 3) / 2 + 1 && Hp >= 1 && Wp >= 1);
    FM_CHECK_ARG(src.kind == 0 ? in != nullptr : (src.kind == 2 && src.frame[0] && src.fw > 0 && src.fh > 0 && src.boxes));
    if (src.kind == 2) return launch_kind<2>(src, in, in_cs, in_coff, out, out_cs, out_coff, w, bias, N, H, W, Hc, Wc, Hp, Wp, ppad, cout, s);
    return launch_kind<0>(src, in, in_cs, in_coff, out, out_cs, out_coff, w, bias, N, H, W, Hc, Wc, Hp, Wp, ppad, cout, s);
}
