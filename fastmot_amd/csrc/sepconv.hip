// MobileNet separable block in one launch (FM_OP_SEPCONV):
//   t = act1(dw3x3(x) + b_dw)          depthwise 3x3, stride 1 or 2, TF "SAME" padding (asymmetric at stride 2)
//   y = act2(W_pw t + b_pw)            pointwise 1x1, cin -> cout
// -- TF-slim MobileNetV1's Conv2d_{i}_depthwise + Conv2d_{i}_pointwise (BN folded, ReLU6 on both).  Unfused, the depthwise
// tensor goes to HBM and comes back (FM_OP_DWCONV + a 1x1 conv); here it is never stored.
//
// A workgroup (4 waves) owns BN = 32 * PT consecutive output pixels of the flat [N * Ho * Wo] index (a tile may straddle a
// sample boundary: every pixel is decomposed on its own) and CT cout tiles of 32.  K = cin is walked in chunks of KC
// channels:
//   phase A  all 256 threads compute the depthwise result of (pixel, 8-channel group) items straight from global memory
//            (16-byte loads, consecutive threads = consecutive channel groups of one pixel), the same fmaf chain in the
//            same tap order as dwconv_kernel (ops.hip), + bias + act1, ROUNDED TO FP16 -- exactly what the unfused layer
//            would have stored -- into an LDS tile [BN][KC + 8] (rows padded by 16 B, as pair11.hip pads its tiles);
//   phase B  wave w multiplies pixel tile w % PT by its share of the cout tiles: B fragments from the LDS tile, A
//            fragments (the pointwise weights in MFMA fragment order, Graph._pack_frag) straight from L2, 16-wide K steps
//            in ascending order into the same accumulators.
// Two LDS tiles alternate, so one barrier per chunk suffices: the depthwise of chunk k + 1 may start while other waves
// still multiply chunk k.  LDS: 2 * BN * (KC + 8) * 2 B = 36.0 KB (PT 4, KC 64) / 33.0 KB (PT 1, KC 256).
// Channels of a chunk beyond cin (cin % 16 == 8) are written as zeros; the packed weights are zero there too.
#include "net.h"

namespace {

struct SepParams {
    const f16* in;  int in_cs, in_coff;
    f16* out;       int out_cs, out_coff;
    const f16* wdw;         // [9][cin] fp16
    const float* bdw;       // f32 [cin]
    const f16* wpw;         // [ceil32(cout) / 32][ceil16(cin) / 16][64][8] fp16
    const float* bpw;       // f32 [ceil32(cout)]
    int H, W, Ho, Wo, cin, cout, stride, pad_y, pad_x, act1, act2;
    long P;                 // N * Ho * Wo
};

template <int PT, int CT, int KC>
__global__ __launch_bounds__(256) void sepconv_kernel(const SepParams p) {
    constexpr int BN = 32 * PT, S = KC + 8, WPT = 4 / PT, NACC = CT / WPT;
    static_assert(4 % PT == 0 && CT % WPT == 0 && KC % 16 == 0, "tile shape");
    __shared__ __attribute__((aligned(16))) f16 tile[2][BN * S];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 31, fh = lane >> 5;
    const int pt = wave % PT, part = wave / PT;
    const long p0 = (long)blockIdx.x * BN;
    const int ct0 = blockIdx.y * CT;                        // first cout tile of this workgroup
    const int n_ct = (p.cout + 31) >> 5;
    const int k16 = (p.cin + 15) >> 4;                      // K steps of the packed weights
    const int hw = p.Ho * p.Wo;

    f32x16 acc[NACC];
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    int buf = 0;
    for (int kc0 = 0; kc0 < k16 * 16; kc0 += KC, buf ^= 1) {
        const int kw = min(KC, k16 * 16 - kc0);             // channels of this chunk (multiple of 16)
        const int g8 = kw >> 3;
        // ---- phase A: depthwise + bias + act1 -> fp16 -> LDS
        for (int e = tid; e < BN * g8; e += 256) {
            const int row = e / g8, c = kc0 + (e - row * g8) * 8;
            uint4 packed = make_uint4(0, 0, 0, 0);
            if (c < p.cin) {
                const long pix = min(p0 + row, p.P - 1);
                const long n = pix / hw;
                const int rem = (int)(pix - n * hw);
                const int yo = rem / p.Wo, xo = rem - yo * p.Wo;
                const int y0 = yo * p.stride - p.pad_y, x0 = xo * p.stride - p.pad_x;
                const f16* src = p.in + n * p.H * p.W * p.in_cs + p.in_coff + c;
                float a[8];
                {
                    const float4 b0 = *reinterpret_cast<const float4*>(p.bdw + c), b1 = *reinterpret_cast<const float4*>(p.bdw + c + 4);
                    a[0] = b0.x; a[1] = b0.y; a[2] = b0.z; a[3] = b0.w; a[4] = b1.x; a[5] = b1.y; a[6] = b1.z; a[7] = b1.w;
                }
                // all nine taps (and their weights) are requested before the first is used -- addresses clamped into the map,
                // taps outside it skipped in the arithmetic only: with a branch around each load the taps were nine dependent
                // trips to memory per item
                uint4 raw[9], wk[9];
                bool ok[9];
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int yy = y0 + t / 3, xx = x0 + t % 3;
                    ok[t] = yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
                    const int yc = min(max(yy, 0), p.H - 1), xc = min(max(xx, 0), p.W - 1);
                    raw[t] = *reinterpret_cast<const uint4*>(src + ((long)yc * p.W + xc) * p.in_cs);
                    wk[t] = *reinterpret_cast<const uint4*>(p.wdw + t * p.cin + c);
                }
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    if (!ok[t]) continue;
                    float v[8], k[8];
                    unpack8(raw[t], v);
                    unpack8(wk[t], k);
#pragma unroll
                    for (int q = 0; q < 8; ++q) a[q] = fmaf(v[q], k[q], a[q]);
                }
                apply_act_n<8>(a, p.act1);
                packed = pack8(a);
            }
            *reinterpret_cast<uint4*>(&tile[buf][row * S + (c - kc0)]) = packed;
        }
        __syncthreads();
        // ---- phase B: this wave's pixel tile x its cout tiles, K steps of this chunk
        const f16* brow = &tile[buf][(pt * 32 + frow) * S + fh * 8];
        // (branch-free: a cout tile beyond the last one multiplies the last tile's weights again and is never stored, so that
        // the weight loads of several K steps can be in flight at once)
        const f16* wrow[NACC];
#pragma unroll
        for (int j = 0; j < NACC; ++j)
            wrow[j] = p.wpw + (((long)min(ct0 + part + j * WPT, n_ct - 1) * k16 + (kc0 >> 4)) * 64 + lane) * 8;
#pragma unroll 4
        for (int ks = 0; ks < (kw >> 4); ++ks) {
            const f16x8 fb = *reinterpret_cast<const f16x8*>(brow + ks * 16);
#pragma unroll
            for (int j = 0; j < NACC; ++j) {
                const f16x8 fa = *reinterpret_cast<const f16x8*>(wrow[j] + (long)ks * 512);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa, fb, acc[j], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: bias + act2, NHWC fp16 stores (lane = pixel, registers = 4-channel groups of the cout tile)
    const long pix = p0 + pt * 32 + frow;
    if (pix >= p.P) return;
#pragma unroll
    for (int j = 0; j < NACC; ++j) {
        const int ct = ct0 + part + j * WPT;
        if (ct >= n_ct) continue;
        f16* dst = p.out + pix * p.out_cs + p.out_coff + ct * 32;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int co = ct * 32 + g * 8 + fh * 4;
            if (co >= p.cout) continue;                      // (cout % 8 == 0: a 4-channel group is all in or all out)
            const float4 bv = *reinterpret_cast<const float4*>(p.bpw + co);
            float a4[4] = {acc[j][4 * g + 0] + bv.x, acc[j][4 * g + 1] + bv.y, acc[j][4 * g + 2] + bv.z, acc[j][4 * g + 3] + bv.w};
            apply_act_n<4>(a4, p.act2);
            f16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (f16)a4[e];
            *reinterpret_cast<f16x4*>(dst + g * 8 + fh * 4) = o;
        }
    }
}

template <int PT, int CT, int KC>
int launch_sep(const SepParams& p, hipStream_t s) {
    const int n_ct = (p.cout + 31) / 32;
    const dim3 grid((unsigned)((p.P + 32 * PT - 1) / (32 * PT)), (unsigned)((n_ct + CT - 1) / CT)), block(256);
    hipLaunchKernelGGL((sepconv_kernel<PT, CT, KC>), grid, block, 0, s, p);
    FM_HIP(hipGetLastError());
    return 0;
}

}  // namespace

// the one rule behind Graph.sepconv_supported (models/graph.py) and the launch check below
bool sepconv_supported(int cin, int cout, int stride) {
    return cin >= 8 && cin <= 2048 && cin % 8 == 0 && cout >= 8 && cout <= 2048 && cout % 8 == 0 && (stride == 1 || stride == 2);
}
extern "C" int fm_sepconv_supported(int cin, int cout, int stride) { return sepconv_supported(cin, cout, stride) ? 1 : 0; }

// TF "SAME" padding of a 3-tap window: out = ceil(in / stride), total = max((out - 1) * stride + 3 - in, 0), before = total / 2
int tf_same_pad_before(int in, int out, int stride) {
    const int total = (out - 1) * stride + 3 - in;
    return total > 0 ? total / 2 : 0;
}

// wdw [9][cin] fp16, bdw f32[cin]; wpw [ceil32(cout)/32][ceil16(cin)/16][64][8] fp16 (Graph._pack_frag), bpw f32[ceil32(cout)].
// p_choice: the pixel count the tile shape is chosen on (the detector net passes one sample's, so that the same instance
// runs at every batch size; the summation order per output element does not depend on the instance anyway).
int launch_sepconv(const f16* in, int in_cs, int in_coff, f16* out, int out_cs, int out_coff, const f16* wdw,
                   const float* bdw, const f16* wpw, const float* bpw, int N, int H, int W, int Ho, int Wo, int cin,
                   int cout, int stride, int act1, int act2, long p_choice, hipStream_t s) {
    FM_CHECK_ARG(sepconv_supported(cin, cout, stride) && in_cs % 8 == 0 && in_coff % 8 == 0 && out_cs % 4 == 0 && out_coff % 4 == 0);
    FM_CHECK_ARG(N > 0 && H > 0 && W > 0 && Ho == (H + stride - 1) / stride && Wo == (W + stride - 1) / stride);
    SepParams p{};
    p.in = in; p.in_cs = in_cs; p.in_coff = in_coff;
    p.out = out; p.out_cs = out_cs; p.out_coff = out_coff;
    p.wdw = wdw; p.bdw = bdw; p.wpw = wpw; p.bpw = bpw;
    p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo; p.cin = cin; p.cout = cout; p.stride = stride;
    p.pad_y = tf_same_pad_before(H, Ho, stride);
    p.pad_x = tf_same_pad_before(W, Wo, stride);
    p.act1 = act1; p.act2 = act2;
    p.P = (long)N * Ho * Wo;
    // large maps with few channels: 128-pixel tiles, 4 cout tiles per workgroup; otherwise 32-pixel tiles, 4 cout tiles (one
    // per wave: the small maps need the workgroups more than they mind recomputing the depthwise tile per cout slice)
    if (p_choice >= 2048 && cin <= 256) return launch_sep<4, 4, 64>(p, s);
    return launch_sep<1, 4, 256>(p, s);
}
