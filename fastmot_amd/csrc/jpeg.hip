// Entropy-decoded JPEG -> packed BGR u8: the device half of the JPEG ingest path, behind fm_frame_upload_jpeg /
// fm_frame_upload_ahead_jpeg / fm_frame_ring_store_jpeg (frames.hip).  The frame arrives in a device
// staging buffer as quantised coefficients (int16, per component [block_row][block_col][64] over the MCU-padded grid,
// row-major inside a block) plus one 64-entry quantisation table per component -- what jpeg_host.hip's Huffman decoder
// wrote on the host -- and leaves as the BGR frame every consumer already reads, so nothing downstream knows where the
// frame came from.
//
// The arithmetic is libjpeg-turbo's default decode path, integer and exact (fastmot_amd/utils/jpeg.py states it in numpy,
// include/fastmot_hip.h and DESIGN 11d in words; tests compare bit for bit against Pillow): dequantise, "ISLOW" inverse
// DCT (columns with a descale by 11 bits, rows by 18), + 128, clamp; "fancy" chroma upsampling over the chroma plane's
// real samples; YCbCr -> BGR in 16-bit fixed point.
//
// Two launches on the copy's stream:
//   jpeg_idct_kernel      coefficients -> u8 sample planes of every component at their own resolution (MCU padding
//                         included), in the same staging allocation.  Eight lanes own one 8 x 8 block: lane j loads row j
//                         (8 int16 = 16 bytes, so a wavefront reads 1 KiB contiguous per instruction), dequantises it and
//                         puts it into LDS; lane c then takes column c out of LDS, runs the column pass and puts the
//                         result back in place; lane r takes row r, runs the row pass and stores 8 sample bytes.  The
//                         transpose between the passes goes through LDS only.  A block's 64 words are 72 words apart from
//                         the next block's, which spreads the four blocks of a 32-lane ds_read_b32 group over all banks.
//   jpeg_to_bgr_kernel    sample planes -> BGR.  One thread owns 8 pixels of one row: 8 Y bytes, the chroma samples under
//                         them with one neighbour on either side (and the nearer chroma row above / below for 4:2:0), the
//                         triangle filter, the colour conversion, 24 BGR bytes out (bgr_run.h): three 8-byte stores for
//                         frames whose width is a multiple of 8, 4-byte stores for multiples of 4, bytes otherwise.
// The one-launch form (a workgroup's chroma blocks plus a recomputed halo kept in LDS) would save the sample planes'
// round trip, 1.5 bytes per pixel written and read again out of L2.  The two launches together measure 17 us for a
// 1080p 4:2:0 frame, 13 % of the copy they follow (profiles/jpeg_ingest.txt), so the simpler form was kept.
//
// No load or store address depends on a coefficient's value, so no coefficient values can make the kernels fault.
#include "common.h"
#include "bgr_run.h"
#include "yuv_coef.h"      // clamp8

namespace {

struct JpegGeo {
    int W, H;                 // image
    int ncomp, hs, vs;        // luma sampling factors (1, 1 for one component)
    int fancy;                // triangle-filter chroma upsampling (chroma plane wider than 2 samples)
    int CW, CH;               // real chroma samples: ceil(W / hs), ceil(H / vs)
    int bw0, bw1;             // blocks per row of the luma / chroma planes
    int nb0, nb1;             // blocks of the luma plane / of one chroma plane
    long long off1, off2;     // first sample of Cb, Cr in the sample buffer (= first coefficient in the coefficient buffer)
};

constexpr int BLK_STRIDE = 72;            // words of LDS per block (64 used)
constexpr int IDCT_THREADS = 256;         // 32 blocks per workgroup

// One 1-D pass of the ISLOW inverse DCT on in[0..7], results in place, before the descale.
__device__ __forceinline__ void idct_1d(int (&v)[8]) {
    int z1 = (v[2] + v[6]) * 4433;
    const int tmp2 = z1 - v[6] * 15137;
    const int tmp3 = z1 + v[2] * 6270;
    const int tmp0 = (v[0] + v[4]) * 8192;
    const int tmp1 = (v[0] - v[4]) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    int t0 = v[7], t1 = v[5], t2 = v[3], t3 = v[1];
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = (z3 + z4) * 9633;
    t0 *= 2446, t1 *= 16819, t2 *= 25172, t3 *= 12299;
    z1 *= -7373, z2 *= -20995;
    z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
    v[0] = tmp10 + t3, v[7] = tmp10 - t3;
    v[1] = tmp11 + t2, v[6] = tmp11 - t2;
    v[2] = tmp12 + t1, v[5] = tmp12 - t1;
    v[3] = tmp13 + t0, v[4] = tmp13 - t0;
}

// clamp(((x + 2^17) >> 18) + 128, 0, 255), written as a clamp followed by the shift (the same value for every x that
// does not overflow): in the order shift - clamp - pack this compiler forms v_ashr_pk_u8_i32 and mishandles the
// destination's upper half (see yuv_coef.h sat8).
__device__ __forceinline__ uint32_t descale_sample(int x) {
    constexpr int S = 18;
    return (uint32_t)min(max(x + (1 << (S - 1)) + (128 << S), 0), (256 << S) - 1) >> S;
}

__global__ __launch_bounds__(IDCT_THREADS) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const uint16_t* __restrict__ qt,
                                                                 uint8_t* __restrict__ samples, JpegGeo g) {
    __shared__ int ws[(IDCT_THREADS / 8) * BLK_STRIDE];
    const long long nblocks = (long long)g.nb0 + (g.ncomp == 3 ? 2ll * g.nb1 : 0);
    const long long blk = (long long)blockIdx.x * (IDCT_THREADS / 8) + (threadIdx.x >> 3);
    const int j = threadIdx.x & 7;
    const bool active = blk < nblocks;
    int* const w = ws + (threadIdx.x >> 3) * BLK_STRIDE;

    int comp = 0, bw = g.bw0;
    long long local = blk, plane = 0;                  // block index inside its component; first sample of the component
    if (blk >= g.nb0) {
        comp = blk >= (long long)g.nb0 + g.nb1 ? 2 : 1;
        local = blk - g.nb0 - (comp == 2 ? g.nb1 : 0);
        bw = g.bw1;
        plane = comp == 2 ? g.off2 : g.off1;
    }

    if (active) {                                      // row j, dequantised
        const uint4 c = *reinterpret_cast<const uint4*>(coef + blk * 64 + j * 8);
        const uint4 q = *reinterpret_cast<const uint4*>(qt + comp * 64 + j * 8);
        const uint32_t cw[4] = {c.x, c.y, c.z, c.w}, qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int cv = (int)(int16_t)(cw[k >> 1] >> ((k & 1) * 16));
            const int qv = (int)((qw[k >> 1] >> ((k & 1) * 16)) & 0xffffu);
            w[j * 8 + k] = cv * qv;
        }
    }
    __syncthreads();
    if (active) {                                      // column j
        int v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = w[r * 8 + j];
        idct_1d(v);
#pragma unroll
        for (int r = 0; r < 8; ++r) w[r * 8 + j] = (v[r] + (1 << 10)) >> 11;
    }
    __syncthreads();
    if (active) {                                      // row j
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = w[j * 8 + k];
        idct_1d(v);
        uint32_t o[2] = {0, 0};
#pragma unroll
        for (int k = 0; k < 8; ++k) put_byte(o, k, descale_sample(v[k]));
        const long long brow = (int)local / bw, bcol = local - brow * bw;
        uint8_t* const out = samples + plane + ((brow * 8 + j) * bw + bcol) * 8;
        *reinterpret_cast<uint2*>(out) = make_uint2(o[0], o[1]);
    }
}

// The 8 chroma values under pixels x0 .. x0 + 7 of row y, from one chroma plane.
__device__ __forceinline__ void chroma8(const uint8_t* __restrict__ plane, const JpegGeo& g, int pitch, int x0, int y, int (&out)[8]) {
    if (g.hs == 1) {
        const uint2 a = *reinterpret_cast<const uint2*>(plane + (size_t)y * pitch + x0);
        const uint32_t w[2] = {a.x, a.y};
#pragma unroll
        for (int i = 0; i < 8; ++i) out[i] = (int)run_byte(w, i);
        return;
    }
    const bool v2 = g.vs == 2, tri2 = v2 && g.fancy;
    const int cr = v2 ? y >> 1 : y;
    const int nr = min(max(cr + ((y & 1) ? 1 : -1), 0), g.CH - 1);
    const uint8_t* const cur = plane + (size_t)cr * pitch;
    const uint8_t* const near = plane + (size_t)nr * pitch;
    const int c0 = x0 >> 1;
    int t[6];                                          // samples c0 - 1 .. c0 + 4, indices clamped to the real plane
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int c = min(max(c0 - 1 + k, 0), g.CW - 1);
        t[k] = tri2 ? 3 * (int)cur[c] + (int)near[c] : (int)cur[c];
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int m = t[p + 1];
        if (!g.fancy) {
            out[2 * p] = out[2 * p + 1] = m;
        } else if (v2) {
            out[2 * p] = (3 * m + t[p] + 8) >> 4;
            out[2 * p + 1] = (3 * m + t[p + 2] + 7) >> 4;
        } else {
            out[2 * p] = (3 * m + t[p] + 1) >> 2;
            out[2 * p + 1] = (3 * m + t[p + 2] + 2) >> 2;
        }
    }
}

// ALIGN: what the frame's rows allow -- 8: width % 8 == 0 and an 8-byte aligned frame, StoreRule::ALIGNED8; 4: width % 4
// == 0, 4-byte stores; 1: StoreRule::BYTES.  Pixels past the row's end are computed from the planes' padding and not stored.
template <int ALIGN>
__global__ __launch_bounds__(256) void jpeg_to_bgr_kernel(const uint8_t* __restrict__ samples, uint8_t* __restrict__ bgr, JpegGeo g) {
    int y, x0, n;
    if (!run_of(g.W, g.H, y, x0, n)) return;
    const int pitch0 = g.bw0 * 8, pitch1 = g.bw1 * 8;

    const uint2 yy = *reinterpret_cast<const uint2*>(samples + (size_t)y * pitch0 + x0);
    const uint32_t yw[2] = {yy.x, yy.y};
    int cb[8], cr[8];
    if (g.ncomp == 3) {
        chroma8(samples + g.off1, g, pitch1, x0, y, cb);
        chroma8(samples + g.off2, g, pitch1, x0, y, cr);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) cb[i] = cr[i] = 128;    // B = G = R = Y
    }

    uint32_t o[6] = {};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int Y = (int)run_byte(yw, i);
        const int b = cb[i] - 128, r = cr[i] - 128;
        put_px(o, i, clamp8(Y + ((116130 * b + 32768) >> 16)), clamp8(Y + ((-22554 * b - 46802 * r + 32768) >> 16)),
               clamp8(Y + ((91881 * r + 32768) >> 16)));
    }

    uint8_t* const out = bgr + ((size_t)y * g.W + x0) * 3;
    if (ALIGN == 4) {                                      // (a run of 4 pixels is whole words: W % 4 == 0)
#pragma unroll
        for (int q = 0; q < 6; ++q)
            if (x0 + (4 * q + 3) / 3 < g.W) reinterpret_cast<uint32_t*>(out)[q] = o[q];
    } else {
        store_run<ALIGN == 8 ? StoreRule::ALIGNED8 : StoreRule::BYTES>(out, n, o);
    }
}

}  // namespace

size_t fm_jpeg_sample_offset(long long coef_count) { return ((size_t)coef_count * 2 + 3 * 64 * 2 + 15) & ~(size_t)15; }

// Decodes the frame whose coefficients lie at `stage` (int16 x coef_count, then 3 x 64 uint16 quantisation entries) into
// w * h * 3 BGR bytes at `bgr`, on stream `s`; the sample planes go to stage + fm_jpeg_sample_offset(coef_count), coef_count
// bytes.  `info` has been checked by the caller, grid sizes included (jpeg_layout_ok in frames.hip); `stage` is 16-byte aligned.
int fm_jpeg_to_bgr(const uint8_t* stage, uint8_t* bgr, const struct fm_jpeg_info* info, hipStream_t s) {
    FM_CHECK_ARG(stage && bgr && info && !((uintptr_t)stage & 15));
    JpegGeo g;
    g.W = info->width, g.H = info->height, g.ncomp = info->ncomp;
    g.hs = info->ncomp == 3 ? info->hsamp[0] : 1, g.vs = info->ncomp == 3 ? info->vsamp[0] : 1;
    g.CW = (g.W + g.hs - 1) / g.hs, g.CH = (g.H + g.vs - 1) / g.vs;
    g.fancy = g.hs == 2 && g.CW > 2;
    g.bw0 = info->blocks_w[0], g.bw1 = info->blocks_w[1];
    g.nb0 = info->blocks_w[0] * info->blocks_h[0], g.nb1 = info->blocks_w[1] * info->blocks_h[1];
    g.off1 = info->coef_offset[1], g.off2 = info->coef_offset[2];
    const long long nblocks = info->coef_count / 64;
    const long long threads2 = (long long)((g.W + 7) >> 3) * g.H;
    const int16_t* const coef = reinterpret_cast<const int16_t*>(stage);
    const uint16_t* const qt = reinterpret_cast<const uint16_t*>(stage) + info->coef_count;
    uint8_t* const samples = const_cast<uint8_t*>(stage) + fm_jpeg_sample_offset(info->coef_count);
    constexpr int per_wg = IDCT_THREADS / 8;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((nblocks + per_wg - 1) / per_wg)), dim3(IDCT_THREADS), 0, s, coef, qt, samples, g);
    FM_HIP(hipGetLastError());
    const dim3 grid((unsigned)((threads2 + 255) / 256));
    if (g.W % 8 == 0 && !((uintptr_t)bgr & 7))
        hipLaunchKernelGGL(jpeg_to_bgr_kernel<8>, grid, dim3(256), 0, s, samples, bgr, g);
    else if (g.W % 4 == 0 && !((uintptr_t)bgr & 3))
        hipLaunchKernelGGL(jpeg_to_bgr_kernel<4>, grid, dim3(256), 0, s, samples, bgr, g);
    else
        hipLaunchKernelGGL(jpeg_to_bgr_kernel<1>, grid, dim3(256), 0, s, samples, bgr, g);
    FM_HIP(hipGetLastError());
    return 0;
}
