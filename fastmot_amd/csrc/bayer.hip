// Bayer mosaic (one sample per pixel: 8 bits, or 10 / 12 / 14 / 16 bits in a little-endian 16-bit word) -> packed BGR u8:
// the kernel behind fm_frame_upload_bayer / fm_frame_upload_ahead_bayer / fm_frame_ring_store_bayer (frames.hip).
// This is what industrial and embedded cameras hand out (GigE Vision / USB3 Vision BayerRG8 / BayerRG12, V4L2
// SRGGB8 / SRGGB10, CSI sensors).  The frame arrives in device staging with its rows packed to their width (W or 2 W
// bytes) and leaves as the BGR frame every consumer reads.  fastmot_amd/utils/bayer.py states the arithmetic in numpy
// (sample preparation, reflect-101 borders, the bilinear and the Malvar-He-Cutler filters); tests compare bit for bit.
//
// A 256-thread workgroup owns a tile of TW x TH = 128 x 16 output pixels.
// Phase 1: the PREPARED 8-bit samples (black level, the position's gain, the depth: once per sample, here) of the tile
//   and its 2-sample halo go to LDS, 20 rows of 136 bytes: LDS column j holds image column tx0 - 4 + j, so that a tile
//   -- and every thread's run -- begins on a 4-byte boundary of both the LDS row and, where the source row's address
//   allows, of the source row.  The unit of staging is one word of four samples: one 4-byte (8-byte for 16-bit samples)
//   load where the four columns lie inside the frame and the address is aligned, four index-reflected single loads
//   otherwise (the frame's left and right edge, rows of an odd width).  The reflection is arithmetic on the index --
//   reflect(i, n) always lands in 0 .. n - 1, whatever i is --, no branch per sample and no address that could leave the
//   frame.  A reflected index keeps its parity, so the gain follows from the parity of the unreflected one.
// Phase 2: a thread produces 8 horizontally adjacent pixels of one row: from each of the 5 rows under it two aligned
//   8-byte LDS reads (the 12 samples it needs lie in 16), bytes picked with constant shifts.  The rows of one wavefront
//   share their parity (a wavefront takes every other row of 8), so which of a run's pixels are colour sites and which
//   green sites is the same in all 64 lanes: the one branch on it is wave-uniform, everything else is straight-line.
//   The 24 BGR bytes leave by bgr_run.h's StoreRule::BY_ADDRESS: three 8-byte stores where the run is whole and its first
//   byte 8-byte aligned, six 4-byte stores where it is 4-byte aligned, bytes otherwise -- decided per thread.
// No address depends on a sample's value.  LDS: 2720 bytes.
#include "common.h"
#include "bgr_run.h"

namespace {

constexpr int TW = 128, TH = 16;             // output pixels of a workgroup
constexpr int LW = TW + 8, LH = TH + 4;      // staged samples: image columns tx0 - 4 .. tx0 + 131, rows ty0 - 2 .. ty0 + 17
constexpr int LWORDS = LW / 4;

// reflect-101 of any index into 0 .. n - 1 (n >= 2)
__device__ __forceinline__ int reflect(int i, int n) {
    const int m = 2 * (n - 1);
    i %= m;
    if (i < 0) i += m;
    return i >= n ? m - i : i;
}

__device__ __forceinline__ uint32_t prep(uint32_t s, int black, uint32_t gain, int depth) {
    const uint32_t v = (uint32_t)max((int)s - black, 0);
    return min(255u, (v * gain + (1u << (depth - 1))) >> depth);
}

// byte k of the 16 staged samples of one row
__device__ __forceinline__ int bt(const uint32_t (&w)[4], int k) { return (int)run_byte(w, k); }

__device__ __forceinline__ int fin(int sum) { return min(max((sum + 8) >> 4, 0), 255); }

// The 8 pixels of a run.  r[2] is the run's own row, r[0] .. r[4] the rows above and below; pixel i's sample is byte
// 4 + i of a row.  SITE0: pixel 0 (and 2, 4, 6) is a colour site -- R in a row R sits in, B otherwise -- and the odd
// ones green sites; the reverse without.  r_row: the row is one R sits in.
template <int METHOD, bool SITE0>
__device__ __forceinline__ void demosaic_run(const uint32_t (&r)[5][4], bool r_row, uint32_t (&o)[6]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = 4 + i;
        const int c = bt(r[2], k);
        const int hor = bt(r[2], k - 1) + bt(r[2], k + 1), ver = bt(r[1], k) + bt(r[3], k);
        const int diag = bt(r[1], k - 1) + bt(r[1], k + 1) + bt(r[3], k - 1) + bt(r[3], k + 1);
        const bool site = SITE0 == !(i & 1);
        int first, second;              // site: G and the opposite colour; green site: the row's colour and the other one
        if (METHOD == FM_BAYER_BILINEAR) {
            if (site) first = (hor + ver + 2) >> 2, second = (diag + 2) >> 2;
            else first = (hor + 1) >> 1, second = (ver + 1) >> 1;
        } else {
            const int h2 = bt(r[2], k - 2) + bt(r[2], k + 2), v2 = bt(r[0], k) + bt(r[4], k);
            if (site) {
                first = fin(8 * c + 4 * (hor + ver) - 2 * (h2 + v2));
                second = fin(12 * c + 4 * diag - 3 * (h2 + v2));
            } else {
                first = fin(10 * c + 8 * hor - 2 * diag - 2 * h2 + v2);
                second = fin(10 * c + 8 * ver - 2 * diag - 2 * v2 + h2);
            }
        }
        if (site) put_px(o, i, r_row ? second : c, first, r_row ? c : second);
        else put_px(o, i, r_row ? second : first, c, r_row ? first : second);
    }
}

// src: H rows of W samples of BPS bytes, packed (row r at src + r * W * BPS); gain_r / gain_g / gain_b in 1/256 units.
template <int BPS, int METHOD>
__global__ __launch_bounds__(256) void bayer_to_bgr_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ bgr, int W, int H,
                                                           int pattern, int depth, int black, uint32_t gain_r, uint32_t gain_g,
                                                           uint32_t gain_b) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[LH * LWORDS];
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const int pcx = pattern & 1, pcy = pattern >> 1;       // the parities of R's column and row
    const size_t rb = (size_t)W * BPS;

    for (int e = threadIdx.x; e < LH * LWORDS; e += 256) {
        const int ly = e / LWORDS, lw = e - ly * LWORDS;
        const int y = ty0 - 2 + ly, x = tx0 - 4 + 4 * lw;  // (x is even: sample j of the word has the parity of j)
        const bool ry = ((y ^ pcy) & 1) == 0;              // a row R sits in
        // the gains of the word's even and odd samples: the colour at column parity pcx is R (B) in a row R (B) sits in
        const uint32_t g_own = ry ? gain_r : gain_g, g_opp = ry ? gain_g : gain_b;
        const uint32_t g_even = pcx ? g_opp : g_own, g_odd = pcx ? g_own : g_opp;
        const uint8_t* const row = src + (size_t)reflect(y, H) * rb;
        uint32_t s[4];
        const uint8_t* const p = row + (ptrdiff_t)x * BPS;
        if (x >= 0 && x + 3 < W && !((uintptr_t)p & (4 * BPS - 1))) {
            if (BPS == 1) {
                const uint32_t a = *reinterpret_cast<const uint32_t*>(p);
                s[0] = a & 0xffu, s[1] = (a >> 8) & 0xffu, s[2] = (a >> 16) & 0xffu, s[3] = a >> 24;
            } else {
                const uint2 a = *reinterpret_cast<const uint2*>(p);
                s[0] = a.x & 0xffffu, s[1] = a.x >> 16, s[2] = a.y & 0xffffu, s[3] = a.y >> 16;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int xr = reflect(x + j, W);
                s[j] = BPS == 1 ? (uint32_t)row[xr] : (uint32_t)reinterpret_cast<const uint16_t*>(row)[xr];
            }
        }
        tile[e] = prep(s[0], black, g_even, depth) | prep(s[1], black, g_odd, depth) << 8 | prep(s[2], black, g_even, depth) << 16 |
                  prep(s[3], black, g_odd, depth) << 24;
    }
    __syncthreads();

    // wavefront v: rows (v >> 1) * 8 + (v & 1) + 2 * (0 .. 3) of the tile, 16 lanes of 8 pixels a row
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ty = (wave >> 1) * 8 + (wave & 1) + 2 * (lane >> 4), t = lane & 15;
    const int y = ty0 + ty, x0 = tx0 + 8 * t;
    if (y >= H || x0 >= W) return;
    const int n = min(8, W - x0);

    uint32_t r[5][4];
#pragma unroll
    for (int d = 0; d < 5; ++d) {                          // image rows y - 2 .. y + 2 are staged rows ty .. ty + 4
        const uint2* const q = reinterpret_cast<const uint2*>(tile + (ty + d) * LWORDS + 2 * t);
        const uint2 a = q[0], b = q[1];
        r[d][0] = a.x, r[d][1] = a.y, r[d][2] = b.x, r[d][3] = b.y;
    }
    const bool r_row = ((y ^ pcy) & 1) == 0;
    // pixel 0 (an even column) is a colour site where its column parity class equals the row's: R in R's column and
    // row, B in B's column and row
    const bool site0 = (pcx == 0) == r_row;
    uint32_t o[6] = {};
    if (site0) demosaic_run<METHOD, true>(r, r_row, o);
    else demosaic_run<METHOD, false>(r, r_row, o);
    store_run<StoreRule::BY_ADDRESS>(bgr + ((size_t)y * W + x0) * 3, n, o);
}

}  // namespace

// Demosaics the mosaic at `src` (h rows of w samples, packed: 1 byte each for depth 8, 2 above -- then 2-byte aligned)
// to w * h * 3 BGR bytes at `bgr`, on stream `s`.  The callers have checked the arguments.
int fm_bayer_to_bgr(const uint8_t* src, uint8_t* bgr, int w, int h, int pattern, int depth, int method, int black, int gain_r, int gain_g,
                    int gain_b, hipStream_t s) {
    FM_CHECK_ARG(src && bgr && w >= 2 && h >= 2 && w <= FM_SRC_MAX_DIM && h <= FM_SRC_MAX_DIM && fm_bayer_sample_bytes(depth) &&
                 pattern >= FM_BAYER_RGGB && pattern <= FM_BAYER_BGGR && (method == FM_BAYER_BILINEAR || method == FM_BAYER_MHC) &&
                 black >= 0 && black < (1 << depth) && fm_bayer_gain_ok(gain_r) && fm_bayer_gain_ok(gain_g) && fm_bayer_gain_ok(gain_b));
    const int bps = fm_bayer_sample_bytes(depth);
    FM_CHECK_ARG(!((uintptr_t)src & (bps - 1)));
    const dim3 grid((unsigned)((w + TW - 1) / TW), (unsigned)((h + TH - 1) / TH)), block(256);
#define FM_BAYER_LAUNCH(BPS, METHOD)                                                                                          \
    hipLaunchKernelGGL((bayer_to_bgr_kernel<BPS, METHOD>), grid, block, 0, s, src, bgr, w, h, pattern, depth, black, (uint32_t)gain_r, \
                       (uint32_t)gain_g, (uint32_t)gain_b)
    if (bps == 1) {
        if (method == FM_BAYER_MHC) FM_BAYER_LAUNCH(1, FM_BAYER_MHC);
        else FM_BAYER_LAUNCH(1, FM_BAYER_BILINEAR);
    } else {
        if (method == FM_BAYER_MHC) FM_BAYER_LAUNCH(2, FM_BAYER_MHC);
        else FM_BAYER_LAUNCH(2, FM_BAYER_BILINEAR);
    }
#undef FM_BAYER_LAUNCH
    FM_HIP(hipGetLastError());
    return 0;
}
