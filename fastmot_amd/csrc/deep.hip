// 9- to 16-bit YCbCr -> packed BGR u8: the kernel behind fm_frame_upload_deep / fm_frame_upload_ahead_deep /
// fm_frame_ring_store_deep (frames.hip).  Two layouts of 16-bit little-endian words: planar (Y, U, V
// planes, the sample in the LOW bits: libavcodec's yuv420p10le, a Y4M C420p10 frame) and semi-planar (Y plane + a plane
// of interleaved U, V, the sample in the HIGH bits: P010 / P012 / P016, what a hardware HEVC / AV1 Main10 decoder
// delivers).
//
// Arithmetic (fastmot_amd/utils/deep.py states it in numpy, tests compare bit for bit), d the depth, s = d - 8:
//     y = max(Y - (16 << s), 0) * CY, u = U - (128 << s), v = V - (128 << s), h = 1 << (19 + s)
//     R = sat8((y + h + CVR v) >> (20 + s))   G = sat8((y + h + CVG v + CUG u) >> (20 + s))   B = sat8((y + h + CUB u) >> (20 + s))
// i.e. the 8-bit pixel with every sample kept at full precision: yuv_coef.h's 64-bit form (one v_mad_i64_i32 per term,
// one shift, and the 32-bit sat8).
//
// Shape: planar_to_bgr_kernel's (yuv.hip).  One thread owns 8 pixels of a row and, for 4:2:0, the same 8 columns of the
// row below it, so every chroma sample is loaded once: 16 (32) Y bytes and 2 x 8 chroma bytes (2 x 16 for 4:4:4; one
// 16-byte run of U, V pairs for semi-planar) in, 24 (48) BGR bytes out.  Threads are numbered along a row first: a
// wavefront reads 1024 contiguous Y bytes per row and writes 1536 contiguous BGR bytes per row.  Loads are bgr_run.h's
// load_run: a run is one 16-byte (8-byte) load when it is whole and its address aligned to it, narrower ones otherwise
// -- decided per thread from the address, so odd widths and planes that begin at odd sample offsets cost only the
// threads they touch.  Stores: StoreRule::ALIGNED8 when W % 8 == 0 and the frame is 8-byte aligned, StoreRule::BYTES
// otherwise.  Depth, the alignment shift and the mask are kernel arguments, the same for every
// lane.  A streaming kernel (6 bytes per pixel for 4:2:0): no LDS, no reuse beyond what a thread holds in registers.
#include "common.h"
#include "bgr_run.h"
#include "yuv_coef.h"

namespace {

// the n <= N samples of a run at p into w (sample i: word i >> 1, bits 16 * (i & 1)); N = 4: 8 bytes, N = 8: 16 bytes
template <int N>
__device__ __forceinline__ void load_run16(const uint16_t* __restrict__ p, int n, uint32_t (&w)[N / 2]) {
    load_run<N / 2>(reinterpret_cast<const uint8_t*>(p), 2 * n, n == N, w);
}

// SEMI: FM_DEEP_SEMIPLANAR (4:2:0 only; `up` is the UV plane).  CHROMA: FM_YUV_*.  ST8: W % 8 == 0 and an 8-byte aligned
// frame -- every thread's run is whole and its stores aligned.  Pitches in samples.  sample = (word >> rs) & mask.
template <bool SEMI, int CHROMA, bool ST8>
__global__ __launch_bounds__(256) void deep_to_bgr_kernel(const uint16_t* __restrict__ yp, const uint16_t* __restrict__ up,
                                                          const uint16_t* __restrict__ vp, uint8_t* __restrict__ bgr, int W, int H,
                                                          int pitch_y, int pitch_c, Nv12Coef c, int s, int rs, uint32_t mask) {
    constexpr bool PAIR = CHROMA == FM_YUV_420;                              // two rows share a chroma row
    constexpr int SH = (CHROMA == FM_YUV_420 || CHROMA == FM_YUV_422) ? 1 : 0;   // columns per chroma sample, log2
    constexpr int ROWS = PAIR ? 2 : 1;
    constexpr int NC = SEMI ? 8 : 8 >> SH;                                   // samples of a chroma run
    int by, x0, n;                                         // n: pixels of this thread's run
    if (!run_of(W, PAIR ? (H + 1) >> 1 : H, by, x0, n)) return;
    const int y0 = PAIR ? 2 * by : by;
    const int rows = min(ROWS, H - y0);

    uint32_t yw[ROWS][4], uw[NC / 2], vw[NC / 2];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
#pragma unroll
        for (int i = 0; i < 4; ++i) yw[r][i] = 0;
        if (r < rows) load_run16<8>(yp + (size_t)(y0 + r) * pitch_y + x0, n, yw[r]);
    }
#pragma unroll
    for (int i = 0; i < NC / 2; ++i) uw[i] = vw[i] = 0;
    if (CHROMA != FM_YUV_MONO) {
        const int nc = (n + SH) >> SH;                     // chroma samples (semi-planar: U, V pairs) under the run
        if (SEMI) {
            load_run16<NC>(up + (size_t)by * pitch_c + x0, 2 * nc, uw);      // (W is even: the run holds whole pairs)
        } else {
            const size_t at = (size_t)by * pitch_c + (x0 >> SH);
            load_run16<NC>(up + at, nc, uw);
            load_run16<NC>(vp + at, nc, vw);
        }
    }

    uint32_t o[ROWS][6] = {};
    const int yoff = 16 << s, coff = 128 << s;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int u = 0, v = 0;
        if (CHROMA != FM_YUV_MONO) {
            const uint32_t U = SEMI ? run_word16(uw, 2 * (i >> 1)) : run_word16(uw, i >> SH);
            const uint32_t V = SEMI ? run_word16(uw, 2 * (i >> 1) + 1) : run_word16(vw, i >> SH);
            u = (int)((U >> rs) & mask) - coff;
            v = (int)((V >> rs) & mask) - coff;
        }
        long long cb, cg, cr;
        ycc_chroma(c, u, v, s, cb, cg, cr);
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            uint32_t b, g, d;
            ycc_px(c, (int)((run_word16(yw[r], i) >> rs) & mask), yoff, s, cb, cg, cr, b, g, d);
            put_px(o[r], i, b, g, d);
        }
    }

#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        if (r >= rows) break;
        store_run<ST8 ? StoreRule::ALIGNED8 : StoreRule::BYTES>(bgr + ((size_t)(y0 + r) * W + x0) * 3, n, o[r]);
    }
}

struct DeepArgs {
    const uint16_t *y, *u, *v;
    uint8_t* bgr;
    int w, h, py, pc, s, rs;
    uint32_t mask;
    Nv12Coef c;
    dim3 grid;
    hipStream_t stream;
};

template <bool SEMI, int CHROMA>
void launch_deep(const DeepArgs& a) {
    if (a.w % 8 == 0 && !((uintptr_t)a.bgr & 7))
        hipLaunchKernelGGL((deep_to_bgr_kernel<SEMI, CHROMA, true>), a.grid, dim3(256), 0, a.stream, a.y, a.u, a.v, a.bgr, a.w, a.h, a.py,
                           a.pc, a.c, a.s, a.rs, a.mask);
    else
        hipLaunchKernelGGL((deep_to_bgr_kernel<SEMI, CHROMA, false>), a.grid, dim3(256), 0, a.stream, a.y, a.u, a.v, a.bgr, a.w, a.h, a.py,
                           a.pc, a.c, a.s, a.rs, a.mask);
}

}  // namespace

// Converts the packed deep frame at `planes` (2-byte aligned; Y: w * h words, then for FM_DEEP_PLANAR U and V: cw * ch
// words each, cw x ch the chroma planes' size for `chroma`, none for FM_YUV_MONO; for FM_DEEP_SEMIPLANAR h / 2 rows of w
// interleaved U, V words) to w * h * 3 BGR bytes at `bgr`, on stream `s`.  The callers have checked the arguments.
int fm_deep_to_bgr(const uint8_t* planes, uint8_t* bgr, int w, int h, int chroma, int matrix, int depth, int layout, hipStream_t s) {
    FM_CHECK_ARG(planes && bgr && !((uintptr_t)planes & 1) && w >= 1 && h >= 1 && w <= FM_SRC_MAX_DIM && h <= FM_SRC_MAX_DIM);
    FM_CHECK_ARG(fm_deep_layout_ok(w, h, chroma, matrix, depth, layout));
    int cw = 0, ch = 0;
    fm_yuv_chroma_dims(w, h, chroma, &cw, &ch);
    const bool semi = layout == FM_DEEP_SEMIPLANAR;
    DeepArgs a;
    a.y = reinterpret_cast<const uint16_t*>(planes);
    a.u = a.y + (size_t)w * h;
    a.v = semi ? nullptr : a.u + (size_t)cw * ch;
    a.bgr = bgr;
    a.w = w, a.h = h, a.py = w, a.pc = semi ? w : cw;
    a.s = depth - 8;
    a.rs = semi ? 16 - depth : 0;
    a.mask = (1u << depth) - 1;
    a.c = DEEP_COEF[matrix];
    const long long threads = (long long)((w + 7) >> 3) * (chroma == FM_YUV_420 ? (h + 1) >> 1 : h);
    a.grid = dim3((unsigned)((threads + 255) / 256));
    a.stream = s;
    if (semi) {
        launch_deep<true, FM_YUV_420>(a);
    } else {
        switch (chroma) {
        case FM_YUV_420: launch_deep<false, FM_YUV_420>(a); break;
        case FM_YUV_422: launch_deep<false, FM_YUV_422>(a); break;
        case FM_YUV_444: launch_deep<false, FM_YUV_444>(a); break;
        default: launch_deep<false, FM_YUV_MONO>(a); break;
        }
    }
    FM_HIP(hipGetLastError());
    return 0;
}
