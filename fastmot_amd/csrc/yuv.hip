// Planar YCbCr <-> packed BGR u8: the kernels behind fm_frame_upload_planar / fm_frame_upload_ahead_planar /
// fm_frame_ring_store_planar (frames.hip) and the exports fm_frame_export_i420 / fm_i420_from_bgr (below).
// Planar I420 is what software decoders hand out and what a YUV4MPEG2 (.y4m) file holds: a Y plane W x H, then a U and a
// V plane of ceil(W / 2) x ceil(H / 2) (4:2:0), ceil(W / 2) x H (4:2:2) or W x H (4:4:4) samples, or no chroma at all.
//
// In: yuv_coef.h's limited-range arithmetic per pixel (fastmot_amd/utils/yuv.py states both directions in numpy, tests
// compare bit for bit), pixel (r, c) using chroma sample (r >> sv, c >> sh).  One thread owns 8 pixels of a row and, for 4:2:0,
// the same 8 columns of the row below it, so every chroma sample is loaded once: 8 (16) Y bytes and 2 x 4 (2 x 8 for
// 4:4:4) chroma bytes in, 24 (48) BGR bytes out.  Threads are numbered along a row first: a wavefront reads 512 contiguous
// Y bytes per row and writes 1536 contiguous BGR bytes per row.  Loads are bgr_run.h's load_run: one 8-byte (4-byte for four
// chroma samples) access when the thread's run is whole and its address aligned, narrower ones otherwise -- decided per
// thread from the address, so odd widths, odd pitches and planes that begin at odd offsets (the U plane of an odd-sized
// frame) cost only the threads they touch.  Stores: StoreRule::ALIGNED8 when W % 8 == 0 and the frame is 8-byte
// aligned, StoreRule::BYTES otherwise.
//
// Out: BGR -> I420 with the 8-bit BT.601 integer form of utils.nv12.bgr_to_nv12,
//     Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16, U = ((-38 R - 74 G + 112 B + 128) >> 8) + 128,
//     V = ((112 R - 94 G - 18 B + 128) >> 8) + 128, chroma sample = (sum of the 2 x 2 block's four U (V) + 2) >> 2,
// the column / row an odd size lacks being the last one repeated (clamped indices).  One thread owns a 2-row strip of 8
// columns: 2 x 24 BGR bytes in, 16 Y + 4 U + 4 V bytes out.
//
// Both are streaming kernels (4.5 bytes per pixel for 4:2:0): no LDS, no reuse beyond what a thread holds in registers.
#include "common.h"
#include "bgr_run.h"
#include "yuv_coef.h"

const uint8_t* fm_overlay_buffer(fm_ctx* ctx);            // overlay.hip: the overlay picture of the current frame size, or null

namespace {

// CHROMA: FM_YUV_*.  ST8: W % 8 == 0 and an 8-byte aligned frame -- every thread's run is whole and its stores aligned.
template <int CHROMA, bool ST8>
__global__ __launch_bounds__(256) void planar_to_bgr_kernel(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ up,
                                                            const uint8_t* __restrict__ vp, uint8_t* __restrict__ bgr, int W, int H,
                                                            int pitch_y, int pitch_c, Nv12Coef c) {
    constexpr bool PAIR = CHROMA == FM_YUV_420;                              // two rows share a chroma row
    constexpr int SH = (CHROMA == FM_YUV_420 || CHROMA == FM_YUV_422) ? 1 : 0;   // columns per chroma sample, log2
    constexpr int ROWS = PAIR ? 2 : 1;
    constexpr int NCW = 2 >> SH;                                             // words of a chroma run: 8 or 4 samples
    int by, x0, n;                                         // n: pixels of this thread's run
    if (!run_of(W, PAIR ? (H + 1) >> 1 : H, by, x0, n)) return;
    const int y0 = PAIR ? 2 * by : by;
    const int rows = min(ROWS, H - y0);

    uint32_t yw[ROWS][2], uw[NCW] = {}, vw[NCW] = {};
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        yw[r][0] = yw[r][1] = 0;
        if (r < rows) load_run<2>(yp + (size_t)(y0 + r) * pitch_y + x0, n, n == 8, yw[r]);
    }
    if (CHROMA != FM_YUV_MONO) {
        const size_t at = (size_t)by * pitch_c + (x0 >> SH);
        const int nc = (n + SH) >> SH;                     // chroma samples under the run
        load_run<NCW>(up + at, nc, nc == 4 * NCW, uw);
        load_run<NCW>(vp + at, nc, nc == 4 * NCW, vw);
    }

    uint32_t o[ROWS][6] = {};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int u = CHROMA == FM_YUV_MONO ? 0 : (int)run_byte(uw, i >> SH) - 128;
        const int v = CHROMA == FM_YUV_MONO ? 0 : (int)run_byte(vw, i >> SH) - 128;
        int cb, cg, cr;
        ycc_chroma(c, u, v, cb, cg, cr);
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            uint32_t b, g, d;
            ycc_px(c, (int)run_byte(yw[r], i), 16, cb, cg, cr, b, g, d);
            put_px(o[r], i, b, g, d);
        }
    }

#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        if (r >= rows) break;
        store_run<ST8 ? StoreRule::ALIGNED8 : StoreRule::BYTES>(bgr + ((size_t)(y0 + r) * W + x0) * 3, n, o[r]);
    }
}

__global__ __launch_bounds__(256) void bgr_to_i420_kernel(const uint8_t* __restrict__ bgr, long long pitch, uint8_t* __restrict__ yo,
                                                          uint8_t* __restrict__ uo, uint8_t* __restrict__ vo, int W, int H) {
    const int CW = (W + 1) >> 1;
    int by, x0, n;
    if (!run_of(W, (H + 1) >> 1, by, x0, n)) return;
    const int y0 = 2 * by;

    int us[4] = {0, 0, 0, 0}, vs[4] = {0, 0, 0, 0};
    uint32_t yw[2][2] = {};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint8_t* const row = bgr + (size_t)min(y0 + r, H - 1) * pitch + (size_t)x0 * 3;       // (the row below the last: that row again)
        uint32_t w[6] = {};
        if (n == 8 && !((uintptr_t)row & 7)) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint2 a = reinterpret_cast<const uint2*>(row)[q];
                w[2 * q] = a.x, w[2 * q + 1] = a.y;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 24; ++k)                   // (a column right of the last: that column again)
                put_byte(w, k, row[min(k / 3, n - 1) * 3 + k % 3]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int B = (int)run_byte(w, 3 * i), G = (int)run_byte(w, 3 * i + 1), R = (int)run_byte(w, 3 * i + 2);
            const uint32_t Y = (uint32_t)(((66 * R + 129 * G + 25 * B + 128) >> 8) + 16);
            put_byte(yw[r], i, Y);
            us[i >> 1] += ((-38 * R - 74 * G + 112 * B + 128) >> 8) + 128;
            vs[i >> 1] += ((112 * R - 94 * G - 18 * B + 128) >> 8) + 128;
        }
    }

#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (y0 + r >= H) break;
        uint8_t* const out = yo + (size_t)(y0 + r) * W + x0;
        if (n == 8 && !((uintptr_t)out & 7)) {
            *reinterpret_cast<uint2*>(out) = make_uint2(yw[r][0], yw[r][1]);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (i < n) out[i] = (uint8_t)(yw[r][i >> 2] >> ((i & 3) * 8));
        }
    }
    uint32_t u4 = 0, v4 = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        u4 |= (uint32_t)((us[p] + 2) >> 2) << (p * 8);
        v4 |= (uint32_t)((vs[p] + 2) >> 2) << (p * 8);
    }
    const size_t at = (size_t)by * CW + (x0 >> 1);
    const int nc = (n + 1) >> 1;
    if (nc == 4 && !((uintptr_t)(uo + at) & 3) && !((uintptr_t)(vo + at) & 3)) {
        *reinterpret_cast<uint32_t*>(uo + at) = u4;
        *reinterpret_cast<uint32_t*>(vo + at) = v4;
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (p < nc) uo[at + p] = (uint8_t)(u4 >> (p * 8)), vo[at + p] = (uint8_t)(v4 >> (p * 8));
    }
}

template <int CHROMA>
void launch_planar(const uint8_t* y, const uint8_t* u, const uint8_t* v, uint8_t* bgr, int w, int h, int py, int pc, const Nv12Coef& c,
                   dim3 grid, hipStream_t s) {
    if (w % 8 == 0 && !((uintptr_t)bgr & 7))
        hipLaunchKernelGGL((planar_to_bgr_kernel<CHROMA, true>), grid, dim3(256), 0, s, y, u, v, bgr, w, h, py, pc, c);
    else
        hipLaunchKernelGGL((planar_to_bgr_kernel<CHROMA, false>), grid, dim3(256), 0, s, y, u, v, bgr, w, h, py, pc, c);
}

bool size_ok(int w, int h) { return w >= 1 && h >= 1 && w <= FM_SRC_MAX_DIM && h <= FM_SRC_MAX_DIM; }

// BGR in device memory (`pitch` bytes between rows), which work already enqueued on `s` completes -> I420 at `dst`
int launch_i420(const uint8_t* src, long long pitch, int w, int h, uint8_t* dst, hipStream_t s) {
    const size_t npx = (size_t)w * h, nc = (size_t)((w + 1) >> 1) * ((h + 1) >> 1);
    const long long threads = (long long)((w + 7) >> 3) * ((h + 1) >> 1);
    hipLaunchKernelGGL(bgr_to_i420_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, src, pitch, dst, dst + npx,
                       dst + npx + nc, w, h);
    FM_HIP(hipGetLastError());
    return 0;
}

}  // namespace

// The I420 export's buffers: the planes on the device and in page-locked memory, and the staging of fm_i420_from_bgr's pixels
struct YuvState {
    uint8_t *dev = nullptr, *host = nullptr;
    size_t cap = 0;
    uint8_t *stage = nullptr, *stage_host = nullptr;
    size_t stage_cap = 0;
};

void fm_yuv_free(fm_ctx* ctx) {
    YuvState* y = ctx->yuv;
    if (!y) return;
    if (hipStream_t s = fm_jpegenc_stream(ctx)) (void)hipStreamSynchronize(s);
    for (uint8_t* p : {y->dev, y->stage})
        if (p) (void)hipFree(p);
    for (uint8_t* p : {y->host, y->stage_host})
        if (p) (void)hipHostFree(p);
    delete y;
    ctx->yuv = nullptr;
}

// Converts the packed planar frame at `planes` (Y: w * h bytes, then U and V: cw * ch bytes each, cw x ch the chroma
// planes' size for `chroma`; none for FM_YUV_MONO) to w * h * 3 BGR bytes at `bgr`, on stream `s`.  The callers have
// checked the arguments.
int fm_planar_to_bgr(const uint8_t* planes, uint8_t* bgr, int w, int h, int chroma, int matrix, hipStream_t s) {
    FM_CHECK_ARG(planes && bgr && size_ok(w, h) && (matrix == FM_NV12_BT601 || matrix == FM_NV12_BT709));
    int cw = 0, ch = 0;
    FM_CHECK_ARG(fm_yuv_chroma_dims(w, h, chroma, &cw, &ch));
    const uint8_t* const u = planes + (size_t)w * h;
    const uint8_t* const v = u + (size_t)cw * ch;
    const long long threads = (long long)((w + 7) >> 3) * (chroma == FM_YUV_420 ? (h + 1) >> 1 : h);
    const dim3 grid((unsigned)((threads + 255) / 256));
    const Nv12Coef& c = NV12_COEF[matrix];
    switch (chroma) {
    case FM_YUV_420: launch_planar<FM_YUV_420>(planes, u, v, bgr, w, h, w, cw, c, grid, s); break;
    case FM_YUV_422: launch_planar<FM_YUV_422>(planes, u, v, bgr, w, h, w, cw, c, grid, s); break;
    case FM_YUV_444: launch_planar<FM_YUV_444>(planes, u, v, bgr, w, h, w, cw, c, grid, s); break;
    default: launch_planar<FM_YUV_MONO>(planes, u, v, bgr, w, h, w, cw, c, grid, s); break;
    }
    FM_HIP(hipGetLastError());
    return 0;
}

extern "C" size_t fm_i420_bound(int width, int height) {
    if (!size_ok(width, height)) return 0;
    return (size_t)width * height + 2 * (size_t)((width + 1) / 2) * ((height + 1) / 2);
}

// Shared tail of the two exports: `src` (device memory, ordered by the encoder's stream) -> out[0, need)
static int export_i420(fm_ctx* ctx, const uint8_t* src, long long pitch, int w, int h, uint8_t* out, size_t need) {
    YuvState* y = ctx->yuv;
    hipStream_t s = fm_jpegenc_stream(ctx);
    if (need > y->cap) {                                   // (nothing of an earlier export is in flight: it returned synchronised)
        if (y->dev) (void)hipFree(y->dev);
        if (y->host) (void)hipHostFree(y->host);
        y->dev = y->host = nullptr, y->cap = 0;
        FM_HIP(hipMalloc(&y->dev, need));
        FM_HIP(hipHostMalloc(&y->host, need, hipHostMallocDefault));
        y->cap = need;
    }
    if (int rc = launch_i420(src, pitch, w, h, y->dev, s)) return rc;
    uint8_t* const to = fm_host_is_pinned(out, need) ? out : y->host;
    FM_HIP(hipMemcpyAsync(to, y->dev, need, hipMemcpyDeviceToHost, s));
    FM_HIP(hipStreamSynchronize(s));
    if (to != out) memcpy(out, to, need);
    return 0;
}

static int yuv_ensure(fm_ctx* ctx) {
    if (int rc = fm_jpegenc_ensure(ctx, 0, 0)) return rc;          // the encoder's stream, created on first use
    if (!ctx->yuv) ctx->yuv = new YuvState;
    return 0;
}

extern "C" int fm_frame_export_i420(fm_ctx* ctx, int which, uint8_t* out, size_t capacity, size_t* length) {
    FM_CHECK_ARG(ctx && out && length && (which == FM_EXPORT_FRAME || which == FM_EXPORT_OVERLAY) && ctx->frame_cur &&
                 size_ok(ctx->frame_w, ctx->frame_h));
    const uint8_t* const src = which == FM_EXPORT_FRAME ? ctx->frame_cur : fm_overlay_buffer(ctx);
    if (!src) {
        fm_set_error("I420 export: no overlay picture of the current frame size (fm_frame_render_overlay comes first)");
        return FM_ERR_ARG;
    }
    const size_t need = fm_i420_bound(ctx->frame_w, ctx->frame_h);
    *length = need;
    if (capacity < need) {
        fm_set_error("I420 export: capacity %zu < the %zu bytes of a %dx%d frame", capacity, need, ctx->frame_w, ctx->frame_h);
        return FM_ERR_ARG;
    }
    if (int rc = yuv_ensure(ctx)) return rc;
    // No event of the pipeline is waited for: fm_frame_encode_jpeg's argument (jpegenc.hip) for why the current frame is
    // complete on the device holds unchanged, and the overlay buffer was rendered on this very stream.
    return export_i420(ctx, src, (long long)ctx->frame_w * 3, ctx->frame_w, ctx->frame_h, out, need);
}

extern "C" int fm_i420_from_bgr(fm_ctx* ctx, const uint8_t* pixels, int width, int height, size_t pitch, uint8_t* out, size_t capacity,
                                size_t* length) {
    FM_CHECK_ARG(ctx && pixels && out && length && size_ok(width, height) && pitch >= (size_t)width * 3);
    const size_t need = fm_i420_bound(width, height);
    *length = need;
    if (capacity < need) {
        fm_set_error("I420 export: capacity %zu < the %zu bytes of a %dx%d frame", capacity, need, width, height);
        return FM_ERR_ARG;
    }
    if (int rc = yuv_ensure(ctx)) return rc;
    YuvState* y = ctx->yuv;
    hipStream_t s = fm_jpegenc_stream(ctx);
    const size_t row = (size_t)width * 3, bytes = row * height;
    if (bytes > y->stage_cap) {
        if (y->stage) (void)hipFree(y->stage);
        if (y->stage_host) (void)hipHostFree(y->stage_host);
        y->stage = y->stage_host = nullptr, y->stage_cap = 0;
        FM_HIP(hipMalloc(&y->stage, bytes));
        FM_HIP(hipHostMalloc(&y->stage_host, bytes, hipHostMallocDefault));
        y->stage_cap = bytes;
    }
    const uint8_t* from = pixels;
    if (pitch != row || !fm_host_is_pinned(pixels, bytes)) {      // (the previous call's copy out of stage_host is complete: it returned)
        if (pitch == row)
            memcpy(y->stage_host, pixels, bytes);
        else
            for (int r = 0; r < height; ++r) memcpy(y->stage_host + (size_t)r * row, pixels + (size_t)r * pitch, row);
        from = y->stage_host;
    }
    FM_HIP(hipMemcpyAsync(y->stage, from, bytes, hipMemcpyHostToDevice, s));
    return export_i420(ctx, y->stage, (long long)row, width, height, out, need);
}
