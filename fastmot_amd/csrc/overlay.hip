// Overlays on the device frame (fastmot_hip.h "Overlays ON the device frame"): a command list in painter's
// order is applied to a COPY of the current frame, the context's overlay buffer.  The tracker's frame is only read.
//
// One launch.  A workgroup of 256 threads owns a tile of 64 x 16 pixels, a thread four neighbouring pixels of one row,
// which it holds in registers from its only read of the frame to its only write of the overlay buffer.  The list is
// walked 256 commands at a time: thread i tests the bounding box of command base + i against the tile, a ballot and a
// population count per wavefront plus the four wavefront totals give every hit its place IN LIST ORDER in LDS, and then
// every thread applies the hits, in that order, to its four pixels with the functions of overlay_pixel.h -- the text
// fm_overlay_render_host runs on the CPU.  A tile nothing hits is a copy.
//
// Rows are 3 * width bytes without padding, so a thread's 12 bytes are dword-aligned only where the row's start is
// (always when the width is a multiple of four and the frame's base is aligned; one row in four otherwise): aligned
// full quads move as three dwords, everything else -- and the last columns of a frame -- as bytes.
//
// Bounds: a thread touches pixels (x .. x + 3, y) with x < width and y < height only; the list has passed
// fm_overlay_check, so a mask's bytes lie inside the blob whatever the pixel.
#include "common.h"
#include "overlay_pixel.h"

namespace {

constexpr int TILE_W = 64, TILE_H = 16, WG = 256, QUAD = 4;
static_assert(sizeof(fm_overlay_cmd) == 32, "fm_overlay_cmd is two 16-byte words");
static_assert((TILE_W / QUAD) * TILE_H == WG, "one quad per thread");

__global__ __launch_bounds__(WG) void overlay_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int W, int H,
                                                     const fm_overlay_cmd* __restrict__ cmds, int n, const uint8_t* __restrict__ masks) {
    __shared__ uint4 hits[2 * WG];
    __shared__ int wave_hits[WG / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx0 = blockIdx.x * TILE_W, ty0 = blockIdx.y * TILE_H;
    const int x = tx0 + (tid & 15) * QUAD, y = ty0 + (tid >> 4);
    const int npx = y < H ? min(max(W - x, 0), QUAD) : 0;
    const size_t at = ((size_t)y * W + x) * 3;

    unsigned px[QUAD][3];
    const bool wide_in = npx == QUAD && ((uintptr_t)(src + at) & 3) == 0;
    if (wide_in) {
        const uint32_t* const s = reinterpret_cast<const uint32_t*>(src + at);
        const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];
        px[0][0] = w0 & 255, px[0][1] = (w0 >> 8) & 255, px[0][2] = (w0 >> 16) & 255;
        px[1][0] = w0 >> 24, px[1][1] = w1 & 255, px[1][2] = (w1 >> 8) & 255;
        px[2][0] = (w1 >> 16) & 255, px[2][1] = w1 >> 24, px[2][2] = w2 & 255;
        px[3][0] = (w2 >> 8) & 255, px[3][1] = (w2 >> 16) & 255, px[3][2] = w2 >> 24;
    } else {
#pragma unroll
        for (int k = 0; k < QUAD; ++k)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) px[k][ch] = k < npx ? src[at + k * 3 + ch] : 0;
    }

    for (int base = 0; base < n; base += WG) {
        const int idx = base + tid;
        uint4 q0 = {0, 0, 0, 0}, q1 = {0, 0, 0, 0};
        bool hit = false;
        if (idx < n) {
            const uint4* const q = reinterpret_cast<const uint4*>(cmds + idx);
            q0 = q[0], q1 = q[1];
            fm_overlay_cmd c;
            __builtin_memcpy(&c, &q0, 16);
            __builtin_memcpy(reinterpret_cast<char*>(&c) + 16, &q1, 16);
            const FmOvlBox bb = fm_ovl_bbox(c);
            hit = bb.x0 <= bb.x1 && bb.y0 <= bb.y1 && bb.x1 >= tx0 && bb.x0 < tx0 + TILE_W && bb.y1 >= ty0 && bb.y0 < ty0 + TILE_H;
        }
        const unsigned long long ballot = __ballot(hit);
        if (lane == 0) wave_hits[wave] = __popcll(ballot);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int wv = 0; wv < WG / 64; ++wv) {
            const int cnt = wave_hits[wv];
            before += wv < wave ? cnt : 0;
            total += cnt;
        }
        if (hit) {
            const int slot = before + __popcll(ballot & ((1ull << lane) - 1ull));
            hits[2 * slot] = q0, hits[2 * slot + 1] = q1;
        }
        __syncthreads();
        if (npx > 0) {
            for (int h = 0; h < total; ++h) {
                const uint4 a = hits[2 * h], b = hits[2 * h + 1];
                fm_overlay_cmd c;
                __builtin_memcpy(&c, &a, 16);
                __builtin_memcpy(reinterpret_cast<char*>(&c) + 16, &b, 16);
#pragma unroll
                for (int k = 0; k < QUAD; ++k)
                    if (k < npx) fm_ovl_apply(c, masks, x + k, y, px[k][0], px[k][1], px[k][2]);
            }
        }
        __syncthreads();       // hits and wave_hits are written again by the next chunk
    }

    if (npx == QUAD && ((uintptr_t)(dst + at) & 3) == 0) {
        uint32_t* const d = reinterpret_cast<uint32_t*>(dst + at);
        d[0] = px[0][0] | px[0][1] << 8 | px[0][2] << 16 | px[1][0] << 24;
        d[1] = px[1][1] | px[1][2] << 8 | px[2][0] << 16 | px[2][1] << 24;
        d[2] = px[2][2] | px[3][0] << 8 | px[3][1] << 16 | px[3][2] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < QUAD; ++k)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                if (k < npx) dst[at + k * 3 + ch] = (uint8_t)px[k][ch];
    }
}

}  // namespace

struct OvlState {
    uint8_t* buf = nullptr;      // the overlay buffer: width * height * 3 bytes
    size_t buf_cap = 0;
    int w = 0, h = 0;            // the frame size of the last render (0: none yet)
    DevBuf cmds, masks;          // device copies with their page-locked staging
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;
    bool timed = false;
};

void fm_overlay_free(fm_ctx* ctx) {
    OvlState* o = ctx->ovl;
    if (!o) return;
    if (hipStream_t s = fm_jpegenc_stream(ctx)) (void)hipStreamSynchronize(s);
    if (o->buf) (void)hipFree(o->buf);
    o->cmds.release();
    o->masks.release();
    if (o->ev_t0) (void)hipEventDestroy(o->ev_t0);
    if (o->ev_t1) (void)hipEventDestroy(o->ev_t1);
    delete o;
    ctx->ovl = nullptr;
}

extern "C" int fm_frame_render_overlay(fm_ctx* ctx, const fm_overlay_cmd* cmds, int n, const uint8_t* masks, size_t mask_bytes) {
    FM_CHECK_ARG(ctx && ctx->frame_cur && ctx->frame_w >= 1 && ctx->frame_h >= 1);
    const int W = ctx->frame_w, H = ctx->frame_h;
    if (int rc = fm_overlay_check(cmds, n, masks, mask_bytes, W, H)) return rc;
    if (int rc = fm_jpegenc_ensure(ctx, 0, 0)) return rc;          // the encoder's stream, created on first use
    hipStream_t s = fm_jpegenc_stream(ctx);
    if (!ctx->ovl) {
        OvlState* o = new OvlState;
        hipError_t err = hipEventCreate(&o->ev_t0);
        if (err == hipSuccess) err = hipEventCreate(&o->ev_t1);
        if (err != hipSuccess) {
            if (o->ev_t0) (void)hipEventDestroy(o->ev_t0);
            delete o;
            fm_set_error("overlay: creating the events failed -> %s", hipGetErrorString(err));
            return FM_ERR_HIP;
        }
        ctx->ovl = o;
    }
    OvlState* o = ctx->ovl;
    // Nothing of an earlier render may be in flight when the staging below is rewritten.  A render that succeeded
    // returned behind the synchronise at its end; one that failed half way may have left a copy enqueued.
    FM_HIP(hipStreamSynchronize(s));
    const size_t bytes = (size_t)W * H * 3;
    if (bytes > o->buf_cap) {
        if (o->buf) (void)hipFree(o->buf);
        o->buf = nullptr, o->buf_cap = 0;
        FM_HIP(hipMalloc(&o->buf, bytes));
        o->buf_cap = bytes;
    }
    o->w = o->h = 0;                                                // no picture until this render is complete
    const size_t cmd_bytes = (size_t)n * sizeof(fm_overlay_cmd);
    if (n > 0) {
        if (int rc = o->cmds.reserve(cmd_bytes)) return rc;
        memcpy(o->cmds.h, cmds, cmd_bytes);
        FM_HIP(hipMemcpyAsync(o->cmds.d, o->cmds.h, cmd_bytes, hipMemcpyHostToDevice, s));
    }
    if (mask_bytes > 0) {
        if (int rc = o->masks.reserve(mask_bytes)) return rc;
        memcpy(o->masks.h, masks, mask_bytes);
        FM_HIP(hipMemcpyAsync(o->masks.d, o->masks.h, mask_bytes, hipMemcpyHostToDevice, s));
    }
    // The current frame is complete on the device: the argument of fm_frame_encode_jpeg (jpegenc.hip), unchanged.
    FM_HIP(hipEventRecord(o->ev_t0, s));
    hipLaunchKernelGGL(overlay_kernel, dim3((W + TILE_W - 1) / TILE_W, (H + TILE_H - 1) / TILE_H), dim3(WG), 0, s, ctx->frame_cur, o->buf, W,
                       H, o->cmds.dev<fm_overlay_cmd>(), n, o->masks.dev<uint8_t>());
    FM_HIP(hipGetLastError());
    FM_HIP(hipEventRecord(o->ev_t1, s));
    FM_HIP(hipStreamSynchronize(s));
    o->timed = true;
    o->w = W, o->h = H;
    return 0;
}

extern "C" int fm_overlay_read(fm_ctx* ctx, uint8_t* out) {
    FM_CHECK_ARG(ctx && out && ctx->ovl && ctx->ovl->w == ctx->frame_w && ctx->ovl->h == ctx->frame_h && ctx->ovl->w > 0);
    hipStream_t s = fm_jpegenc_stream(ctx);
    FM_HIP(hipMemcpyAsync(out, ctx->ovl->buf, (size_t)ctx->ovl->w * ctx->ovl->h * 3, hipMemcpyDeviceToHost, s));
    FM_HIP(hipStreamSynchronize(s));
    return 0;
}

// For yuv.hip (fm_frame_export_i420): the picture fm_overlay_read would download, or null when there is none
const uint8_t* fm_overlay_buffer(fm_ctx* ctx) {
    const OvlState* o = ctx->ovl;
    return o && o->w > 0 && o->w == ctx->frame_w && o->h == ctx->frame_h ? o->buf : nullptr;
}

extern "C" int fm_overlay_encode_jpeg(fm_ctx* ctx, int quality, uint8_t* out, size_t capacity, size_t* length) {
    FM_CHECK_ARG(ctx && out && length && ctx->ovl && ctx->ovl->w == ctx->frame_w && ctx->ovl->h == ctx->frame_h && ctx->ovl->w > 0);
    return fm_jpegenc_encode_device(ctx, ctx->ovl->buf, ctx->ovl->w, ctx->ovl->h, quality, out, capacity, length);
}

extern "C" int fm_overlay_stream_ms(fm_ctx* ctx, float* ms) {
    FM_CHECK_ARG(ctx && ms);
    *ms = -1.f;
    if (ctx->ovl && ctx->ovl->timed) FM_HIP(hipEventElapsedTime(ms, ctx->ovl->ev_t0, ctx->ovl->ev_t1));
    return 0;
}
