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
// fm_frame_render_redacted (fastmot_hip.h "Redaction of the frames that leave the GPU") runs the second
// instantiation of the kernel, which between the read and the command list replaces each pixel by the value of the last
// redaction region that covers it (redact_pixel.h; the cell means come from redact.hip, launched in front).  The
// instantiation fm_frame_render_overlay launches has no such stage and is the kernel as it was.
//
// Rows are 3 * width bytes without padding, so a thread's 12 bytes are dword-aligned only where the row's start is
// (always when the width is a multiple of four and the frame's base is aligned; one row in four otherwise): aligned
// full quads move as three dwords, everything else -- and the last columns of a frame -- as bytes.
//
// Bounds: a thread touches pixels (x .. x + 3, y) with x < width and y < height only; the list has passed
// fm_overlay_check, so a mask's bytes lie inside the blob whatever the pixel.  A region's means are read only for pixels
// inside its rectangle clipped to the frame, i.e. of cells in imin..imax x jmin..jmax (neighbours clamped into that range),
// which are the words the host counted for it from the same fm_red_grid; indices up to 8191 travel as 16 bits.
#include "common.h"
#include "overlay_pixel.h"
#include "redact_pixel.h"

namespace {

constexpr int TILE_W = 64, TILE_H = 16, WG = 256, QUAD = 4;
static_assert(sizeof(fm_overlay_cmd) == 32, "fm_overlay_cmd is two 16-byte words");
static_assert((TILE_W / QUAD) * TILE_H == WG, "one quad per thread");

template <bool REDACT>
__global__ __launch_bounds__(WG) void overlay_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int W, int H,
                                                     const fm_overlay_cmd* __restrict__ cmds, int n, const uint8_t* __restrict__ masks,
                                                     const fm_redact_region* __restrict__ regions, int nr, const int2* __restrict__ tab,
                                                     const uint32_t* __restrict__ means) {
    __shared__ uint4 hits[(REDACT ? 3 : 2) * WG];
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

    // Redaction (fastmot_hip.h "Redaction of the frames that leave the GPU"): the regions are binned as the commands are
    // below, each hit with its clipped rectangle's cell range and the offset of its means; a pixel takes the value of
    // the LAST region that covers it -- the hits of a chunk are walked backwards until every pixel of the quad is
    // settled, and a later chunk overrides an earlier one.  The values come from the means alone, i.e. from src.
    if constexpr (REDACT) {
        for (int base = 0; base < nr; base += WG) {
            const int idx = base + tid;
            uint4 q0 = {0, 0, 0, 0}, q1 = {0, 0, 0, 0}, q2 = {0, 0, 0, 0};
            bool hit = false;
            if (idx < nr) {
                const uint4* const q = reinterpret_cast<const uint4*>(regions + idx);
                q0 = q[0], q1 = q[1];
                fm_redact_region r;
                __builtin_memcpy(&r, &q0, 16);
                __builtin_memcpy(reinterpret_cast<char*>(&r) + 16, &q1, 16);
                const FmRedGrid g = fm_red_grid(r, W, H);
                hit = g.cx0 <= g.cx1 && g.cy0 <= g.cy1 && g.cx1 >= tx0 && g.cx0 < tx0 + TILE_W && g.cy1 >= ty0 && g.cy0 < ty0 + TILE_H;
                q2 = {(unsigned)g.imin | (unsigned)g.imax << 16, (unsigned)g.jmin | (unsigned)g.jmax << 16, (unsigned)tab[idx].x, 0u};
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
                hits[3 * slot] = q0, hits[3 * slot + 1] = q1, hits[3 * slot + 2] = q2;
            }
            __syncthreads();
            unsigned todo = (1u << npx) - 1u;
            for (int h = total - 1; h >= 0 && todo; --h) {
                const uint4 a = hits[3 * h], b = hits[3 * h + 1], e = hits[3 * h + 2];
                fm_redact_region r;
                __builtin_memcpy(&r, &a, 16);
                __builtin_memcpy(reinterpret_cast<char*>(&r) + 16, &b, 16);
                if (y < r.y0 || y > r.y1 || x + QUAD - 1 < r.x0 || x > r.x1) continue;
                FmRedGrid g;
                g.cx0 = g.cy0 = 0, g.cx1 = W - 1, g.cy1 = H - 1;       // (fm_red_value reads the index ranges only)
                g.imin = e.x & 0xffff, g.imax = e.x >> 16, g.jmin = e.y & 0xffff, g.jmax = e.y >> 16;
                const uint32_t* const m = means + e.z;
#pragma unroll
                for (int k = 0; k < QUAD; ++k)
                    if ((todo >> k & 1u) && fm_red_covers(r, x + k, y)) {
                        const uint32_t v = fm_red_value(r, g, m, x + k, y);
                        px[k][0] = v & 255, px[k][1] = (v >> 8) & 255, px[k][2] = (v >> 16) & 255;
                        todo &= ~(1u << k);
                    }
            }
            __syncthreads();       // hits and wave_hits are written again by the next chunk
        }
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
    DevBuf regions;              // fm_frame_render_redacted: the region list, then its table of {means offset, cell rows before}
    DevBuf means;                // one B, G, R, 0 word per cell (device only)
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr, ev_r0 = nullptr;
    bool timed = false, redact_timed = false;
};

int fm_redact_means_launch(hipStream_t s, const uint8_t* src, int W, int H, const fm_redact_region* regions, int n, const int2* tab,
                           int rows, uint32_t* means);      // redact.hip

void fm_overlay_free(fm_ctx* ctx) {
    OvlState* o = ctx->ovl;
    if (!o) return;
    if (hipStream_t s = fm_jpegenc_stream(ctx)) (void)hipStreamSynchronize(s);
    if (o->buf) (void)hipFree(o->buf);
    o->cmds.release();
    o->masks.release();
    o->regions.release();
    o->means.release();
    for (hipEvent_t ev : {o->ev_t0, o->ev_t1, o->ev_r0})
        if (ev) (void)hipEventDestroy(ev);
    delete o;
    ctx->ovl = nullptr;
}

// fm_frame_render_overlay (redacted = false: no region, the kernel without the redaction stage) and
// fm_frame_render_redacted; both lists have passed their checks
static int render(fm_ctx* ctx, bool redacted, const fm_redact_region* regions, int nr, const fm_overlay_cmd* cmds, int n, const uint8_t* masks,
                  size_t mask_bytes) {
    const int W = ctx->frame_w, H = ctx->frame_h;
    if (int rc = fm_jpegenc_ensure(ctx, 0, 0)) return rc;          // the encoder's stream, created on first use
    hipStream_t s = fm_jpegenc_stream(ctx);
    if (!ctx->ovl) {
        OvlState* o = new OvlState;
        o->means.pinned_mirror = false;
        hipError_t err = hipEventCreate(&o->ev_t0);
        if (err == hipSuccess) err = hipEventCreate(&o->ev_t1);
        if (err == hipSuccess) err = hipEventCreate(&o->ev_r0);
        if (err != hipSuccess) {
            for (hipEvent_t ev : {o->ev_t0, o->ev_t1, o->ev_r0})
                if (ev) (void)hipEventDestroy(ev);
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
    const fm_redact_region* d_regions = nullptr;
    const int2* d_tab = nullptr;
    int rows = 0;
    if (nr > 0) {
        const size_t reg_bytes = (size_t)nr * sizeof(fm_redact_region), all = reg_bytes + (size_t)(nr + 1) * sizeof(int2);
        if (int rc = o->regions.reserve(all)) return rc;
        memcpy(o->regions.h, regions, reg_bytes);
        int2* const tab = reinterpret_cast<int2*>(o->regions.host<char>() + reg_bytes);
        int cells = 0;
        for (int k = 0; k < nr; ++k) {
            const FmRedGrid g = fm_red_grid(regions[k], W, H);
            const int mine = (int)fm_red_cells(regions[k], g);     // (fm_redact_check: at most FM_REDACT_MAX_CELLS in all)
            tab[k] = {cells, rows};
            cells += mine, rows += mine > 0 ? g.jmax - g.jmin + 1 : 0;
        }
        tab[nr] = {cells, rows};
        if (cells > 0)
            if (int rc = o->means.reserve((size_t)cells * sizeof(uint32_t))) return rc;
        FM_HIP(hipMemcpyAsync(o->regions.d, o->regions.h, all, hipMemcpyHostToDevice, s));
        d_regions = o->regions.dev<fm_redact_region>();
        d_tab = reinterpret_cast<const int2*>(o->regions.dev<char>() + reg_bytes);
    }
    // The current frame is complete on the device: the argument of fm_frame_encode_jpeg (jpegenc.hip), unchanged.
    const dim3 grid((W + TILE_W - 1) / TILE_W, (H + TILE_H - 1) / TILE_H);
    if (redacted) FM_HIP(hipEventRecord(o->ev_r0, s));
    if (nr > 0) {
        if (int rc = fm_redact_means_launch(s, ctx->frame_cur, W, H, d_regions, nr, d_tab, rows, o->means.dev<uint32_t>())) return rc;
        FM_HIP(hipEventRecord(o->ev_t0, s));
        hipLaunchKernelGGL(overlay_kernel<true>, grid, dim3(WG), 0, s, ctx->frame_cur, o->buf, W, H, o->cmds.dev<fm_overlay_cmd>(), n,
                           o->masks.dev<uint8_t>(), d_regions, nr, d_tab, o->means.dev<uint32_t>());
    } else {
        FM_HIP(hipEventRecord(o->ev_t0, s));
        hipLaunchKernelGGL(overlay_kernel<false>, grid, dim3(WG), 0, s, ctx->frame_cur, o->buf, W, H, o->cmds.dev<fm_overlay_cmd>(), n,
                           o->masks.dev<uint8_t>(), d_regions, 0, d_tab, (const uint32_t*)nullptr);
    }
    FM_HIP(hipGetLastError());
    FM_HIP(hipEventRecord(o->ev_t1, s));
    FM_HIP(hipStreamSynchronize(s));
    o->timed = true, o->redact_timed = redacted;
    o->w = W, o->h = H;
    return 0;
}

extern "C" int fm_frame_render_overlay(fm_ctx* ctx, const fm_overlay_cmd* cmds, int n, const uint8_t* masks, size_t mask_bytes) {
    FM_CHECK_ARG(ctx && ctx->frame_cur && ctx->frame_w >= 1 && ctx->frame_h >= 1);
    if (int rc = fm_overlay_check(cmds, n, masks, mask_bytes, ctx->frame_w, ctx->frame_h)) return rc;
    return render(ctx, false, nullptr, 0, cmds, n, masks, mask_bytes);
}

extern "C" int fm_frame_render_redacted(fm_ctx* ctx, const fm_redact_region* regions, int n_regions, const fm_overlay_cmd* cmds, int n_cmds,
                                        const uint8_t* masks, size_t mask_bytes) {
    FM_CHECK_ARG(ctx && ctx->frame_cur && ctx->frame_w >= 1 && ctx->frame_h >= 1);
    if (int rc = fm_redact_check(regions, n_regions, ctx->frame_w, ctx->frame_h)) return rc;
    if (int rc = fm_overlay_check(cmds, n_cmds, masks, mask_bytes, ctx->frame_w, ctx->frame_h)) return rc;
    return render(ctx, true, regions, n_regions, cmds, n_cmds, masks, mask_bytes);
}

extern "C" int fm_redact_stream_ms(fm_ctx* ctx, float* ms) {
    FM_CHECK_ARG(ctx && ms);
    *ms = -1.f;
    if (ctx->ovl && ctx->ovl->redact_timed) FM_HIP(hipEventElapsedTime(ms, ctx->ovl->ev_r0, ctx->ovl->ev_t1));
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
