// Frames on the device: the context's frame buffers (the current frame, the look-ahead slots, the ring) and every way a
// frame gets into one.  Nine families of entry points -- BGR, NV12, JPEG, described source (a frame of another size),
// planar, packed, Bayer, deep and device frames -- times three slot protocols: into the current frame, into look-ahead
// slot k, into a ring entry.  Each protocol is written once (into_current, into_ahead, into_ring below) and takes the
// family's part as a callable.  A family brings its argument check (*_ok) and its enqueue_* function: the copies into its
// staging and the kernels that write the BGR frame (nv12.hip, jpeg.hip, resize.hip, remap.hip, yuv.hip, packed.hip,
// hwc.hip, bayer.hip, deep.hip, devsrc.hip; bgr_run.h is what they share).  Its three extern "C" entry points are that check and the protocol.
// Host code only: no kernel lives here.
#include "pixel_source.h"
#include "remap_pixel.h"
#include <mutex>
#include <utility>
#include <vector>

// ---- page-locked frame buffers handed to the caller (process-wide registry of their ranges)
namespace {
std::mutex g_host_mu;
std::vector<std::pair<const uint8_t*, size_t>> g_host_ranges;

bool is_pinned_range(const uint8_t* p, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_host_mu);
    for (auto& r : g_host_ranges)
        if (p >= r.first && p + bytes <= r.first + r.second) return true;
    return false;
}
}  // namespace

bool fm_host_is_pinned(const void* p, size_t bytes) { return is_pinned_range((const uint8_t*)p, bytes); }   // (yuv.hip, jpegenc.hip)

extern "C" int fm_host_alloc(size_t bytes, void** out) {
    FM_CHECK_ARG(out && bytes > 0);
    void* p = nullptr;
    FM_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        g_host_ranges.emplace_back((const uint8_t*)p, bytes);
    }
    *out = p;
    return 0;
}

extern "C" int fm_host_free(void* p) {
    if (!p) return 0;
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        for (size_t i = 0; i < g_host_ranges.size(); ++i)
            if (g_host_ranges[i].first == (const uint8_t*)p) {
                g_host_ranges.erase(g_host_ranges.begin() + i);
                break;
            }
    }
    FM_HIP(hipHostFree(p));
    return 0;
}

// ---- staging: what the families keep between calls, all of it sized by the frame or by the source and allocated on
// first use
static void src_stages_free(fm_ctx::SrcStage* stages, int n) {
    for (int i = 0; i < n; ++i) {
        fm_ctx::SrcStage& e = stages[i];
        if (e.bgr) (void)hipFree(e.bgr);
        if (e.dev) (void)hipFree(e.dev);
        if (e.pinned) (void)hipHostFree(e.pinned);
        if (e.ev) (void)hipEventDestroy(e.ev);
        e = fm_ctx::SrcStage{};
    }
}

// ---- the correction map (remap.hip): while one is set, every described-source call -- fm_frame_*_src and the planar,
// packed, Bayer and deep families below -- takes sources of the map's size only, stages them at that size even when it is the
// configured one, and ends in fm_remap_bgr where it ends in fm_resize_bgr without.
static void remap_free(fm_ctx* ctx) {
    if (ctx->remap_xy) (void)hipFree(ctx->remap_xy);
    ctx->remap_xy = nullptr;
    ctx->remap_sw = ctx->remap_sh = 0;
    ctx->remap_border = 0;
}

// the streams whose queued kernels may still read the map: the three the described-source calls launch on
static int remap_idle(fm_ctx* ctx) {
    FM_HIP(hipStreamSynchronize(ctx->s_det));
    FM_HIP(hipStreamSynchronize(ctx->s_ext));
    if (fm_det_front_stream(ctx)) FM_HIP(hipStreamSynchronize(fm_det_front_stream(ctx)));
    FM_HIP(hipStreamSynchronize(nullptr));
    return 0;
}

extern "C" int fm_frame_remap_set(fm_ctx* ctx, int src_w, int src_h, const int32_t* xy, const uint8_t border_bgr[3]) {
    FM_CHECK_ARG(ctx && ctx->frame_own && xy && border_bgr);
    FM_CHECK_ARG(src_w >= 1 && src_h >= 1 && src_w <= FM_SRC_MAX_DIM && src_h <= FM_SRC_MAX_DIM);
    const size_t n = (size_t)ctx->frame_w * ctx->frame_h;
    for (size_t i = 0; i < n; ++i) FM_CHECK_ARG(fm_remap_entry_ok(xy[2 * i], xy[2 * i + 1], src_w, src_h));
    int rc = remap_idle(ctx);
    if (rc) return rc;
    int32_t* dev = nullptr;
    FM_HIP(hipMalloc(&dev, n * 2 * sizeof(int32_t)));
    if (hipError_t e = hipMemcpy(dev, xy, n * 2 * sizeof(int32_t), hipMemcpyHostToDevice); e != hipSuccess) {
        (void)hipFree(dev);
        FM_HIP(e);
    }
    remap_free(ctx);
    ctx->remap_xy = dev;
    ctx->remap_sw = src_w, ctx->remap_sh = src_h;
    ctx->remap_border = (uint32_t)border_bgr[0] | (uint32_t)border_bgr[1] << 8 | (uint32_t)border_bgr[2] << 16;
    return 0;
}

extern "C" int fm_frame_remap_clear(fm_ctx* ctx) {
    FM_CHECK_ARG(ctx);
    if (!ctx->remap_xy) return 0;
    int rc = remap_idle(ctx);
    if (rc) return rc;
    remap_free(ctx);
    return 0;
}

// a w x h source is one the described-source calls take now: any without a map, the map's size with one
static bool remap_takes(const fm_ctx* ctx, int w, int h) { return !ctx->remap_xy || (w == ctx->remap_sw && h == ctx->remap_sh); }

// a w x h source needs no kernel of the tail below: it has the configured size and no map is set
static bool src_on_size(const fm_ctx* ctx, int w, int h) { return !ctx->remap_xy && w == ctx->frame_w && h == ctx->frame_h; }
static bool src_on_size(const fm_ctx* ctx, const struct fm_frame_src* f) { return src_on_size(ctx, f->width, f->height); }

// Frees every family's staging, the off-size sources' and the correction map: fm_frame_configure (they are allocated
// again on first use at the new size; a map is for one frame size and is set again by the caller) and fm_ctx_destroy.
// No sync: the caller's.
void fm_frame_staging_free(fm_ctx* ctx) {
    for (uint8_t** stage : {ctx->frame_nv12, ctx->frame_planar, ctx->frame_packed, ctx->frame_bayer, ctx->frame_jpeg})
        for (int i = 0; i < FM_MAX_DET_BATCH + 2; ++i) {
            if (stage[i]) (void)hipFree(stage[i]);
            stage[i] = nullptr;
        }
    for (uint8_t*& p : ctx->frame_jpeg_pinned) {
        if (p) (void)hipHostFree(p);
        p = nullptr;
    }
    src_stages_free(ctx->frame_src, FM_MAX_DET_BATCH + 2);
    src_stages_free(ctx->frame_deep, FM_MAX_DET_BATCH + 2);
    remap_free(ctx);
}

extern "C" int fm_frame_configure(fm_ctx* ctx, int width, int height, int ring_size) {
    FM_CHECK_ARG(ctx && width > 0 && height > 0 && ring_size >= 0);
    FM_HIP(hipDeviceSynchronize());
    for (void* p : {(void*)ctx->frame_own, (void*)ctx->frame_own2, (void*)ctx->frame_ring})
        if (p) (void)hipFree(p);
    for (void* p : {(void*)ctx->frame_pinned, (void*)ctx->frame_pinned2})
        if (p) (void)hipHostFree(p);
    ctx->frame_own = ctx->frame_own2 = ctx->frame_ring = ctx->frame_pinned = ctx->frame_pinned2 = nullptr;
    ctx->frame_next = nullptr;
    for (int k = 2; k <= FM_MAX_DET_BATCH; ++k) {      // look-ahead slots: allocated again on first use at the new size
        if (ctx->frame_up[k]) (void)hipFree(ctx->frame_up[k]);
        if (ctx->frame_up_pinned[k]) (void)hipHostFree(ctx->frame_up_pinned[k]);
        ctx->frame_up[k] = ctx->frame_up_pinned[k] = ctx->frame_ahead[k] = nullptr;
    }
    fm_frame_staging_free(ctx);
    const size_t bytes = (size_t)width * height * 3;
    FM_HIP(hipMalloc(&ctx->frame_own, bytes + FM_FRAME_SLACK));        // (pixel_source.h load_px2 reads 8 bytes at a pixel)
    FM_HIP(hipMalloc(&ctx->frame_own2, bytes + FM_FRAME_SLACK));
    FM_HIP(hipHostMalloc(&ctx->frame_pinned, bytes, hipHostMallocDefault));
    FM_HIP(hipHostMalloc(&ctx->frame_pinned2, bytes, hipHostMallocDefault));
    if (ring_size > 0) FM_HIP(hipMalloc(&ctx->frame_ring, bytes * ring_size + FM_FRAME_SLACK));
    ctx->frame_w = width;
    ctx->frame_h = height;
    ctx->ring_size = ring_size;
    ctx->frame_cur = ctx->frame_own;
    return 0;
}

// at least `bytes` at p; a buffer that has to grow is given up once `s`, the stream whose copies and kernels use it, is idle
static int src_reserve(uint8_t*& p, size_t& cap, size_t bytes, bool host, hipStream_t s) {
    if (bytes <= cap) return 0;
    if (p) {
        FM_HIP(hipStreamSynchronize(s));
        if (host) (void)hipHostFree(p); else (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    if (host) FM_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    else FM_HIP(hipMalloc(&p, bytes));
    cap = bytes;
    return 0;
}

// page-locked staging of `bytes` for the entry, free to be written: the previous H2D copy out of it is done
static int src_pinned(fm_ctx::SrcStage& st, size_t bytes, hipStream_t s) {
    int rc = src_reserve(st.pinned, st.pinned_cap, bytes, true, s);
    if (rc) return rc;
    if (st.ev) FM_HIP(hipEventSynchronize(st.ev));
    return 0;
}
static int src_pinned_copied(fm_ctx::SrcStage& st, hipStream_t s) {
    if (!st.ev) FM_HIP(hipEventCreateWithFlags(&st.ev, hipEventDisableTiming));
    FM_HIP(hipEventRecord(st.ev, s));
    return 0;
}

// The page-locked buffer that rows are packed into when they cannot be copied from where they lie.  Either a slot's own
// (`pinned`, with `reuse`, the event behind the previous copy out of it; the slot protocol records that event again), or a
// SrcStage's (`own`: grown to the bytes asked for, with the event it keeps itself).
struct Staging {
    uint8_t* pinned;
    hipEvent_t reuse;
    fm_ctx::SrcStage* own;
    // the buffer, at least `bytes` and free to be written: the previous H2D copy out of it is done
    int acquire(size_t bytes, hipStream_t s, uint8_t** out) const {
        if (own) {
            int rc = src_pinned(*own, bytes, s);
            *out = own->pinned;
            return rc;
        }
        if (reuse) FM_HIP(hipEventSynchronize(reuse));
        *out = pinned;
        return 0;
    }
    // an H2D copy out of the buffer has been enqueued on `s`
    int copied(hipStream_t s) const { return own ? src_pinned_copied(*own, s) : 0; }
};

// ---- the copy every row-shaped family makes: the rows of a frame's planes, packed to their bytes, one plane behind the
// other, into device staging
struct Plane {
    const uint8_t* ptr;
    size_t pitch, row_bytes;
    int rows;
};

// which planes are copied from where they lie
enum class Direct {
    SURFACE,            // packed rows, one plane right behind the other, inside one page-locked buffer: one copy
    PLANES_OR_SURFACE,  // packed rows, every plane inside a page-locked buffer: a copy per plane, or one for a surface
    PLANES,             // the same, always a copy per plane
};

// `blocking`: a blocking hipMemcpy2D per plane.  Otherwise copies on `s`: from where the planes lie when `direct` allows
// it; if not, the rows are packed into `staging` once the previous copy out of it is done, and one copy follows.
static int copy_planes(uint8_t* dev, const Plane* planes, int n, Direct direct, const Staging& staging, hipStream_t s, bool blocking) {
    size_t off[4] = {}, total = 0;         // (n <= 3)
    bool packed = true, contiguous = true;
    for (int p = 0; p < n; ++p) {
        off[p] = total;
        packed = packed && planes[p].pitch == planes[p].row_bytes;
        contiguous = contiguous && planes[p].ptr == planes[0].ptr + total;
        total += planes[p].row_bytes * planes[p].rows;
    }
    off[n] = total;
    if (blocking) {
        for (int p = 0; p < n; ++p)
            FM_HIP(hipMemcpy2D(dev + off[p], planes[p].row_bytes, planes[p].ptr, planes[p].pitch, planes[p].row_bytes, planes[p].rows,
                               hipMemcpyHostToDevice));
        return 0;
    }
    bool surface = false, each = false;
    if (direct == Direct::SURFACE) {
        surface = packed && contiguous && is_pinned_range(planes[0].ptr, total);
    } else if (packed) {
        each = true;
        for (int p = 0; p < n; ++p) each = each && is_pinned_range(planes[p].ptr, off[p + 1] - off[p]);
        surface = each && contiguous && direct == Direct::PLANES_OR_SURFACE;
    }
    if (surface) {
        FM_HIP(hipMemcpyAsync(dev, planes[0].ptr, total, hipMemcpyHostToDevice, s));
    } else if (each) {
        for (int p = 0; p < n; ++p) FM_HIP(hipMemcpyAsync(dev + off[p], planes[p].ptr, off[p + 1] - off[p], hipMemcpyHostToDevice, s));
    } else {
        uint8_t* pin = nullptr;
        int rc = staging.acquire(total, s, &pin);
        if (rc) return rc;
        for (int p = 0; p < n; ++p)
            for (int r = 0; r < planes[p].rows; ++r)
                memcpy(pin + off[p] + (size_t)r * planes[p].row_bytes, planes[p].ptr + (size_t)r * planes[p].pitch, planes[p].row_bytes);
        FM_HIP(hipMemcpyAsync(dev, pin, total, hipMemcpyHostToDevice, s));
        if ((rc = staging.copied(s))) return rc;
    }
    return 0;
}

// ---- the three slot protocols.  What a protocol hands to a family's enqueue_* function:
struct Target {
    int entry;          // the family's staging entry: 0 the current frame, k look-ahead slot k, FM_MAX_DET_BATCH + 1 the ring
    uint8_t* dst;       // the BGR frame to write
    hipStream_t s;      // the copies and kernels go here
    uint8_t* pinned;    // the slot's BGR-sized page-locked buffer (the ring has none) ...
    hipEvent_t reuse;   // ... and the event behind the previous copy out of it, when there is one
    bool blocking;      // blocking copies from where the source lies
};

// Into the current frame.
template <class Enqueue> static int into_current(fm_ctx* ctx, Enqueue enqueue) {
    // every consumer of the previous frame must be done before it is overwritten
    FM_HIP(hipStreamSynchronize(ctx->s_det));
    FM_HIP(hipStreamSynchronize(ctx->s_ext));
    FM_HIP(hipStreamSynchronize(ctx->s_flow));
    FM_HIP(hipStreamSynchronize(ctx->s_flow2));
    if (fm_det_front_stream(ctx)) FM_HIP(hipStreamSynchronize(fm_det_front_stream(ctx)));    // (a detector front reads its frame there)
    int rc = enqueue(Target{0, ctx->frame_own, ctx->s_det, ctx->frame_pinned, nullptr, false});
    if (rc) return rc;
    FM_HIP(hipStreamSynchronize(ctx->s_det));   // the other streams read the frame too (and a caller's memory has been read)
    ctx->frame_cur = ctx->frame_own;
    return 0;
}

// ---- next-frame prefetch: the detector may be started on frame t+1 while frame t is still being tracked
// (MOT.step(frame, next_frame)).  The next frame lives in the second upload slot (or the ring) and becomes
// the current one with fm_frame_promote_next -- no second upload.
// Look-ahead slot k: the frame the step k steps ahead receives.  Slot 1 is the fields of the next-frame prefetch
// (frame_next, upload slot frame_own2 / frame_pinned2 / ev_next_upload), slots 2.. those of fm_ctx::frame_ahead /
// frame_up / frame_up_pinned / ev_up (fm_ahead_frame / _buf / _event in common.h).  An upload slot's buffers move with its
// frame when fm_frame_promote_next shifts the slots, so that slot 1's frame always lies in frame_own2 when it was uploaded.
static uint8_t*& ahead_pinned(fm_ctx* ctx, int k) { return k == 1 ? ctx->frame_pinned2 : ctx->frame_up_pinned[k]; }

// Into look-ahead slot k (1 <= k <= FM_MAX_DET_BATCH, checked by the caller).  An enqueue that fails leaves the slot as
// it was: no event recorded, no frame in it.
template <class Enqueue> static int into_ahead(fm_ctx* ctx, int k, Enqueue enqueue) {
    const size_t bytes = (size_t)ctx->frame_w * ctx->frame_h * 3;
    if (!fm_ahead_buf(ctx, k)) {       // slots k >= 2: on first use, with the staging a plain upload into the slot expects
        FM_HIP(hipMalloc(&fm_ahead_buf(ctx, k), bytes + FM_FRAME_SLACK));
        FM_HIP(hipHostMalloc(&ahead_pinned(ctx, k), bytes, hipHostMallocDefault));
    }
    uint8_t* const buf = fm_ahead_buf(ctx, k);
    hipEvent_t& ev = fm_ahead_event(ctx, k);
    // The previous readers of the slot's buffer -- every stage of the step before the last promote, its detector pass
    // included -- are done (fm_frame_promote_next synchronised the ReID / KLT streams, that pass was collected; a batched
    // pass is complete once any of its frames was collected).  The
    // copy goes to the ReID stream: that stream is idle at this point of a step (its network starts once this frame's
    // detections have been collected, long after a 6 MB copy), it is a high-priority stream, and the pass on the new
    // frame waits for the copy's event only.  On the low-priority stream that carries the post-processing the copy was
    // held back while the KLT / ReID kernels of the running step kept the high-priority queues busy, and the detector
    // -- the longest chain of a step -- started late every frame: 662 -> 780 frames/s for this move alone, 872 together
    // with MOT.step enqueueing the prefetch before it starts the KLT job (config[1]; config[4] 100 -> 158;
    // profiles/r03_pipeline_order_ab.txt holds the whole matrix, the tracker stream and a high-priority upload stream
    // included: 550-600 and 450).
    // The slot's event is recorded behind the family's LAST kernel: a reader that waits for it (the detector pass,
    // fm_frame_promote_next) finds the BGR frame complete.  The slot's buffers and that event move with the frame at a
    // promote; a family's own staging (frame_nv12 .. frame_jpeg, frame_src, frame_deep) stays with the slot NUMBER: its
    // device buffers need no event (copies and kernels of a slot share one stream), its page-locked ones have their own
    // (ev_jpeg[k], SrcStage::ev).
    hipStream_t cs = ctx->s_ext;
    fm_trace_mark(ctx, cs, 30);
    int rc = enqueue(Target{k, buf, cs, ahead_pinned(ctx, k), ev, false});
    if (rc) return rc;
    fm_trace_mark(ctx, cs, 31);
    if (!ev) FM_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    FM_HIP(hipEventRecord(ev, cs));
    // see flush_post (detect.hip).  With front-ahead on the post-processing stream the pass that follows this upload
    // enqueues its front there first and the pending post-processing, which waits for the running pass, behind it.
    if (k == 1 && fm_det_defers_flush(ctx))
        ctx->det_flush_deferred = true;
    else if ((rc = fm_det_flush_post(ctx))) return rc;
    fm_ahead_frame(ctx, k) = buf;
    return 0;
}

// Into ring entry `index` (checked by the caller).  Synchronous, filling the ring is set-up work: blocking copies from
// where the source lies, then the kernels on the null stream.
template <class Enqueue> static int into_ring(fm_ctx* ctx, int index, Enqueue enqueue) {
    uint8_t* const dst = ctx->frame_ring + (size_t)ctx->frame_w * ctx->frame_h * 3 * index;
    int rc = enqueue(Target{FM_MAX_DET_BATCH + 1, dst, nullptr, nullptr, nullptr, true});
    if (rc) return rc;
    FM_HIP(hipStreamSynchronize(nullptr));
    return 0;
}

// ---- BGR frames of the configured size.
// H2D copy of the frame (the copy engine; a copy KERNEL measured no faster in round 2): from where it lies in page-locked
// memory, through the slot's staging otherwise -- and only then is the event behind that staging's previous copy waited for
static int enqueue_bgr(fm_ctx* ctx, const Target& t, const uint8_t* bgr) {
    const size_t bytes = (size_t)ctx->frame_w * ctx->frame_h * 3;
    const uint8_t* src = bgr;
    if (!is_pinned_range(bgr, bytes)) {
        // previous H2D copy out of the staging buffer: its event, not the stream (a detector pass may be running)
        if (t.reuse) FM_HIP(hipEventSynchronize(t.reuse));
        memcpy(t.pinned, bgr, bytes);
        src = t.pinned;
    }
    FM_HIP(hipMemcpyAsync(t.dst, src, bytes, hipMemcpyHostToDevice, t.s));
    return 0;
}

extern "C" int fm_frame_upload(fm_ctx* ctx, const uint8_t* bgr) {
    FM_CHECK_ARG(ctx && bgr && ctx->frame_own);
    return into_current(ctx, [&](const Target& t) { return enqueue_bgr(ctx, t, bgr); });
}

extern "C" int fm_frame_upload_next(fm_ctx* ctx, const uint8_t* bgr) { return fm_frame_upload_ahead(ctx, 1, bgr); }

extern "C" int fm_frame_upload_ahead(fm_ctx* ctx, int k, const uint8_t* bgr) {
    FM_CHECK_ARG(ctx && bgr && ctx->frame_own2 && k >= 1 && k <= FM_MAX_DET_BATCH);
    return into_ahead(ctx, k, [&](const Target& t) { return enqueue_bgr(ctx, t, bgr); });
}

extern "C" int fm_frame_ring_select_next(fm_ctx* ctx, int index) { return fm_frame_ring_select_ahead(ctx, 1, index); }

extern "C" int fm_frame_ring_select_ahead(fm_ctx* ctx, int k, int index) {
    FM_CHECK_ARG(ctx && index >= 0 && index < ctx->ring_size && k >= 1 && k <= FM_MAX_DET_BATCH);
    fm_ahead_frame(ctx, k) = ctx->frame_ring + (size_t)ctx->frame_w * ctx->frame_h * 3 * index;
    return 0;
}

extern "C" int fm_frame_promote_next(fm_ctx* ctx) {
    FM_CHECK_ARG(ctx && ctx->frame_next);
    if (ctx->frame_next == ctx->frame_own2) {
        // the upload of the prefetched frame was enqueued on the ReID stream (fm_frame_upload_next); every stream that
        // reads the frame from now on waits for that copy's event
        FM_HIP(hipStreamSynchronize(ctx->s_ext));
        FM_HIP(hipStreamSynchronize(ctx->s_flow));
        FM_HIP(hipStreamSynchronize(ctx->s_flow2));
        // (the copy ran a step ago: when the host already sees its event complete, four barrier packets -- one in front of
        // the next frame's copy on the ReID stream -- need not be enqueued at all)
        if (hipEventQuery(ctx->ev_next_upload) != hipSuccess) {
            (void)hipGetLastError();
            FM_HIP(hipStreamWaitEvent(ctx->s_ext, ctx->ev_next_upload, 0));
            FM_HIP(hipStreamWaitEvent(ctx->s_flow, ctx->ev_next_upload, 0));
            FM_HIP(hipStreamWaitEvent(ctx->s_flow2, ctx->ev_next_upload, 0));
            FM_HIP(hipStreamWaitEvent(ctx->s_main, ctx->ev_next_upload, 0));
        }
        std::swap(ctx->frame_own, ctx->frame_own2);
        std::swap(ctx->frame_pinned, ctx->frame_pinned2);
        ctx->frame_cur = ctx->frame_own;
    } else {
        ctx->frame_cur = ctx->frame_next;
    }
    ctx->frame_next = nullptr;
    // look-ahead: slot k becomes slot k - 1; a frame in its upload slot takes that slot's buffers along (the free buffer
    // -- the previous frame's -- moves up in exchange)
    for (int k = 2; k <= FM_MAX_DET_BATCH; ++k) {
        uint8_t* f = ctx->frame_ahead[k];
        if (f && f == ctx->frame_up[k]) {
            std::swap(fm_ahead_buf(ctx, k - 1), fm_ahead_buf(ctx, k));
            std::swap(ahead_pinned(ctx, k - 1), ahead_pinned(ctx, k));
            std::swap(fm_ahead_event(ctx, k - 1), fm_ahead_event(ctx, k));
        }
        fm_ahead_frame(ctx, k - 1) = f;
        ctx->frame_ahead[k] = nullptr;
    }
    return 0;
}

// (one blocking copy: no staging entry, no kernel, nothing on the null stream to wait for)
extern "C" int fm_frame_ring_store(fm_ctx* ctx, int index, const uint8_t* bgr) {
    FM_CHECK_ARG(ctx && bgr && index >= 0 && index < ctx->ring_size);
    const size_t bytes = (size_t)ctx->frame_w * ctx->frame_h * 3;
    FM_HIP(hipMemcpy(ctx->frame_ring + bytes * index, bgr, bytes, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int fm_frame_ring_select(fm_ctx* ctx, int index) {
    FM_CHECK_ARG(ctx && index >= 0 && index < ctx->ring_size);
    ctx->frame_cur = ctx->frame_ring + (size_t)ctx->frame_w * ctx->frame_h * 3 * index;
    return 0;
}

extern "C" int fm_frame_read(fm_ctx* ctx, uint8_t* bgr) {
    FM_CHECK_ARG(ctx && bgr && ctx->frame_cur);
    FM_HIP(hipDeviceSynchronize());
    FM_HIP(hipMemcpy(bgr, ctx->frame_cur, (size_t)ctx->frame_w * ctx->frame_h * 3, hipMemcpyDeviceToHost));
    return 0;
}

// ---- NV12 ingest: a Y plane + an interleaved UV plane with a row pitch.  Between the H2D copy (1.5 bytes per pixel, into
// ctx->frame_nv12[entry]) and whatever follows it on the stream, the conversion kernel of nv12.hip writes the BGR frame.
#define FM_CHECK_NV12(ctx, y, uv, pitch, matrix)                                                                  \
    FM_CHECK_ARG((y) && (uv) && (pitch) >= (ctx)->frame_w && ((matrix) == FM_NV12_BT601 || (matrix) == FM_NV12_BT709) && \
                 !((ctx)->frame_w & 1) && !((ctx)->frame_h & 1))

// Planes that cannot be copied from where they are (pageable memory, or a pitch) go through the slot's staging.
static int enqueue_nv12(fm_ctx* ctx, const Target& t, const uint8_t* y, const uint8_t* uv, int pitch, int matrix) {
    const int w = ctx->frame_w, h = ctx->frame_h;
    const size_t npx = (size_t)w * h;
    uint8_t*& stage = ctx->frame_nv12[t.entry];
    if (!stage) FM_HIP(hipMalloc(&stage, npx + npx / 2));
    const Plane planes[2] = {{y, (size_t)pitch, (size_t)w, h}, {uv, (size_t)pitch, (size_t)w, h / 2}};
    int rc = copy_planes(stage, planes, 2, Direct::PLANES_OR_SURFACE, Staging{t.pinned, t.reuse, nullptr}, t.s, t.blocking);
    if (rc) return rc;
    fm_trace_mark(ctx, t.s, 36);               // (the conversion's share of the caller's 30 .. 31 interval)
    return fm_nv12_to_bgr(stage, t.dst, w, h, matrix, t.s);
}

extern "C" int fm_frame_upload_nv12(fm_ctx* ctx, const uint8_t* y, const uint8_t* uv, int pitch, int matrix) {
    FM_CHECK_ARG(ctx && ctx->frame_own);
    FM_CHECK_NV12(ctx, y, uv, pitch, matrix);
    return into_current(ctx, [&](const Target& t) { return enqueue_nv12(ctx, t, y, uv, pitch, matrix); });
}

extern "C" int fm_frame_upload_ahead_nv12(fm_ctx* ctx, int k, const uint8_t* y, const uint8_t* uv, int pitch, int matrix) {
    FM_CHECK_ARG(ctx && ctx->frame_own2 && k >= 1 && k <= FM_MAX_DET_BATCH);
    FM_CHECK_NV12(ctx, y, uv, pitch, matrix);
    return into_ahead(ctx, k, [&](const Target& t) { return enqueue_nv12(ctx, t, y, uv, pitch, matrix); });
}

extern "C" int fm_frame_ring_store_nv12(fm_ctx* ctx, int index, const uint8_t* y, const uint8_t* uv, int pitch, int matrix) {
    FM_CHECK_ARG(ctx && index >= 0 && index < ctx->ring_size);
    FM_CHECK_NV12(ctx, y, uv, pitch, matrix);
    return into_ring(ctx, index, [&](const Target& t) { return enqueue_nv12(ctx, t, y, uv, pitch, matrix); });
}
#undef FM_CHECK_NV12

// ---- JPEG ingest: a frame that arrives as the output of fm_jpeg_entropy_decode (jpeg_host.hip).  Between the H2D copy
// (coefficients + quantisation tables, into ctx->frame_jpeg[entry]) and whatever follows it on the stream, the two kernels
// of jpeg.hip write the BGR frame.

// int16 coefficients of the largest supported layout of a w x h frame: 4:4:4 on a grid padded to 16 pixels (which bounds
// the 8-pixel grid 4:4:4 really has, and 4:2:2 / 4:2:0 / one component at half that or less)
static size_t jpeg_max_coefs(int w, int h) { return (size_t)3 * ((w + 15) & ~15) * ((h + 15) & ~15); }
static size_t jpeg_stage_bytes(int w, int h) { return fm_jpeg_sample_offset((long long)jpeg_max_coefs(w, h)) + jpeg_max_coefs(w, h); }

// `info` describes a supported layout of a w x h frame, every derived field as fm_jpeg_info computes it
static bool jpeg_layout_ok_size(const struct fm_jpeg_info* info, int w, int h) {
    if (!info || info->width != w || info->height != h) return false;
    struct fm_jpeg_info want;
    if (fm_jpeg_layout(info->width, info->height, info->ncomp, info->hsamp[0], info->vsamp[0], &want)) return false;
    for (int c = 0; c < 3; ++c)
        if (info->blocks_w[c] != want.blocks_w[c] || info->blocks_h[c] != want.blocks_h[c] || info->coef_offset[c] != want.coef_offset[c])
            return false;
    // (the launch grids of jpeg.hip: one lane per block row, one thread per 8 pixels of a row)
    if (want.coef_count / 64 >= (1ll << 28) || (long long)((info->width + 7) >> 3) * info->height >= (1ll << 31)) return false;
    return info->coef_count == want.coef_count && (size_t)want.coef_count <= jpeg_max_coefs(w, h);
}
// ... of the configured frame size
static bool jpeg_layout_ok(const fm_ctx* ctx, const struct fm_jpeg_info* info) { return jpeg_layout_ok_size(info, ctx->frame_w, ctx->frame_h); }
#define FM_CHECK_JPEG(ctx, info, coef, qt) FM_CHECK_ARG((coef) && (qt) && jpeg_layout_ok(ctx, info))

// Buffers that cannot be copied from where they are (pageable memory) are packed into the entry's own page-locked staging
// first, frame_jpeg_pinned[entry].  A look-ahead entry has ev_jpeg[entry] behind the previous copy out of it: waited for
// before the buffer is written, recorded again behind the new copy.  (Entry 0 needs none: fm_frame_upload_jpeg returns
// with its stream idle.)
static int enqueue_jpeg(fm_ctx* ctx, const Target& t, const struct fm_jpeg_info* info, const int16_t* coef, const uint16_t* qt) {
    const size_t cbytes = (size_t)info->coef_count * 2, qbytes = 3 * 64 * 2;
    hipStream_t s = t.s;
    uint8_t*& stage = ctx->frame_jpeg[t.entry];
    if (!stage) FM_HIP(hipMalloc(&stage, jpeg_stage_bytes(ctx->frame_w, ctx->frame_h)));
    const uint8_t* const c8 = reinterpret_cast<const uint8_t*>(coef);
    const uint8_t* const q8 = reinterpret_cast<const uint8_t*>(qt);
    if (t.blocking) {
        FM_HIP(hipMemcpy(stage, c8, cbytes, hipMemcpyHostToDevice));
        FM_HIP(hipMemcpy(stage + cbytes, q8, qbytes, hipMemcpyHostToDevice));
    } else if (is_pinned_range(c8, cbytes) && is_pinned_range(q8, qbytes)) {
        if (q8 == c8 + cbytes) {
            FM_HIP(hipMemcpyAsync(stage, c8, cbytes + qbytes, hipMemcpyHostToDevice, s));
        } else {
            FM_HIP(hipMemcpyAsync(stage, c8, cbytes, hipMemcpyHostToDevice, s));
            FM_HIP(hipMemcpyAsync(stage + cbytes, q8, qbytes, hipMemcpyHostToDevice, s));
        }
    } else {
        uint8_t*& pinned = ctx->frame_jpeg_pinned[t.entry];
        hipEvent_t* const reuse = t.entry ? &ctx->ev_jpeg[t.entry] : nullptr;
        if (!pinned) FM_HIP(hipHostMalloc(&pinned, jpeg_max_coefs(ctx->frame_w, ctx->frame_h) * 2 + qbytes, hipHostMallocDefault));
        if (reuse && *reuse) FM_HIP(hipEventSynchronize(*reuse));
        memcpy(pinned, c8, cbytes);
        memcpy(pinned + cbytes, q8, qbytes);
        FM_HIP(hipMemcpyAsync(stage, pinned, cbytes + qbytes, hipMemcpyHostToDevice, s));
        if (reuse) {
            if (!*reuse) FM_HIP(hipEventCreateWithFlags(reuse, hipEventDisableTiming));
            FM_HIP(hipEventRecord(*reuse, s));
        }
    }
    fm_trace_mark(ctx, s, 37);                 // (the decode's share of the caller's 30 .. 31 interval)
    return fm_jpeg_to_bgr(stage, t.dst, info, s);
}

extern "C" int fm_frame_upload_jpeg(fm_ctx* ctx, const struct fm_jpeg_info* info, const int16_t* coef, const uint16_t* qt) {
    FM_CHECK_ARG(ctx && ctx->frame_own);
    FM_CHECK_JPEG(ctx, info, coef, qt);
    return into_current(ctx, [&](const Target& t) { return enqueue_jpeg(ctx, t, info, coef, qt); });
}

extern "C" int fm_frame_upload_ahead_jpeg(fm_ctx* ctx, int k, const struct fm_jpeg_info* info, const int16_t* coef, const uint16_t* qt) {
    FM_CHECK_ARG(ctx && ctx->frame_own2 && k >= 1 && k <= FM_MAX_DET_BATCH);
    FM_CHECK_JPEG(ctx, info, coef, qt);
    return into_ahead(ctx, k, [&](const Target& t) { return enqueue_jpeg(ctx, t, info, coef, qt); });
}

extern "C" int fm_frame_ring_store_jpeg(fm_ctx* ctx, int index, const struct fm_jpeg_info* info, const int16_t* coef, const uint16_t* qt) {
    FM_CHECK_ARG(ctx && index >= 0 && index < ctx->ring_size);
    FM_CHECK_JPEG(ctx, info, coef, qt);
    return into_ring(ctx, index, [&](const Target& t) { return enqueue_jpeg(ctx, t, info, coef, qt); });
}
#undef FM_CHECK_JPEG

// ---- frames at another size than the configured one: a described source (struct fm_frame_src).  A source of the
// configured size goes to the counterpart above.  Any other is copied -- and, for NV12 / JPEG, converted by the kernels
// above -- at ITS size into ctx->frame_src[entry].bgr, and the kernel of resize.hip writes the frame the counterpart would
// have written.  The staging is this path's own and sized by the source.
static bool src_ok(const struct fm_frame_src* f) {
    if (!f || f->width < 1 || f->height < 1 || f->width > FM_SRC_MAX_DIM || f->height > FM_SRC_MAX_DIM) return false;
    switch (f->kind) {
    case FM_SRC_BGR: return f->bgr != nullptr;
    case FM_SRC_NV12:
        return f->y && f->uv && f->pitch >= f->width && (f->matrix == FM_NV12_BT601 || f->matrix == FM_NV12_BT709) &&
               !(f->width & 1) && !(f->height & 1);
    case FM_SRC_JPEG: return f->coef && f->qt && jpeg_layout_ok_size(f->info, f->width, f->height);
    }
    return false;
}

// The last kernel of every described-source route: the source-size BGR frame `bgr` (w x h, + FM_FRAME_SLACK) into the
// configured-size frame `dst` on `s` -- through the correction map when one is set, resized otherwise.
static int enqueue_src_tail(fm_ctx* ctx, const uint8_t* bgr, int w, int h, uint8_t* dst, hipStream_t s) {
    fm_trace_mark(ctx, s, 38);                 // (the resize's / remap's share of the caller's 30 .. 31 interval)
    if (ctx->remap_xy) return fm_remap_bgr(bgr, w, h, ctx->remap_xy, dst, ctx->frame_w, ctx->frame_h, ctx->remap_border, s);
    return fm_resize_bgr(bgr, w, h, dst, ctx->frame_w, ctx->frame_h, s);
}

// The off-size source `f` (checked by the caller) into the entry's source-resolution buffers and, resized, into t.dst.
static int enqueue_src(fm_ctx* ctx, const Target& t, const struct fm_frame_src* f) {
    fm_ctx::SrcStage& st = ctx->frame_src[t.entry];
    hipStream_t s = t.s;
    const int w = f->width, h = f->height;
    const size_t npx = (size_t)w * h;
    int rc = src_reserve(st.bgr, st.bgr_cap, npx * 3 + FM_FRAME_SLACK, false, s);     // (resize.hip reads 8 bytes at a pixel)
    if (rc) return rc;
    if (f->kind == FM_SRC_BGR) {
        if (t.blocking) {
            FM_HIP(hipMemcpy(st.bgr, f->bgr, npx * 3, hipMemcpyHostToDevice));
        } else if (is_pinned_range(f->bgr, npx * 3)) {
            FM_HIP(hipMemcpyAsync(st.bgr, f->bgr, npx * 3, hipMemcpyHostToDevice, s));
        } else {
            if ((rc = src_pinned(st, npx * 3, s))) return rc;
            memcpy(st.pinned, f->bgr, npx * 3);
            FM_HIP(hipMemcpyAsync(st.bgr, st.pinned, npx * 3, hipMemcpyHostToDevice, s));
            if ((rc = src_pinned_copied(st, s))) return rc;
        }
    } else if (f->kind == FM_SRC_NV12) {
        if ((rc = src_reserve(st.dev, st.dev_cap, npx + npx / 2, false, s))) return rc;
        const Plane planes[2] = {{f->y, (size_t)f->pitch, (size_t)w, h}, {f->uv, (size_t)f->pitch, (size_t)w, h / 2}};
        if ((rc = copy_planes(st.dev, planes, 2, Direct::PLANES, Staging{nullptr, nullptr, &st}, s, t.blocking))) return rc;
        fm_trace_mark(ctx, s, 36);
        if ((rc = fm_nv12_to_bgr(st.dev, st.bgr, w, h, f->matrix, s))) return rc;
    } else {
        const size_t cbytes = (size_t)f->info->coef_count * 2, qbytes = 3 * 64 * 2;
        if ((rc = src_reserve(st.dev, st.dev_cap, jpeg_stage_bytes(w, h), false, s))) return rc;
        const uint8_t* const c8 = reinterpret_cast<const uint8_t*>(f->coef);
        const uint8_t* const q8 = reinterpret_cast<const uint8_t*>(f->qt);
        if (t.blocking) {
            FM_HIP(hipMemcpy(st.dev, c8, cbytes, hipMemcpyHostToDevice));
            FM_HIP(hipMemcpy(st.dev + cbytes, q8, qbytes, hipMemcpyHostToDevice));
        } else if (is_pinned_range(c8, cbytes) && is_pinned_range(q8, qbytes)) {
            FM_HIP(hipMemcpyAsync(st.dev, c8, cbytes, hipMemcpyHostToDevice, s));
            FM_HIP(hipMemcpyAsync(st.dev + cbytes, q8, qbytes, hipMemcpyHostToDevice, s));
        } else {
            if ((rc = src_pinned(st, jpeg_max_coefs(w, h) * 2 + qbytes, s))) return rc;
            memcpy(st.pinned, c8, cbytes);
            memcpy(st.pinned + cbytes, q8, qbytes);
            FM_HIP(hipMemcpyAsync(st.dev, st.pinned, cbytes + qbytes, hipMemcpyHostToDevice, s));
            if ((rc = src_pinned_copied(st, s))) return rc;
        }
        fm_trace_mark(ctx, s, 37);
        if ((rc = fm_jpeg_to_bgr(st.dev, st.bgr, f->info, s))) return rc;
    }
    return enqueue_src_tail(ctx, st.bgr, w, h, t.dst, s);
}

extern "C" int fm_frame_upload_src(fm_ctx* ctx, const struct fm_frame_src* src) {
    FM_CHECK_ARG(ctx && ctx->frame_own && src_ok(src));
    FM_CHECK_ARG(remap_takes(ctx, src->width, src->height));      // (a correction map is for one source size)
    if (src_on_size(ctx, src)) {
        if (src->kind == FM_SRC_BGR) return fm_frame_upload(ctx, src->bgr);
        if (src->kind == FM_SRC_NV12) return fm_frame_upload_nv12(ctx, src->y, src->uv, src->pitch, src->matrix);
        return fm_frame_upload_jpeg(ctx, src->info, src->coef, src->qt);
    }
    return into_current(ctx, [&](const Target& t) { return enqueue_src(ctx, t, src); });
}

extern "C" int fm_frame_upload_ahead_src(fm_ctx* ctx, int k, const struct fm_frame_src* src) {
    FM_CHECK_ARG(ctx && ctx->frame_own2 && k >= 1 && k <= FM_MAX_DET_BATCH && src_ok(src));
    FM_CHECK_ARG(remap_takes(ctx, src->width, src->height));      // (a correction map is for one source size)
    if (src_on_size(ctx, src)) {
        if (src->kind == FM_SRC_BGR) return fm_frame_upload_ahead(ctx, k, src->bgr);
        if (src->kind == FM_SRC_NV12) return fm_frame_upload_ahead_nv12(ctx, k, src->y, src->uv, src->pitch, src->matrix);
        return fm_frame_upload_ahead_jpeg(ctx, k, src->info, src->coef, src->qt);
    }
    return into_ahead(ctx, k, [&](const Target& t) { return enqueue_src(ctx, t, src); });
}

extern "C" int fm_frame_ring_store_src(fm_ctx* ctx, int index, const struct fm_frame_src* src) {
    FM_CHECK_ARG(ctx && index >= 0 && index < ctx->ring_size && src_ok(src));
    FM_CHECK_ARG(remap_takes(ctx, src->width, src->height));      // (a correction map is for one source size)
    if (src_on_size(ctx, src)) {
        if (src->kind == FM_SRC_BGR) return fm_frame_ring_store(ctx, index, src->bgr);
        if (src->kind == FM_SRC_NV12) return fm_frame_ring_store_nv12(ctx, index, src->y, src->uv, src->pitch, src->matrix);
        return fm_frame_ring_store_jpeg(ctx, index, src->info, src->coef, src->qt);
    }
    return into_ring(ctx, index, [&](const Target& t) { return enqueue_src(ctx, t, src); });
}

// ---- planar YCbCr ingest (struct fm_frame_planar: what software decoders hand out, and a YUV4MPEG2 frame).  A frame of
// the configured size goes through ctx->frame_planar[entry] and the kernel of yuv.hip writes the BGR frame; a frame of any
// other size takes the route of fm_frame_*_src with that path's buffers (ctx->frame_src[entry]): yuv.hip writes the
// source-size BGR frame, resize.hip the frame.
static bool planar_ok(const struct fm_frame_planar* f) {
    if (!f || f->width < 1 || f->height < 1 || f->width > FM_SRC_MAX_DIM || f->height > FM_SRC_MAX_DIM) return false;
    int cw = 0, ch = 0;
    if (!fm_yuv_chroma_dims(f->width, f->height, f->chroma, &cw, &ch)) return false;
    if (f->matrix != FM_NV12_BT601 && f->matrix != FM_NV12_BT709) return false;
    if (!f->y || f->pitch_y < f->width) return false;
    return f->chroma == FM_YUV_MONO || (f->u && f->v && f->pitch_c >= cw);
}

// H2D copy of the planes into device staging, the conversion and -- off size -- the resize into t.dst.  On size, planes
// that cannot be copied from where they are go through the slot's BGR-sized staging (it holds every planar layout).
static int enqueue_planar(fm_ctx* ctx, const Target& t, const struct fm_frame_planar* f) {
    hipStream_t s = t.s;
    const int w = f->width, h = f->height;
    int cw = 0, ch = 0;
    fm_yuv_chroma_dims(w, h, f->chroma, &cw, &ch);
    const size_t npx = (size_t)w * h, total = npx + 2 * (size_t)cw * ch;
    const bool on_size = src_on_size(ctx, w, h);
    fm_ctx::SrcStage& st = ctx->frame_src[t.entry];
    uint8_t* stage = nullptr;
    int rc;
    if (on_size) {
        uint8_t*& p = ctx->frame_planar[t.entry];
        if (!p) FM_HIP(hipMalloc(&p, npx * 3));
        stage = p;
    } else {
        if ((rc = src_reserve(st.bgr, st.bgr_cap, npx * 3 + FM_FRAME_SLACK, false, s))) return rc;     // (resize.hip reads 8 bytes at a pixel)
        if ((rc = src_reserve(st.dev, st.dev_cap, total, false, s))) return rc;
        stage = st.dev;
    }
    const Plane planes[3] = {{f->y, (size_t)f->pitch_y, (size_t)w, h}, {f->u, (size_t)f->pitch_c, (size_t)cw, ch}, {f->v, (size_t)f->pitch_c, (size_t)cw, ch}};
    const Staging staging = on_size ? Staging{t.pinned, t.reuse, nullptr} : Staging{nullptr, nullptr, &st};
    if ((rc = copy_planes(stage, planes, ch ? 3 : 1, Direct::SURFACE, staging, s, t.blocking))) return rc;
    fm_trace_mark(ctx, s, 39);                 // (the conversion's share of the caller's 30 .. 31 interval)
    if (on_size) return fm_planar_to_bgr(stage, t.dst, w, h, f->chroma, f->matrix, s);
    if ((rc = fm_planar_to_bgr(stage, st.bgr, w, h, f->chroma, f->matrix, s))) return rc;
    return enqueue_src_tail(ctx, st.bgr, w, h, t.dst, s);
}

extern "C" int fm_frame_upload_planar(fm_ctx* ctx, const struct fm_frame_planar* f) {
    FM_CHECK_ARG(ctx && ctx->frame_own && planar_ok(f));
    FM_CHECK_ARG(remap_takes(ctx, f->width, f->height));      // (a correction map is for one source size)
    return into_current(ctx, [&](const Target& t) { return enqueue_planar(ctx, t, f); });
}

extern "C" int fm_frame_upload_ahead_planar(fm_ctx* ctx, int k, const struct fm_frame_planar* f) {
    FM_CHECK_ARG(ctx && ctx->frame_own2 && k >= 1 && k <= FM_MAX_DET_BATCH && planar_ok(f));
    FM_CHECK_ARG(remap_takes(ctx, f->width, f->height));      // (a correction map is for one source size)
    return into_ahead(ctx, k, [&](const Target& t) { return enqueue_planar(ctx, t, f); });
}

extern "C" int fm_frame_ring_store_planar(fm_ctx* ctx, int index, const struct fm_frame_planar* f) {
    FM_CHECK_ARG(ctx && index >= 0 && index < ctx->ring_size && planar_ok(f));
    FM_CHECK_ARG(remap_takes(ctx, f->width, f->height));      // (a correction map is for one source size)
    return into_ring(ctx, index, [&](const Target& t) { return enqueue_planar(ctx, t, f); });
}

// ---- packed 4:2:2 / RGB ingest (struct fm_frame_packed: what UVC / V4L2 cameras, capture cards, image libraries and
// `appsink` hand out).  A frame of the configured size goes through ctx->frame_packed[entry] and a kernel of packed.hip
// writes the BGR frame; a frame of any other size takes the route of fm_frame_*_src with that path's buffers
// (ctx->frame_src[entry]): packed.hip writes the source-size BGR frame, resize.hip the frame.  Rows that cannot be copied
// from where they lie are packed into ctx->frame_src[entry].pinned for both sizes (the slots' own page-locked buffers hold
// 3 bytes per pixel; BGRx has 4).
static bool packed_ok(const struct fm_frame_packed* f) {
    if (!f || f->width < 1 || f->height < 1 || f->width > FM_SRC_MAX_DIM || f->height > FM_SRC_MAX_DIM) return false;
    const size_t rb = fm_packed_row_bytes(f->width, f->format);
    return rb && fm_packed_matrix_ok(f->matrix) && f->data && f->pitch > 0 && (size_t)f->pitch >= rb;
}

// H2D copy of the rows into device staging, the conversion and -- off size -- the resize into t.dst.
static int enqueue_packed(fm_ctx* ctx, const Target& t, const struct fm_frame_packed* f) {
    hipStream_t s = t.s;
    const int w = f->width, h = f->height;
    const size_t rb = fm_packed_row_bytes(w, f->format), npx = (size_t)w * h;
    const bool on_size = src_on_size(ctx, w, h);
    fm_ctx::SrcStage& st = ctx->frame_src[t.entry];
    uint8_t* stage = nullptr;
    int rc;
    if (on_size) {
        uint8_t*& p = ctx->frame_packed[t.entry];
        if (!p) FM_HIP(hipMalloc(&p, npx * 4));            // (4 * ceil(w / 2) <= 4 w: every layout fits)
        stage = p;
    } else {
        if ((rc = src_reserve(st.bgr, st.bgr_cap, npx * 3 + FM_FRAME_SLACK, false, s))) return rc;     // (resize.hip reads 8 bytes at a pixel)
        if ((rc = src_reserve(st.dev, st.dev_cap, rb * h, false, s))) return rc;
        stage = st.dev;
    }
    const Plane rows = {f->data, (size_t)f->pitch, rb, h};
    if ((rc = copy_planes(stage, &rows, 1, Direct::SURFACE, Staging{nullptr, nullptr, &st}, s, t.blocking))) return rc;
    fm_trace_mark(ctx, s, 48);                 // (the conversion's share of the caller's 30 .. 31 interval)
    if (on_size) return fm_packed_to_bgr(stage, t.dst, w, h, f->format, f->matrix, s);
    if ((rc = fm_packed_to_bgr(stage, st.bgr, w, h, f->format, f->matrix, s))) return rc;
    return enqueue_src_tail(ctx, st.bgr, w, h, t.dst, s);
}

extern "C" int fm_frame_upload_packed(fm_ctx* ctx, const struct fm_frame_packed* f) {
    FM_CHECK_ARG(ctx && ctx->frame_own && packed_ok(f));
    FM_CHECK_ARG(remap_takes(ctx, f->width, f->height));      // (a correction map is for one source size)
    return into_current(ctx, [&](const Target& t) { return enqueue_packed(ctx, t, f); });
}

extern "C" int fm_frame_upload_ahead_packed(fm_ctx* ctx, int k, const struct fm_frame_packed* f) {
    FM_CHECK_ARG(ctx && ctx->frame_own2 && k >= 1 && k <= FM_MAX_DET_BATCH && packed_ok(f));
    FM_CHECK_ARG(remap_takes(ctx, f->width, f->height));      // (a correction map is for one source size)
    return into_ahead(ctx, k, [&](const Target& t) { return enqueue_packed(ctx, t, f); });
}

extern "C" int fm_frame_ring_store_packed(fm_ctx* ctx, int index, const struct fm_frame_packed* f) {
    FM_CHECK_ARG(ctx && index >= 0 && index < ctx->ring_size && packed_ok(f));
    FM_CHECK_ARG(remap_takes(ctx, f->width, f->height));      // (a correction map is for one source size)
    return into_ring(ctx, index, [&](const Target& t) { return enqueue_packed(ctx, t, f); });
}

// ---- Bayer ingest (struct fm_frame_bayer: the raw mosaic of an industrial or embedded camera).  A frame of the
// configured size goes through ctx->frame_bayer[entry] and the kernel of bayer.hip writes the BGR frame; a frame of any
// other size takes the route of fm_frame_*_src with that path's buffers (ctx->frame_src[entry]): bayer.hip writes the
// source-size BGR frame, resize.hip the frame.  Rows that cannot be copied from where they lie are packed into
// ctx->frame_src[entry].pinned for both sizes, as packed frames' are.
static bool bayer_ok(const struct fm_frame_bayer* f) {
    if (!f || f->width < 2 || f->height < 2 || f->width > FM_SRC_MAX_DIM || f->height > FM_SRC_MAX_DIM) return false;
    const int bps = fm_bayer_sample_bytes(f->depth);
    if (!bps || f->pattern < FM_BAYER_RGGB || f->pattern > FM_BAYER_BGGR) return false;
    if (f->method != FM_BAYER_BILINEAR && f->method != FM_BAYER_MHC) return false;
    if (f->black < 0 || f->black >= (1 << f->depth)) return false;
    if (!fm_bayer_gain_ok(f->gain_r) || !fm_bayer_gain_ok(f->gain_g) || !fm_bayer_gain_ok(f->gain_b)) return false;
    return f->data && f->pitch > 0 && (size_t)f->pitch >= (size_t)f->width * bps;
}

// H2D copy of the rows into device staging, the demosaicing and -- off size -- the resize into t.dst.
static int enqueue_bayer(fm_ctx* ctx, const Target& t, const struct fm_frame_bayer* f) {
    hipStream_t s = t.s;
    const int w = f->width, h = f->height;
    const size_t rb = (size_t)w * fm_bayer_sample_bytes(f->depth), npx = (size_t)w * h;
    const bool on_size = src_on_size(ctx, w, h);
    fm_ctx::SrcStage& st = ctx->frame_src[t.entry];
    uint8_t* stage = nullptr;
    int rc;
    if (on_size) {
        uint8_t*& p = ctx->frame_bayer[t.entry];
        if (!p) FM_HIP(hipMalloc(&p, npx * 2));            // (16-bit samples: every depth fits)
        stage = p;
    } else {
        if ((rc = src_reserve(st.bgr, st.bgr_cap, npx * 3 + FM_FRAME_SLACK, false, s))) return rc;     // (resize.hip reads 8 bytes at a pixel)
        if ((rc = src_reserve(st.dev, st.dev_cap, rb * h, false, s))) return rc;
        stage = st.dev;
    }
    const Plane rows = {f->data, (size_t)f->pitch, rb, h};
    if ((rc = copy_planes(stage, &rows, 1, Direct::SURFACE, Staging{nullptr, nullptr, &st}, s, t.blocking))) return rc;
    fm_trace_mark(ctx, s, 49);                 // (the demosaicing's share of the caller's 30 .. 31 interval)
    uint8_t* const out = on_size ? t.dst : st.bgr;
    if ((rc = fm_bayer_to_bgr(stage, out, w, h, f->pattern, f->depth, f->method, f->black, f->gain_r, f->gain_g, f->gain_b, s))) return rc;
    if (on_size) return 0;
    return enqueue_src_tail(ctx, st.bgr, w, h, t.dst, s);
}

extern "C" int fm_frame_upload_bayer(fm_ctx* ctx, const struct fm_frame_bayer* f) {
    FM_CHECK_ARG(ctx && ctx->frame_own && bayer_ok(f));
    FM_CHECK_ARG(remap_takes(ctx, f->width, f->height));      // (a correction map is for one source size)
    return into_current(ctx, [&](const Target& t) { return enqueue_bayer(ctx, t, f); });
}

extern "C" int fm_frame_upload_ahead_bayer(fm_ctx* ctx, int k, const struct fm_frame_bayer* f) {
    FM_CHECK_ARG(ctx && ctx->frame_own2 && k >= 1 && k <= FM_MAX_DET_BATCH && bayer_ok(f));
    FM_CHECK_ARG(remap_takes(ctx, f->width, f->height));      // (a correction map is for one source size)
    return into_ahead(ctx, k, [&](const Target& t) { return enqueue_bayer(ctx, t, f); });
}

extern "C" int fm_frame_ring_store_bayer(fm_ctx* ctx, int index, const struct fm_frame_bayer* f) {
    FM_CHECK_ARG(ctx && index >= 0 && index < ctx->ring_size && bayer_ok(f));
    FM_CHECK_ARG(remap_takes(ctx, f->width, f->height));      // (a correction map is for one source size)
    return into_ring(ctx, index, [&](const Target& t) { return enqueue_bayer(ctx, t, f); });
}

// ---- deep YCbCr ingest (struct fm_frame_deep: 9- to 16-bit samples in 16-bit words, planar as a software decoder or a
// Y4M C420p10 frame holds them, semi-planar as a hardware decoder's P010 / P016 surface): replaces the host narrowing +
// conversion of a Main10 decoder's / a 10-bit Y4M file's frames.  The staging is this family's own for every size,
// ctx->frame_deep[entry].dev and .pinned, grown by src_reserve / src_pinned with their reuse ordering: a frame is up to 6
// bytes per pixel, and the slots' device and page-locked buffers hold 3.  The kernel of deep.hip writes the BGR frame; for
// a frame of another size than the configured one it writes ctx->frame_src[entry].bgr and resize.hip (remap.hip) the
// frame, the route of fm_frame_*_src.
static bool deep_ok(const struct fm_frame_deep* f) {
    if (!f || f->width < 1 || f->height < 1 || f->width > FM_SRC_MAX_DIM || f->height > FM_SRC_MAX_DIM) return false;
    if (!fm_deep_layout_ok(f->width, f->height, f->chroma, f->matrix, f->depth, f->layout)) return false;
    int cw = 0, ch = 0;
    fm_yuv_chroma_dims(f->width, f->height, f->chroma, &cw, &ch);
    if (!f->y || f->pitch_y % 2 || f->pitch_y < 2 * f->width) return false;
    if (f->chroma == FM_YUV_MONO) return true;
    if (f->layout == FM_DEEP_SEMIPLANAR) cw = f->width;        // (U, V pairs: width words a row)
    return f->u && (f->v || f->layout == FM_DEEP_SEMIPLANAR) && f->pitch_c % 2 == 0 && f->pitch_c >= 2 * cw;
}

// H2D copy of the planes into the entry's device staging, the conversion and -- off size -- the resize into t.dst.
static int enqueue_deep(fm_ctx* ctx, const Target& t, const struct fm_frame_deep* f) {
    hipStream_t s = t.s;
    const int w = f->width, h = f->height;
    const bool semi = f->layout == FM_DEEP_SEMIPLANAR;
    int cw = 0, ch = 0;
    fm_yuv_chroma_dims(w, h, f->chroma, &cw, &ch);
    // the chroma planes as byte rows: two (U, V) of 2 cw bytes for planar, one (UV) of 2 w bytes for semi-planar
    const int nplanes = !ch ? 0 : semi ? 1 : 2;
    const size_t yrow = (size_t)w * 2, crow = semi ? yrow : (size_t)cw * 2, npx = (size_t)w * h;
    const bool on_size = src_on_size(ctx, w, h);
    fm_ctx::SrcStage& st = ctx->frame_deep[t.entry];
    fm_ctx::SrcStage& off = ctx->frame_src[t.entry];
    int rc;
    if (!on_size && (rc = src_reserve(off.bgr, off.bgr_cap, npx * 3 + FM_FRAME_SLACK, false, s))) return rc;     // (resize.hip reads 8 bytes at a pixel)
    if ((rc = src_reserve(st.dev, st.dev_cap, yrow * h + nplanes * crow * ch, false, s))) return rc;
    const Plane planes[3] = {{f->y, (size_t)f->pitch_y, yrow, h}, {f->u, (size_t)f->pitch_c, crow, ch}, {f->v, (size_t)f->pitch_c, crow, ch}};
    if ((rc = copy_planes(st.dev, planes, 1 + nplanes, Direct::SURFACE, Staging{nullptr, nullptr, &st}, s, t.blocking))) return rc;
    fm_trace_mark(ctx, s, 58);                 // (the conversion's share of the caller's 30 .. 31 interval)
    uint8_t* const out = on_size ? t.dst : off.bgr;
    if ((rc = fm_deep_to_bgr(st.dev, out, w, h, f->chroma, f->matrix, f->depth, f->layout, s))) return rc;
    if (on_size) return 0;
    return enqueue_src_tail(ctx, off.bgr, w, h, t.dst, s);
}

extern "C" int fm_frame_upload_deep(fm_ctx* ctx, const struct fm_frame_deep* f) {
    FM_CHECK_ARG(ctx && ctx->frame_own && deep_ok(f));
    FM_CHECK_ARG(remap_takes(ctx, f->width, f->height));      // (a correction map is for one source size)
    return into_current(ctx, [&](const Target& t) { return enqueue_deep(ctx, t, f); });
}

extern "C" int fm_frame_upload_ahead_deep(fm_ctx* ctx, int k, const struct fm_frame_deep* f) {
    FM_CHECK_ARG(ctx && ctx->frame_own2 && k >= 1 && k <= FM_MAX_DET_BATCH && deep_ok(f));
    FM_CHECK_ARG(remap_takes(ctx, f->width, f->height));      // (a correction map is for one source size)
    return into_ahead(ctx, k, [&](const Target& t) { return enqueue_deep(ctx, t, f); });
}

extern "C" int fm_frame_ring_store_deep(fm_ctx* ctx, int index, const struct fm_frame_deep* f) {
    FM_CHECK_ARG(ctx && index >= 0 && index < ctx->ring_size && deep_ok(f));
    FM_CHECK_ARG(remap_takes(ctx, f->width, f->height));      // (a correction map is for one source size)
    return into_ring(ctx, index, [&](const Target& t) { return enqueue_deep(ctx, t, f); });
}

// ---- frames that lie in device memory already (struct fm_frame_device: a decoder's surface, a torch / CuPy tensor, another
// model's output).  Same protocols, the same remap_takes check -- and no copy: a kernel of devsrc.hip reads the caller's
// memory and writes the BGR frame, straight into t.dst on size, into ctx->frame_src[entry].bgr (and enqueue_src_tail from
// there) off size.  What is new here is that the memory is somebody else's: every plane is checked against what the
// runtime knows about its pointer before anything is enqueued, the slot's stream is ordered behind the producer's, and a
// look-ahead call leaves an event behind the conversion kernel -- the last reader of the caller's memory -- for
// fm_frame_device_done.

// `f` passes fm_frame_device_check and every plane of it is device memory of the context's device, its whole extent --
// where the runtime knows the allocation -- inside that allocation.  Nothing is enqueued.
static int device_ok(const fm_ctx* ctx, const struct fm_frame_device* f) {
    int rc = fm_frame_device_check(f);
    if (rc) return rc;
    const size_t rb = fm_dev_row_bytes(f);
    for (int p = 0; p < fm_dev_planes(f->layout); ++p) {
        const uint8_t* const base = static_cast<const uint8_t*>(f->plane[p]);
        const size_t extent = (size_t)f->pitch[p] * (fm_dev_plane_rows(f, p) - 1) + rb;
        hipPointerAttribute_t attr{};
        const hipError_t e = hipPointerGetAttributes(&attr, base);
        if (e != hipSuccess) (void)hipGetLastError();          // (a pointer the runtime has never seen is no sticky error)
        if (e != hipSuccess || attr.type != hipMemoryTypeDevice || attr.isManaged || attr.device != ctx->device) {
            fm_set_error("%s:%d bad argument: plane %d of the device frame (%p) is not device memory of device %d -- host, page-locked, "
                         "managed and other-device frames go through the host calls: fm_frame_upload, _nv12, _planar, _packed, _bayer, "
                         "_deep or _src", __FILE__, __LINE__, p, (const void*)base, ctx->device);
            return FM_ERR_ARG;
        }
        hipDeviceptr_t abase = nullptr;
        size_t asize = 0;
        if (hipMemGetAddressRange(&abase, &asize, (hipDeviceptr_t)base) == hipSuccess) {
            const uint8_t* const a0 = static_cast<const uint8_t*>(abase);
            if (base < a0 || extent > asize || (size_t)(base - a0) > asize - extent) {
                fm_set_error("%s:%d bad argument: plane %d of the device frame (%zu bytes from %p) runs past its allocation (%zu bytes from %p)",
                             __FILE__, __LINE__, p, extent, (const void*)base, asize, (const void*)a0);
                return FM_ERR_ARG;
            }
        } else {
            (void)hipGetLastError();                           // (virtual-memory allocators: the attributes alone decide)
        }
    }
    return 0;
}

// a wait for `ev` on `s` -- unless the host already sees it complete: a barrier packet that is not enqueued does not
// park on a shared hardware queue (the rule of fm_frame_promote_next and acquire_slots)
static int wait_unless_complete(hipStream_t s, hipEvent_t ev) {
    if (hipEventQuery(ev) != hipSuccess) {
        (void)hipGetLastError();                               // (hipErrorNotReady is not an error)
        FM_HIP(hipStreamWaitEvent(s, ev, 0));
    }
    return 0;
}

// The conversion of the device frame `f` (device_ok) and -- off size -- the resize into t.dst, behind the producer's
// stream; `consumed`, when given, is recorded behind the conversion kernel.
static int enqueue_device(fm_ctx* ctx, const Target& t, const struct fm_frame_device* f, hipEvent_t consumed) {
    hipStream_t s = t.s;
    const int w = f->width, h = f->height;
    const bool on_size = src_on_size(ctx, w, h);
    fm_ctx::SrcStage& st = ctx->frame_src[t.entry];
    int rc;
    if (!on_size && (rc = src_reserve(st.bgr, st.bgr_cap, (size_t)w * h * 3 + FM_FRAME_SLACK, false, s))) return rc;   // (resize.hip reads 8 bytes at a pixel)
    if (!(f->flags & FM_DEV_READY)) {
        hipEvent_t& in = ctx->ev_dev_in[t.entry];
        if (!in) FM_HIP(hipEventCreateWithFlags(&in, hipEventDisableTiming));
        FM_HIP(hipEventRecord(in, static_cast<hipStream_t>(f->stream)));
        if ((rc = wait_unless_complete(s, in))) return rc;
    }
    fm_trace_mark(ctx, s, 59);                 // (the conversion's share of the caller's 30 .. 31 interval)
    if ((rc = fm_device_to_bgr(f, on_size ? t.dst : st.bgr, s))) return rc;
    fm_trace_mark(ctx, s, 60);                 // (59 .. 60: the kernel without the event record behind it)
    if (consumed) FM_HIP(hipEventRecord(consumed, s));
    return on_size ? 0 : enqueue_src_tail(ctx, st.bgr, w, h, t.dst, s);
}

extern "C" int fm_frame_upload_device(fm_ctx* ctx, const struct fm_frame_device* f) {
    FM_CHECK_ARG(ctx && ctx->frame_own && f);
    int rc = device_ok(ctx, f);
    if (rc) return rc;
    FM_CHECK_ARG(remap_takes(ctx, f->width, f->height));      // (a correction map is for one source size)
    return into_current(ctx, [&](const Target& t) { return enqueue_device(ctx, t, f, nullptr); });
}

extern "C" int fm_frame_upload_ahead_device(fm_ctx* ctx, int k, const struct fm_frame_device* f, uint64_t* ticket) {
    FM_CHECK_ARG(ctx && ctx->frame_own2 && k >= 1 && k <= FM_MAX_DET_BATCH && f);
    int rc = device_ok(ctx, f);
    if (rc) return rc;
    FM_CHECK_ARG(remap_takes(ctx, f->width, f->height));      // (a correction map is for one source size)
    // the ticket's place in the ring: whoever held it before is consumed before it is given away
    const uint64_t tk = ctx->dev_ticket_next;
    fm_ctx::DevTicket& place = ctx->dev_ticket[tk % FM_DEV_TICKETS];
    if (!place.ev) FM_HIP(hipEventCreateWithFlags(&place.ev, hipEventDisableTiming));
    else if (place.ticket) FM_HIP(hipEventSynchronize(place.ev));
    return into_ahead(ctx, k, [&](const Target& t) {
        int rc_e = enqueue_device(ctx, t, f, place.ev);
        if (rc_e) return rc_e;
        place.ticket = tk;                  // booked once the kernel that records the ticket's event is enqueued
        ctx->dev_ticket_next = tk + 1;
        if (ticket) *ticket = tk;
        return 0;
    });
}

extern "C" int fm_frame_ring_store_device(fm_ctx* ctx, int index, const struct fm_frame_device* f) {
    FM_CHECK_ARG(ctx && index >= 0 && index < ctx->ring_size && f);
    int rc = device_ok(ctx, f);
    if (rc) return rc;
    FM_CHECK_ARG(remap_takes(ctx, f->width, f->height));      // (a correction map is for one source size)
    return into_ring(ctx, index, [&](const Target& t) { return enqueue_device(ctx, t, f, nullptr); });
}

extern "C" int fm_frame_device_done(fm_ctx* ctx, uint64_t ticket, int wait) {
    if (!ctx || !ticket || ticket >= ctx->dev_ticket_next) {
        fm_set_error("%s:%d bad argument: no such ticket", __FILE__, __LINE__);
        return FM_ERR_ARG;
    }
    const fm_ctx::DevTicket& place = ctx->dev_ticket[ticket % FM_DEV_TICKETS];
    if (place.ticket != ticket) return 1;                      // (older than the ring: consumed before its place was given away)
    if (wait) {
        FM_HIP(hipEventSynchronize(place.ev));
        return 1;
    }
    const hipError_t e = hipEventQuery(place.ev);
    if (e == hipSuccess) return 1;
    (void)hipGetLastError();
    if (e == hipErrorNotReady) return 0;
    FM_HIP(e);
    return 0;
}

void fm_frame_dev_free(fm_ctx* ctx) {
    for (fm_ctx::DevTicket& place : ctx->dev_ticket) {
        if (place.ev) {
            (void)hipEventSynchronize(place.ev);
            (void)hipEventDestroy(place.ev);
        }
        place = fm_ctx::DevTicket{};
    }
    for (hipEvent_t& e : ctx->ev_dev_in) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}
