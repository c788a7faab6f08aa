// Internal definitions shared by the libfastmot_hip.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/fastmot_hip.h"
#ifdef FM_DIAG
#include "../../include/fastmot_hip_diag.h"
#endif

#define FM_ERR_HIP (-1)
#define FM_ERR_ARG (-2)
#define FM_ERR_STATE (-3)

void fm_set_error(const char* fmt, ...);

#define FM_HIP(call)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            fm_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            return FM_ERR_HIP;                                                              \
        }                                                                                   \
    } while (0)

#define FM_CHECK_ARG(cond)                                                     \
    do {                                                                       \
        if (!(cond)) {                                                         \
            fm_set_error("%s:%d bad argument: %s", __FILE__, __LINE__, #cond); \
            return FM_ERR_ARG;                                                 \
        }                                                                      \
    } while (0)

// Growable device buffer with a pinned host mirror (HostDeviceMem of utils/inference.py:7-36).
// batches up to this many tracks exchange their (tiny) kernel inputs / outputs through pinned,
// device-mapped host memory instead of blit copies
bool fm_lap_host(const double* cost, int nr, int nc, long rs, long cs, int32_t* col4row_out);
int fm_greedy_host(const double* cost, int nr, int nc, double max_cost, int32_t* m_rows, int32_t* m_cols);
#define FM_ZERO_COPY_TRACKS (ctx->opt_zero_copy_tracks)

struct DevBuf {
    void* d = nullptr;
    void* h = nullptr;   // pinned
    size_t cap = 0;
    bool pinned_mirror = true;
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        size_t ncap = cap ? cap : 4096;
        while (ncap < bytes) ncap *= 2;
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        d = h = nullptr;
        cap = 0;
        FM_HIP(hipMalloc(&d, ncap));
        if (pinned_mirror) FM_HIP(hipHostMalloc(&h, ncap, hipHostMallocDefault));
        cap = ncap;
        return 0;
    }
    void release() {
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        d = h = nullptr;
        cap = 0;
    }
    template <typename T> T* dev() { return reinterpret_cast<T*>(d); }
    template <typename T> T* host() { return reinterpret_cast<T*>(h); }
};

struct KFConst {           // constants derived from fm_kf_params, passed by value to kernels
    double F_pos_self;     // vel_coupling * dt
    double F_pos_other;    // (1 - vel_coupling) * dt
    double F_vel;          // 0.5^(dt / half_life)
    double q_pp, q_pv, q_vv;   // dt^4/4, dt^3/2, dt^2
    double std_factor_acc, std_offset_acc;
    double fac_det[2], fac_klt[2], min_det[2], min_klt[2];
    double init_pos_weight, init_vel_weight;
};

struct NetState;     // conv engine (net.hip)
struct DetState;     // detector pre/post (detect.hip)
struct ExtState;     // extractor pre (extract.hip)
struct FlowState;    // KLT (flow.hip)
struct EncState;     // JPEG output path (jpegenc.hip)
struct OvlState;     // overlays on the device frame (overlay.hip)
struct YuvState;     // I420 export (yuv.hip)
struct SsdState;     // SSD detector pre/post (ssd.hip)
struct GalleryState; // cross-stream ReID-gallery all-gather over RCCL (gallery.hip)
constexpr int FM_GALLERY_CHANNELS = 2;

struct fm_ctx {
    int device = 0;
    // tunables (fm_ctx_set_option; initial values from the environment)
    int opt_zero_copy_tracks = 2048;   // FASTMOT_ZERO_COPY: 0 = always blit copies
    int opt_host_lap_elems = 262144;   // FASTMOT_HOST_LAP: cost matrices up to this size use lap_host.hip (measured: the
                                       // host solver is ~5x faster at every size up to 400 x 400, profiles/r02_lap_crossover.txt)
    int opt_use_graphs = 1;            // FASTMOT_GRAPHS: 0 = launch network layers one by one (no hipGraph)
    int opt_fused_input = 1;           // "fused_input" / FASTMOT_FUSED_INPUT: the networks' stem convolutions compute their input pixels from the
                                       // frame themselves (pixel_source.h); 0 = front-end kernel + input tensor (tests compare the two, A/B)
    int opt_net_timing = 0;            // "net_timing" = N: HIP events around the detector network on every N-th pass (fm_detect_net_ms); 0 = never
    int opt_nms_general = 0;           // "nms_path" = 1: always the three-kernel sort / bit matrix / scan path (tests, A/B)
    int opt_dfl_decode_form = 0;       // "dfl_decode_form": 0 = 16 lanes per cell (dfl_decode_kernel), 1 = one thread per cell (A/B, dfl_decode.h)
    // front-ahead (detect.hip detect_pass): the leading layers of a single-frame pass run on another stream beside the
    // previous pass's tail
    int opt_det_front_ahead = 1;       // "det_front_ahead": 0 off, 1 when a pass is still in flight on the detector stream, 2 always (tests)
    int opt_det_front_layers = -1;     // "det_front_layers": 0 off, k the first k layers, -1 the rule (net.hip fm_net_front_prepare)
    int opt_det_front_stream = 0;      // "det_front_stream": the stream that carries the front: 0 s_up, 1 s_ext
    bool det_flush_deferred = false;   // a look-ahead upload left the pending post-processing to the pass that follows it
    int opt_lk_variant = 0;            // "lk_variant": diagnostic variants of the LK kernel (lk_core.h lk_diag_kernel)
    void* predict_worker = nullptr;    // native KLT + Kalman worker thread of this context (flow_estimate.hip)
    hipStream_t s_main = nullptr;   // tracker kernels
    hipStream_t s_det = nullptr;    // detector network
    hipStream_t s_up = nullptr;     // detector post-processing (sort, NMS, D2H), off the detector stream (detect.hip flush_post)
    hipStream_t s_ext = nullptr;    // ReID network
    hipStream_t s_ext_x[FM_MAX_EXTRA_EXTRACTORS] = {};   // streams of the extra ReID instances
    hipEvent_t ev_ext_in = nullptr, ev_ext_x_done[FM_MAX_EXTRA_EXTRACTORS] = {};
    hipStream_t s_flow = nullptr;   // KLT
    hipStream_t s_flow2 = nullptr;  // KLT: pyramid of the new frame (independent of the keypoint preparation on s_flow)
    hipEvent_t ev_pyr = nullptr;    // completion of that pyramid; s_flow waits on it before its first reader (LK)
    bool pyr_pending = false;
    hipEvent_t ev_prep = nullptr, ev_bg = nullptr;   // fork / join of the background-keypoint branch of fm_flow_prepare
    hipEvent_t ev_feat = nullptr;   // last reader of ctx->emb on s_main (fm_feat_update); s_ext waits on it
    hipEvent_t ev_ext_net = nullptr;   // the ReID network's last launch of a batch on s_ext (embeddings complete on the device):
                                       // fm_assoc_prepare2 orders the pairwise kernel behind it without the host
    hipEvent_t ev_ext_done = nullptr;  // embeddings exported to page-locked memory (fm_extract_sync waits for this, not for the stream)
    hipEvent_t ev_pair = nullptr;      // pairwise kernel of fm_assoc_prepare / fm_assoc_prepare2 done (its pinned mirror is complete)
    bool ext_net_recorded = false;     // ev_ext_net belongs to the batch ctx->emb holds
    size_t as_in_bytes = 0;
    bool as_in_device = true;          // as_in's device copy holds this frame's inputs (not for an early launch: fm_assoc_stage refuses)
    bool as_mirror = false;            // the pairwise terms of this frame also lie in as_pair's pinned mirror (host cascade)

    // ---- device-resident track table
    int slot_cap = 0;
    double* mean = nullptr;      // [cap][8]
    double* cov = nullptr;       // [cap][64]
    int feat_dim = 512;
    float* feat_sum = nullptr;   // [cap][dim]
    float* feat_avg = nullptr;   // [cap][dim]
    int32_t* feat_cnt = nullptr; // [cap]
    KFConst kf{};
    bool kf_set = false;
    double frame_rect[4] = {0, 0, 0, 0};

    // ---- per-frame embeddings on the device [n][dim] f32
    float* emb = nullptr;
    float* emb_host = nullptr;   // page-locked mirror [emb_cap][dim]: the ReID head writes a row to both (no export launch, round 6)
    int emb_cap = 0;
    int emb_n = 0;

    // ---- association scratch
    int as_nT = 0, as_nD = 0, as_metric = 0;
    size_t as_off[6] = {0, 0, 0, 0, 0, 0};   // slots|trk_tlbr|trk_label|det_tlbr|det_label|det_occ
    DevBuf as_in;       // packed inputs of fm_assoc_prepare
    DevBuf as_pair;     // feat | maha | iou  [3][nT][nD] f64
    DevBuf as_stage_in; // rows, cols, labels
    DevBuf as_cost;     // [nr][nc] f64
    DevBuf as_work;     // LAP work arrays
    DevBuf as_out;      // matches
    DevBuf io0, io1;    // generic staging (kalman etc.)
    DevBuf occ_in, occ_out;   // fm_find_occluded (own buffers: may run concurrently with the Kalman thread)
    DevBuf feat_in;     // fm_feat_update staging (own buffer: the call returns without synchronising)

    // ---- frames (BGR u8) resident on the device
    int frame_w = 0, frame_h = 0, ring_size = 0;
    uint8_t* frame_cur = nullptr;          // points into frame_own or the ring
    uint8_t* frame_own = nullptr;          // upload slot of the current frame
    uint8_t* frame_own2 = nullptr;         // second upload slot (prefetched next frame); the two swap roles
    uint8_t* frame_next = nullptr;         // frame the detector was prefetched on (fm_frame_*_next)
    uint8_t* frame_pinned2 = nullptr;
    hipEvent_t ev_next_upload = nullptr;   // completion of the prefetched frame's H2D copy (enqueued on the ReID stream)
    // look-ahead slots k = 2..FM_MAX_DET_BATCH (fm_frame_*_ahead; slot 1 is frame_next / frame_own2 / frame_pinned2 /
    // ev_next_upload): the frame of slot k, and upload slot k with its staging buffer and copy event (allocated on first use)
    uint8_t* frame_ahead[FM_MAX_DET_BATCH + 1] = {};
    uint8_t* frame_up[FM_MAX_DET_BATCH + 1] = {};
    uint8_t* frame_up_pinned[FM_MAX_DET_BATCH + 1] = {};
    hipEvent_t ev_up[FM_MAX_DET_BATCH + 1] = {};
    uint8_t* frame_ring = nullptr;
    uint8_t* frame_pinned = nullptr;

    DetState* det = nullptr;
    SsdState* ssd = nullptr;             // created by fm_ssd_configure
    ExtState* ext = nullptr;
    NetState* det_net = nullptr;
    NetState* ext_net = nullptr;
    NetState* ext_net_x[FM_MAX_EXTRA_EXTRACTORS] = {};   // FM_NET_EXTRACTOR_B + i: further parts of a split batch
    FlowState* flow = nullptr;
    EncState* enc = nullptr;             // created by the first fm_frame_encode_jpeg / fm_jpeg_encode_bgr
    OvlState* ovl = nullptr;             // created by the first fm_frame_render_overlay
    YuvState* yuv = nullptr;             // created by the first fm_frame_export_i420 / fm_i420_from_bgr
    GalleryState* gallery[2] = {nullptr, nullptr};   // [FM_GALLERY_CHANNELS]

    // ---- event trace of the pipeline (fm_trace_start / fm_trace_read, scripts/trace_pipeline.py); empty = off
    std::vector<hipEvent_t> trace_ev;
    std::vector<int> trace_tag;
    std::atomic<int> trace_n{0};
    std::atomic<bool> trace_on{false};   // set once the two vectors are in place, cleared before they are taken away
    std::atomic<int> trace_busy{0};      // fm_trace_mark calls in flight (the prediction worker marks too): fm_trace_read
                                         // takes the vectors away only when none is left
    hipEvent_t trace_base = nullptr;

    // ---- device staging of NV12 frames (1.5 bytes per pixel; csrc/nv12.hip converts out of it), allocated on first NV12 use:
    // [0] fm_frame_upload_nv12, [k] look-ahead slot k, [FM_MAX_DET_BATCH + 1] fm_frame_ring_store_nv12.  Unlike the
    // slots' BGR buffers these stay where they are at a promote: copy and kernel of a slot share one stream.
    uint8_t* frame_nv12[FM_MAX_DET_BATCH + 2] = {};
    // ... and of planar frames of the configured size (fm_frame_*_planar; csrc/yuv.hip converts out of it), entries and
    // rules as frame_nv12's; sized for the largest layout, 4:4:4.  (Planar frames of another size use frame_src below.)
    uint8_t* frame_planar[FM_MAX_DET_BATCH + 2] = {};
    // ... and of packed 4:2:2 / RGB frames of the configured size (fm_frame_*_packed; csrc/packed.hip converts out of
    // it), entries and rules as frame_nv12's; sized for the widest layout, 4 bytes per pixel.  Their page-locked staging
    // is frame_src[entry].pinned with its event: the slots' BGR-sized buffers are too small for 4 bytes per pixel.
    uint8_t* frame_packed[FM_MAX_DET_BATCH + 2] = {};
    // ... and of Bayer mosaics of the configured size (fm_frame_*_bayer; csrc/bayer.hip demosaics out of it), entries
    // and rules as frame_packed's, page-locked staging included; sized for 16-bit samples, 2 bytes per pixel.
    uint8_t* frame_bayer[FM_MAX_DET_BATCH + 2] = {};

    // ---- device staging of entropy-decoded JPEG frames (coefficients, quantisation tables and the sample planes
    // csrc/jpeg.hip makes of them), entries as frame_nv12's, allocated on first JPEG use for the largest layout of the
    // frame size; frame_jpeg_pinned: page-locked host staging for coefficient buffers that are not in fm_host_alloc memory
    uint8_t* frame_jpeg[FM_MAX_DET_BATCH + 2] = {};
    uint8_t* frame_jpeg_pinned[FM_MAX_DET_BATCH + 2] = {};
    hipEvent_t ev_jpeg[FM_MAX_DET_BATCH + 2] = {};      // [k]: behind the last H2D copy out of frame_jpeg_pinned[k]

    // ---- frames that arrive at another size than frame_w x frame_h (fm_frame_*_src; csrc/resize.hip resizes out of
    // `bgr`), entries as frame_nv12's.  Everything is sized by the SOURCE, allocated on first use, regrown for a larger
    // source and separate from the staging above; like that staging it stays where it is at a promote.
    struct SrcStage {
        uint8_t* bgr = nullptr;      // the source-resolution BGR frame on the device (+ FM_FRAME_SLACK)
        uint8_t* dev = nullptr;      // NV12 planes / JPEG coefficients, tables and sample planes on the device
        uint8_t* pinned = nullptr;   // page-locked host staging for sources that are not in fm_host_alloc memory
        size_t bgr_cap = 0, dev_cap = 0, pinned_cap = 0;
        hipEvent_t ev = nullptr;     // behind the last H2D copy out of `pinned`
    };
    SrcStage frame_src[FM_MAX_DET_BATCH + 2];
    // ... and the staging of deep YCbCr frames of every size (fm_frame_*_deep; csrc/deep.hip converts out of `dev`),
    // entries as frame_nv12's: `dev` and `pinned` grow to the frame's bytes -- up to 6 per pixel, which the slots'
    // BGR-sized buffers do not hold -- by frame_src's rules; `bgr` stays unused (an off-size frame's BGR form is
    // frame_src[entry].bgr).  Freed by fm_frame_configure and fm_ctx_destroy (fm_frame_staging_free).
    SrcStage frame_deep[FM_MAX_DET_BATCH + 2];

    // ---- frames that lie in device memory already (fm_frame_*_device; csrc/devsrc.hip converts from where they lie): no
    // staging.  ev_dev_in[entry], entries as frame_nv12's: recorded on the producer's stream, waited for by the slot's.
    // dev_ticket[t % FM_DEV_TICKETS]: the event behind the conversion kernel of look-ahead ticket t (fm_frame_device_done);
    // events are created on first use and destroyed by fm_ctx_destroy (fm_frame_dev_free).
    hipEvent_t ev_dev_in[FM_MAX_DET_BATCH + 2] = {};
    struct DevTicket {
        uint64_t ticket = 0;         // 0: the place has never been used
        hipEvent_t ev = nullptr;
    };
    DevTicket dev_ticket[FM_DEV_TICKETS];
    uint64_t dev_ticket_next = 1;

    // ---- the correction map of the described-source calls (fm_frame_remap_set; csrc/remap.hip gathers through it in
    // place of the resize): [frame_h][frame_w][2] int32 on the device, null = none.  Dropped by fm_frame_remap_clear,
    // fm_frame_configure and fm_ctx_destroy.
    int32_t* remap_xy = nullptr;
    int remap_sw = 0, remap_sh = 0;        // the one source size the map is for
    uint32_t remap_border = 0;             // b | g << 8 | r << 16
};

// one timed event on stream `s` (no-op unless a trace is running; both host threads of a context may call it)
inline void fm_trace_mark(fm_ctx* ctx, hipStream_t s, int tag) {
    if (!ctx->trace_on.load(std::memory_order_acquire)) return;
    ctx->trace_busy.fetch_add(1);                               // (seq_cst on both sides of the handshake)
    if (ctx->trace_on.load()) {       // (re-checked: a reader that disarmed waits for busy == 0)
        const int i = ctx->trace_n.fetch_add(1);
        if (i < (int)ctx->trace_ev.size()) {
            ctx->trace_tag[i] = tag;
            (void)hipEventRecord(ctx->trace_ev[i], s);
        }
    }
    ctx->trace_busy.fetch_sub(1);
}

int fm_ensure_slots(fm_ctx* ctx, int max_slot_plus_1);
int fm_nv12_to_bgr(const uint8_t* nv12, uint8_t* bgr, int w, int h, int matrix, hipStream_t s);   // nv12.hip
// nv12.hip: the same for planes that lie anywhere in device memory, rows sy / suv bytes apart
int fm_nv12_planes_to_bgr(const uint8_t* y, const uint8_t* uv, long long sy, long long suv, uint8_t* bgr, int w, int h, int matrix,
                          hipStream_t s);
// width x height of the U and V planes of a w x h frame (0 x 0 for FM_YUV_MONO); false for an unknown `chroma`
inline bool fm_yuv_chroma_dims(int w, int h, int chroma, int* cw, int* ch) {
    switch (chroma) {
    case FM_YUV_420: *cw = (w + 1) / 2, *ch = (h + 1) / 2; return true;
    case FM_YUV_422: *cw = (w + 1) / 2, *ch = h; return true;
    case FM_YUV_444: *cw = w, *ch = h; return true;
    case FM_YUV_MONO: *cw = *ch = 0; return true;
    }
    return false;
}
int fm_planar_to_bgr(const uint8_t* planes, uint8_t* bgr, int w, int h, int chroma, int matrix, hipStream_t s);   // yuv.hip
// bytes of a row of w pixels in the packed layout `format` (FM_PACKED_*); 0 for an unknown format
inline size_t fm_packed_row_bytes(int w, int format) {
    if (format < FM_PACKED_RGB || format > FM_PACKED_YVYU) return 0;
    if (format >= FM_PACKED_YUY2) return 4 * (size_t)((w + 1) / 2);
    return (size_t)w * (format <= FM_PACKED_BGR ? 3 : 4);
}
inline bool fm_packed_matrix_ok(int matrix) {
    return matrix == FM_PACKED_BT601 || matrix == FM_PACKED_BT709 || matrix == FM_PACKED_BT601_FULL || matrix == FM_PACKED_BT709_FULL;
}
int fm_packed_to_bgr(const uint8_t* src, uint8_t* bgr, int w, int h, int format, int matrix, hipStream_t s);   // packed.hip
// hwc.hip: h rows of w 3- or 4-byte pixels (format: FM_PACKED_RGB .. FM_PACKED_XBGR), `pitch` bytes apart, anywhere in
// device memory -> w * h * 3 BGR bytes at `bgr`, on `s`
int fm_hwc_to_bgr(const uint8_t* src, long long pitch, uint8_t* bgr, int w, int h, int format, hipStream_t s);
// bytes of one Bayer sample of `depth` bits (FM_BAYER frames); 0 for an unknown depth
inline int fm_bayer_sample_bytes(int depth) {
    return depth == 8 ? 1 : depth == 10 || depth == 12 || depth == 14 || depth == 16 ? 2 : 0;
}
inline bool fm_bayer_gain_ok(int gain) { return gain >= 1 && gain <= 4096; }
int fm_bayer_to_bgr(const uint8_t* src, uint8_t* bgr, int w, int h, int pattern, int depth, int method, int black, int gain_r, int gain_g,
                    int gain_b, hipStream_t s);                                                   // bayer.hip
// a deep frame's description apart from its pointers and pitches (struct fm_frame_deep) is one csrc/deep.hip converts
inline bool fm_deep_layout_ok(int w, int h, int chroma, int matrix, int depth, int layout) {
    int cw = 0, ch = 0;
    if (depth < 9 || depth > 16 || matrix < FM_DEEP_BT601 || matrix > FM_DEEP_BT2020 || !fm_yuv_chroma_dims(w, h, chroma, &cw, &ch)) return false;
    if (layout == FM_DEEP_SEMIPLANAR) return chroma == FM_YUV_420 && w % 2 == 0 && h % 2 == 0;
    return layout == FM_DEEP_PLANAR;
}
int fm_deep_to_bgr(const uint8_t* planes, uint8_t* bgr, int w, int h, int chroma, int matrix, int depth, int layout,
                   hipStream_t s);                                                                // deep.hip
// devsrc.hip: the device frame `f` (checked by fm_frame_device_check) -> f->width * f->height * 3 BGR bytes at `bgr`, on `s`
int fm_device_to_bgr(const struct fm_frame_device* f, uint8_t* bgr, hipStream_t s);
// bytes of an element of `dtype` (FM_DEV_*); 0 for an unknown one
inline int fm_dev_elem_bytes(int dtype) { return dtype == FM_DEV_U8 ? 1 : dtype == FM_DEV_F16 ? 2 : dtype == FM_DEV_F32 ? 4 : 0; }
// planes a layout uses, and the rows and row bytes of plane `p` of the checked frame `f`
inline int fm_dev_planes(int layout) { return layout == FM_DEV_HWC ? 1 : layout == FM_DEV_CHW ? 3 : layout == FM_DEV_NV12 ? 2 : 0; }
inline int fm_dev_plane_rows(const struct fm_frame_device* f, int p) { return f->layout == FM_DEV_NV12 && p == 1 ? f->height / 2 : f->height; }
inline size_t fm_dev_row_bytes(const struct fm_frame_device* f) {
    if (f->layout == FM_DEV_HWC) return (size_t)f->width * (f->format <= FM_PACKED_BGR ? 3 : 4);
    return (size_t)f->width * fm_dev_elem_bytes(f->dtype);
}
void fm_ssd_free(fm_ctx* ctx);                                                                    // ssd.hip
void fm_yuv_free(fm_ctx* ctx);                                                                    // yuv.hip
int fm_resize_bgr(const uint8_t* src, int sw, int sh, uint8_t* dst, int dw, int dh, hipStream_t s);   // resize.hip
// remap.hip: `src` through the device map `xy` ([dh][dw][2] int32, remap_pixel.h); border = b | g << 8 | r << 16
int fm_remap_bgr(const uint8_t* src, int sw, int sh, const int32_t* xy, uint8_t* dst, int dw, int dh, uint32_t border, hipStream_t s);
// frames.hip.  Look-ahead slot k, the frame the step k steps ahead receives: slot 1 is the fields of the next-frame
// prefetch, slots 2.. those of the arrays (fm_ctx above) -- its frame, and its upload buffer with the event behind the
// last upload into it
inline uint8_t*& fm_ahead_frame(fm_ctx* ctx, int k) { return k == 1 ? ctx->frame_next : ctx->frame_ahead[k]; }
inline uint8_t*& fm_ahead_buf(fm_ctx* ctx, int k) { return k == 1 ? ctx->frame_own2 : ctx->frame_up[k]; }
inline hipEvent_t& fm_ahead_event(fm_ctx* ctx, int k) { return k == 1 ? ctx->ev_next_upload : ctx->ev_up[k]; }
bool fm_host_is_pinned(const void* p, size_t bytes);      // frames.hip: inside a buffer from fm_host_alloc
// frames.hip: frees every format's staging, the off-size sources' and the correction map (no sync: the caller's) ...
void fm_frame_staging_free(fm_ctx* ctx);
void fm_frame_dev_free(fm_ctx* ctx);     // ... and destroys the device frames' events, waiting for the tickets' (fm_ctx_destroy)
hipStream_t fm_det_front_stream(fm_ctx* ctx);   // detect.hip: the stream that carried a detector front last (nullptr: none)
bool fm_det_defers_flush(fm_ctx* ctx);          // detect.hip: front-ahead on s_up -- the pending post-processing waits for the next pass's front
int fm_det_flush_post(fm_ctx* ctx);      // detect.hip: enqueues the pending pass's post-processing; nothing without a detector
int fm_jpeg_to_bgr(const uint8_t* stage, uint8_t* bgr, const struct fm_jpeg_info* info, hipStream_t s);   // jpeg.hip
// fm_jpeg_info's description of a width x height frame with ncomp 1 or 3 and luma sampling hsamp0 x vsamp0 (jpeg_host.hip)
int fm_jpeg_layout(int width, int height, int ncomp, int hsamp0, int vsamp0, struct fm_jpeg_info* out);
size_t fm_jpeg_sample_offset(long long coef_count);                                               // jpeg.hip
void fm_ext_invalidate_export(fm_ctx* ctx);
void fm_predict_worker_free(fm_ctx* ctx);
void fm_gallery_free(fm_ctx* ctx);
void fm_jpegenc_free(fm_ctx* ctx);                                                                // jpegenc.hip
int fm_jpegenc_ensure(fm_ctx* ctx, int mcus_x, int mcus_y);   // the encoder's stream, and its buffers for that many MCUs
hipStream_t fm_jpegenc_stream(fm_ctx* ctx);                   // null before the first fm_jpegenc_ensure
int fm_jpegenc_encode_device(fm_ctx* ctx, const uint8_t* src, int width, int height, int quality, uint8_t* out, size_t capacity,
                             size_t* length);                 // packed BGR in device memory, ordered by the encoder's stream
void fm_overlay_free(fm_ctx* ctx);                                                                // overlay.hip
