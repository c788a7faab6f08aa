// Detector front/back end on the device: preprocessing, YOLO head decode, score/class filter,
// per-class DIoU-NMS, box filter.  (The frames it reads are put on the device by frames.hip.)
//
// Replaces (reference file:line, relative to /root/reference)
//   YOLODetector._preprocess        fastmot/detector.py:289-300  (CuPy zoom order=1 mode='opencv'
//                                   grid_mode=True in uint8, BGR->RGB, HWC->CHW, * 1/255)
//   YOLODetector._create_letterbox  fastmot/detector.py:302-320  (ROI, pad value 0.5)
//   CalDetection / _NewCoords       fastmot/plugins/yolo_layer.cu:127-230
//   YOLODetector._filter_dets       fastmot/detector.py:322-365
//   diou_nms                        fastmot/utils/rect.py:199-244
//
// Differences by design: the reference copies ALL candidates (22 743 x 28 B @608) to the host and
// filters there; here decode + threshold + compaction are one kernel, NMS runs on the device
// (pair matrix as bit masks + one-wave scan) and only the final detections (48 B each) cross
// PCIe.  Candidate order: the reference sorts with unstable quicksorts (ties undefined);
// the device sort is deterministic: (class asc, box_conf desc, original index asc).
// Arithmetic: decode in fp32 with fast exp like the plugin; NMS terms in the types Numba gives
// them (areas f32, box corners / IoU / DIoU f64); rounding half-to-even.
// Roofline: HBM bound -- reads (5+C)*A*sum(HW)*4 B of head tensors (7.7 MB @608/80 classes),
// frame 6.2 MB in, 608*608*8*2 B out.
#include "pixel_source.h"
#include <cmath>
#include <string>
#include <vector>

struct DetState {
    fm_yolo_cfg cfg{};
    bool configured = false;
    int cap = 8192;
    // Results and the post-processing buffers form a ring of slots, one per frame, completed by events: the pass on the
    // NEXT frame(s) can be queued behind this one (MOT.step with next_frame / detector look-ahead: the detector stream never
    // idles) while the host still has to collect this frame's detections.  Frames are collected in enqueue order.  A
    // batched pass (fm_detect_async_ahead) fills FM_MAX_DET_BATCH consecutive slots at most; the ring holds such a pass,
    // the frame being collected and a stale prefetch: `nslot` = FM_MAX_DET_BATCH + 2 slots.  A tiled detector
    // (fm_detect_configure_tiles) fills one slot per TILE and every frame is a pass of n_tiles slots: the ring then holds
    // three such passes -- the one being collected, a prefetched one and a stale one to drop -- `nslot` = 3 n_tiles.
    static constexpr int NSLOT_UNTILED = FM_MAX_DET_BATCH + 2;
    static constexpr int NSLOT = 3 * FM_MAX_DET_BATCH;      // (capacity of the arrays below; slots [0, nslot) are in use)
    int nslot = NSLOT_UNTILED;
    // tiling (n_tiles >= 2; 0: untiled): sample t of every pass is tile t of the ONE frame of the pass
    int n_tiles = 0;
    int tile_x[FM_MAX_DET_BATCH] = {}, tile_y[FM_MAX_DET_BATCH] = {};   // tile origins in the tiling region
    int region_w = 0, region_h = 0;
    double tile_offset[FM_MAX_DET_BATCH][2] = {};           // the decode's box offset per tile (its scale: cfg.size)
    double merge_thresh = 0.6;
    std::vector<fm_det48> tile_stage;                       // one tile's detections while a frame is collected
    std::vector<fm_det48> tile_dets;                        // the frame collected last: per-tile detections, tile-major ...
    std::vector<int32_t> tile_ids;                          // ... their tiles ...
    int tile_count[FM_MAX_DET_BATCH] = {};                  // ... rows per tile
    int tile_sum[2] = {};                                   // ... and the candidates / detections summed over the tiles
    float* cand[NSLOT] = {};        // [cap][8] : x y w h box_conf class cls_prob orig_idx(as float bits)
    float* sorted[NSLOT] = {};      // [cap][8]
    int32_t* counters[NSLOT] = {};  // [0]=n_cand [1]=overflow [2]=n_det
    uint64_t* mask[NSLOT] = {};     // [cap/64][cap]
    fm_det48* dets[NSLOT] = {};     // [cap]
    bool used[NSLOT] = {};
    hipEvent_t ev_dec[NSLOT] = {};  // candidates of the pass complete (stream that produced them; first slot of a pass)
    int post_pending = -1;          // first slot of the pass whose sort + NMS has not been enqueued yet (flush_post) ...
    int post_pending_n = 0;         // ... and its number of slots (images)
    bool general_post = false;                      // the three-kernel sort / bit matrix / scan path (more than 4096 candidates,
                                                    // fm_ctx option "nms_path" = 1); default: nms_greedy_kernel
    static constexpr int GREEDY_RETRY = 1024;       // passes on the general path before the greedy kernel gets another try
    int general_passes = 0;
    int greedy_kmax = 2048, greedy_shrink = 0;      // LDS capacity (candidates) of the next greedy launches; passes since it was too large
    bool sorted_valid[NSLOT] = {};      // d->sorted[slot] holds the pass's sorted rows (general path / test hook)
    static constexpr int PREFIX = 2048;        // detections copied back with the pass (more: synchronous fallback)
    fm_det48* dets_host[NSLOT] = {};
    int32_t* counters_host[NSLOT] = {};
    hipEvent_t ev_done[NSLOT] = {};
    hipStream_t s_fallback = nullptr;          // redo of a pass the greedy kernel declined (collect): NOT s_up, see there
    hipEvent_t ev0[NSLOT] = {}, ev1[NSLOT] = {};   // bracket the network launches (first slot of a pass)
    bool timed[NSLOT] = {};                        // ... of the passes that were timed (fm_ctx option "net_timing")
    // front-ahead (detect_pass): a pass whose leading layers ran on another stream
    hipEvent_t evf0[NSLOT] = {}, evf1[NSLOT] = {}; // bracket the front's launches on that stream (timed passes) ...
    bool timed_front[NSLOT] = {};                  // ... when the timed pass in the slot had a front
    hipEvent_t ev_front[2] = {};                   // front of the pass on buffer set i complete
    int set_slot[2] = {-1, -1};                    // first slot of the pass that used buffer set i last: behind its ev_dec nothing
                                                   // of that pass touches the set any more
    long n_passes = 0;
    int wr = 0, rd = 0, pending = 0, last = -1;   // slot written next / collected next / passes in flight / last collected
    uint8_t* label_mask = nullptr;
    float* rows_in = nullptr;     // test hook upload
    int rows_cap = 0;
    // anchor-free heads with a DFL box branch (fm_detect_configure_dfl): detect_pass launches dfl_decode.h's kernel
    bool dfl = false;
    fm_dfl_heads dfl_heads{};
};

void fm_det_free(DetState* d) {
    if (!d) return;
    for (int i = 0; i < DetState::NSLOT; ++i) {
        for (void* q : {(void*)d->cand[i], (void*)d->sorted[i], (void*)d->counters[i], (void*)d->mask[i], (void*)d->dets[i]})
            if (q) (void)hipFree(q);
    }
    for (void* p : {(void*)d->label_mask, (void*)d->rows_in})
        if (p) (void)hipFree(p);
    if (d->s_fallback) (void)hipStreamDestroy(d->s_fallback);
    for (int i = 0; i < DetState::NSLOT; ++i) {
        if (d->dets_host[i]) (void)hipHostFree(d->dets_host[i]);
        if (d->counters_host[i]) (void)hipHostFree(d->counters_host[i]);
        for (hipEvent_t e : {d->ev_done[i], d->ev_dec[i], d->ev0[i], d->ev1[i], d->evf0[i], d->evf1[i]})
            if (e) (void)hipEventDestroy(e);
    }
    for (hipEvent_t e : d->ev_front)
        if (e) (void)hipEventDestroy(e);
    delete d;
}

namespace {

// ------------------------------------------------------------------------------------ preprocess
// bilinear resize in uint8 with half-pixel centres and edge clamp (cupyx zoom mode='opencv',
// grid_mode=True: src = (dst + 0.5) * (in/out) - 0.5; affine_transform order=1, mode='nearest'),
// result rounded to uint8 (rint), then BGR->RGB, * 1/255 (fp32) and stored as fp16 NHWC with the
// channel dimension padded to 8 (zeros).  Outside the letterbox ROI the input is 0.5.
// One launch for the n images of a batched pass: blockIdx.z = the image (frame src.frame[z], input sample z).
__global__ void preprocess_kernel(const StemSrc src, f16* __restrict__ inp, int in_w, int in_h, int cs) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y, n = blockIdx.z;
    // candidate counters of this frame's decode (one memset node fewer on the detector stream; the previous
    // frame's counters were copied to the host earlier on the same stream)
    int32_t* counters = pick_sample(src.zero4, n);
    if (counters && x < 4 && y == 0) counters[x] = 0;
    if (x >= in_w || y >= in_h) return;
    float rgb[3];
    det_input_pixel(pick_sample(src.frame, n), src.fw, src.fh, x, y, pick_sample(src.roi_x, n), pick_sample(src.roi_y, n),
                    src.roi_w, src.roi_h, rgb);      // (pixel_source.h: shared with the fused stem)
    f16x8 o;
    o[0] = (f16)rgb[0]; o[1] = (f16)rgb[1]; o[2] = (f16)rgb[2];
#pragma unroll
    for (int e = 3; e < 8; ++e) o[e] = (f16)0.f;
    *reinterpret_cast<f16x8*>(inp + (((size_t)n * in_h + y) * in_w + x) * cs) = o;
}

// ------------------------------------------------------------------------------------ decode
struct HeadArgs {
    const float* data;   // NHWC fp32 [H][W][cs]
    int cs, gw, gh, na, base_index;
    float anchors[2 * FM_MAX_ANCHORS];
    float scale_xy;
};

__device__ __forceinline__ float sigmoid_fast(float x) { return 1.0f / (1.0f + __expf(-x)); }

struct FilterArgs {
    const uint8_t* label_mask;
    int num_classes;
    float conf_thresh;
    double size[2], offset[2];
    float* cand;
    int32_t* counters;
    int cap;
};

// appends one candidate row if it survives detector.py:331-341 (class mask, score threshold),
// scaled to pixels: det[:4] *= (size, size); det[:2] -= offset  (in-place float32 arithmetic)
__device__ __forceinline__ void emit_candidate(const FilterArgs& fa, float bx, float by, float bw, float bh,
                                               float box_conf, int cls, float cls_prob, int orig) {
    if (cls < 0 || cls >= 128 || !fa.label_mask[cls]) return;
    const float score = box_conf * cls_prob;
    if (!(score >= fa.conf_thresh)) return;
    const int slot = atomicAdd(fa.counters, 1);
    if (slot >= fa.cap) {
        fa.counters[1] = 1;
        return;
    }
    float* r = fa.cand + (size_t)slot * 8;
    float x = (float)((double)bx * fa.size[0]);
    float y = (float)((double)by * fa.size[1]);
    r[2] = (float)((double)bw * fa.size[0]);
    r[3] = (float)((double)bh * fa.size[1]);
    r[0] = (float)((double)x - fa.offset[0]);
    r[1] = (float)((double)y - fa.offset[1]);
    r[4] = box_conf;
    r[5] = (float)cls;
    r[6] = cls_prob;
    r[7] = __int_as_float(orig);
}

struct HeadSet {
    HeadArgs h[FM_MAX_HEADS];
    int first_block[FM_MAX_HEADS + 1];   // head i owns blocks [first_block[i], first_block[i + 1])
    float* cand[FM_MAX_DET_BATCH];       // image z (blockIdx.y) of a batched pass: its slot's candidate list ...
    int32_t* counters[FM_MAX_DET_BATCH]; // ... and counters (FilterArgs.cand / counters are image 0's)
    double off_x[FM_MAX_DET_BATCH], off_y[FM_MAX_DET_BATCH];   // ... and box offset (FilterArgs.offset): one value for the frames
                                                               // of a batched pass, one per tile for a tiled pass
};

// one thread per (head, anchor, cell), all heads in one launch: plugins/yolo_layer.cu:127-173 (classic) /
// :185-230 (new_coords)
// (blockIdx.y: the image of a batched pass -- its sample of the head tensors, its slot's candidate list)
__global__ void decode_kernel(HeadSet hs, FilterArgs fa, int in_w, int in_h, int new_coords) {
    int hi = 0;
#pragma unroll
    for (int i = 1; i < FM_MAX_HEADS; ++i) hi += (int)blockIdx.x >= hs.first_block[i] ? 1 : 0;
    const HeadArgs& h = hs.h[hi];
    const int idx = ((int)blockIdx.x - hs.first_block[hi]) * blockDim.x + threadIdx.x;
    const int cells = h.gw * h.gh;
    if (idx >= cells * h.na) return;
    const int img = blockIdx.y;
    fa.cand = pick_sample(hs.cand, img);
    fa.counters = pick_sample(hs.counters, img);
    fa.offset[0] = pick_sample(hs.off_x, img);
    fa.offset[1] = pick_sample(hs.off_y, img);
    const int a = idx / cells, cell = idx - a * cells;
    const int row = cell / h.gw, col = cell - row * h.gw;
    const int info = 5 + fa.num_classes;
    const float* p = h.data + ((size_t)img * cells + cell) * h.cs + a * info;
    int cls = 0;
    float best = -INFINITY;
    // four class logits per (4-byte aligned) 16-byte load, scanned in ascending order with the strict comparison of the
    // reference kernel (the first maximum wins): a quarter of the dependent load -> compare steps of the one-by-one loop
    typedef float4 f4u __attribute__((aligned(4)));
    int i = 5;
    for (; i + 4 <= info; i += 4) {
        const float4 v = *reinterpret_cast<const f4u*>(p + i);
        if (v.x > best) { best = v.x; cls = i - 5; }
        if (v.y > best) { best = v.y; cls = i - 4; }
        if (v.z > best) { best = v.z; cls = i - 3; }
        if (v.w > best) { best = v.w; cls = i - 2; }
    }
    for (; i < info; ++i) {
        const float l = p[i];
        if (l > best) { best = l; cls = i - 5; }
    }
    float bx, by, bw, bh, box_prob, cls_prob;
    const float s = h.scale_xy;
    if (!new_coords) {
        cls_prob = sigmoid_fast(best);
        box_prob = sigmoid_fast(p[4]);
        bx = (col + (s * sigmoid_fast(p[0]) - (s - 1.0f) * 0.5f)) / h.gw;
        by = (row + (s * sigmoid_fast(p[1]) - (s - 1.0f) * 0.5f)) / h.gh;
        bw = __expf(p[2]) * h.anchors[2 * a + 0] / in_w;
        bh = __expf(p[3]) * h.anchors[2 * a + 1] / in_h;
    } else {
        cls_prob = best;
        box_prob = p[4];
        bx = (col + (s * p[0] - (s - 1.0f) * 0.5f)) / h.gw;
        by = (row + (s * p[1] - (s - 1.0f) * 0.5f)) / h.gh;
        bw = p[2] * p[2] * 4 * h.anchors[2 * a + 0] / in_w;
        bh = p[3] * p[3] * 4 * h.anchors[2 * a + 1] / in_h;
    }
    bx -= bw / 2;   // centre -> top-left
    by -= bh / 2;
    emit_candidate(fa, bx, by, bw, bh, box_prob, cls, cls_prob, h.base_index + idx);
}

// test hook: candidate rows given by the host ([n][7], fractions of the frame)
__global__ void rows_filter_kernel(const float* __restrict__ rows, int n, FilterArgs fa) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* r = rows + (size_t)i * 7;
    emit_candidate(fa, r[0], r[1], r[2], r[3], r[4], (int)r[5], r[6], i);
}

#include "dfl_decode.h"     // (the decode of anchor-free DFL heads: YOLOv8)

// ------------------------------------------------------------------------------------ sort + NMS + final filter
#include "nms_core.h"       // (the device code of the candidate sort and of both NMS routes)

}  // namespace
// front-ahead with the front on s_up, for a network that has a front: whoever would enqueue the pending post-processing
// early leaves it to the next pass
bool fm_det_defers_flush(fm_ctx* ctx) {
    return ctx->det && ctx->det_net && ctx->det_net->front_k > 0 && ctx->opt_det_front_ahead && ctx->opt_det_front_layers &&
           ctx->opt_det_front_stream == 0;
}
namespace {

int ensure_det(fm_ctx* ctx) {
    if (ctx->det) return 0;
    ctx->det = new DetState();
    return 0;
}

int alloc_post(DetState* d, int cap, int nslot) {
    cap = (cap + 63) & ~63;
    if (d->cand[0] && cap == d->cap && nslot == d->nslot) return 0;
    // (every slot at a new capacity; at the same one only the slots beyond a shorter ring: a tiled detector's nine or
    // twelve slots do not outlive it -- at 65536 candidates the suppression mask alone is 0.5 GB a slot)
    for (int i = (cap != d->cap || !d->cand[0]) ? 0 : nslot; i < DetState::NSLOT; ++i) {
        for (void* p : {(void*)d->cand[i], (void*)d->sorted[i], (void*)d->mask[i], (void*)d->dets[i]})
            if (p) (void)hipFree(p);
        if (d->dets_host[i]) (void)hipHostFree(d->dets_host[i]);
        d->dets_host[i] = nullptr;
        d->cand[i] = d->sorted[i] = nullptr; d->mask[i] = nullptr; d->dets[i] = nullptr;
    }
    for (int i = 0; i < DetState::NSLOT; ++i) d->used[i] = false;
    d->cap = cap;
    d->nslot = nslot;
    d->wr = d->rd = d->pending = 0;
    d->last = -1;
    d->post_pending = -1;
    d->post_pending_n = 0;
    d->set_slot[0] = d->set_slot[1] = -1;       // (the callers left the detector's streams idle)
    for (int i = 0; i < nslot; ++i) {
        if (d->cand[i]) continue;                       // (a slot the shorter ring of the same capacity had already)
        FM_HIP(hipMalloc(&d->cand[i], sizeof(float) * 8 * cap));
        FM_HIP(hipMalloc(&d->sorted[i], sizeof(float) * 8 * cap));
        FM_HIP(hipMalloc(&d->mask[i], sizeof(uint64_t) * (size_t)cap * (cap / 64)));
        FM_HIP(hipMalloc(&d->dets[i], sizeof(fm_det48) * cap));
        FM_HIP(hipHostMalloc(&d->dets_host[i], sizeof(fm_det48) * cap, hipHostMallocDefault));
    }
    for (int i = 0; i < nslot; ++i) {
        if (d->counters[i]) continue;
        FM_HIP(hipMalloc(&d->counters[i], sizeof(int32_t) * 4));
        FM_HIP(hipHostMalloc(&d->counters_host[i], sizeof(int32_t) * 4, hipHostMallocDefault));
        FM_HIP(hipEventCreateWithFlags(&d->ev_done[i], hipEventDisableTiming));
        FM_HIP(hipEventCreateWithFlags(&d->ev_dec[i], hipEventDisableTiming));
        FM_HIP(hipEventCreate(&d->ev0[i]));
        FM_HIP(hipEventCreate(&d->ev1[i]));
        FM_HIP(hipEventCreate(&d->evf0[i]));
        FM_HIP(hipEventCreate(&d->evf1[i]));
    }
    for (hipEvent_t& e : d->ev_front)
        if (!e) FM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (!d->label_mask) FM_HIP(hipMalloc(&d->label_mask, 128));
    return 0;
}

FilterArgs filter_args(DetState* d, int slot) {
    FilterArgs fa{};
    fa.label_mask = d->label_mask;
    fa.num_classes = d->cfg.num_classes;
    fa.conf_thresh = (float)d->cfg.conf_thresh;
    const bool tiled = d->n_tiles > 1;      // (the offset is tile 0's: decode_kernel takes each image's from its HeadSet)
    fa.size[0] = d->cfg.size[0]; fa.size[1] = d->cfg.size[1];
    fa.offset[0] = tiled ? d->tile_offset[0][0] : d->cfg.offset[0]; fa.offset[1] = tiled ? d->tile_offset[0][1] : d->cfg.offset[1];
    fa.cand = d->cand[slot];
    fa.counters = d->counters[slot];
    fa.cap = d->cap;
    return fa;
}

// where the last kernel of a route leaves the detections of `slot` (PostOut, nms_core.h)
static PostOut post_out(const DetState* d, int slot) {
    return {d->cfg.max_area, d->cfg.min_aspect_ratio, d->dets[slot], d->dets_host[slot],
            d->cap < DetState::PREFIX ? d->cap : DetState::PREFIX, d->counters_host[slot]};
}

// a kernel may ask for `bytes` of dynamic LDS from now on (set once per kernel: `done` is the caller's static flag)
template <typename Kernel>
static int allow_dynamic_lds(Kernel kernel, size_t bytes, bool& done) {
    if (done) return 0;
    FM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done = true;
    return 0;
}

static int launch_rank_sort(DetState* d, int slot, hipStream_t sp) {
    const int cap = d->cap;
    static bool configured = false;
    if (int rc = allow_dynamic_lds(rank_sort_lds_kernel, sizeof(uint64_t) * (16384 + 8), configured)) return rc;
    if (cap <= 16384)
        hipLaunchKernelGGL(rank_sort_lds_kernel, dim3(cap / 64 + 1), dim3(256), sizeof(uint64_t) * (cap + 8), sp,
                           d->cand[slot], d->sorted[slot], d->counters[slot], cap);
    else
        hipLaunchKernelGGL(rank_sort_kernel, dim3(cap / 256 + 1), dim3(256), 0, sp, d->cand[slot], d->sorted[slot],
                           d->counters[slot], cap);
    FM_HIP(hipGetLastError());
    d->sorted_valid[slot] = true;
    return 0;
}

// the general three-kernel path: sort, suppression bit matrix, chunked scan (any number of candidates up to the capacity)
static int enqueue_general_post(fm_ctx* ctx, DetState* d, int slot, hipStream_t sp, bool sorted_already = false) {
    const int cap = d->cap;
    if (!sorted_already) {
        int rc = launch_rank_sort(d, slot, sp);
        if (rc) return rc;
    }
    fm_trace_mark(ctx, sp, 22);
    hipLaunchKernelGGL(nms_mask_kernel, dim3(std::min(NMS_MASK_GRID, (cap / 64) * (cap / 64 + 1) / 2)), dim3(256), 0, sp, d->sorted[slot],
                       d->counters[slot], cap, d->cfg.nms_thresh, d->mask[slot]);
    fm_trace_mark(ctx, sp, 23);
    hipLaunchKernelGGL(nms_scan_kernel, dim3(1), dim3(1024), sizeof(uint64_t) * (cap / 64), sp, d->sorted[slot],
                       d->counters[slot], cap, d->mask[slot], post_out(d, slot));
    FM_HIP(hipGetLastError());
    return 0;
}

// sort + the greedy kernel (LDS for `greedy_kmax` candidates, chosen from the candidate counts of the passes collected so
// far; a pass with more is declined by the kernel and collect() runs the bit matrix + scan for it)
static int enqueue_greedy_post(fm_ctx* ctx, DetState* d, int slot, hipStream_t sp) {
    static bool configured = false;
    if (int rc = allow_dynamic_lds(nms_greedy_kernel, ng_lds_bytes(NG_KMAX), configured)) return rc;
    int rc = launch_rank_sort(d, slot, sp);
    if (rc) return rc;
    fm_trace_mark(ctx, sp, 22);
    const int kmax = d->greedy_kmax < d->cap ? d->greedy_kmax : (d->cap < NG_KMAX ? d->cap : NG_KMAX);
    hipLaunchKernelGGL(nms_greedy_kernel, dim3(1), dim3(NG_T), ng_lds_bytes(kmax), sp, d->sorted[slot], d->counters[slot],
                       d->cap, kmax, d->cfg.nms_thresh, post_out(d, slot));
    FM_HIP(hipGetLastError());
    return 0;
}

// sort + NMS + final filter + read-back of the result of the pass in `slot`, on a low-priority stream of their own
// (s_up) behind the event that marks the pass's candidates complete.  The NMS scan is one workgroup for tens of
// microseconds: on the detector stream it kept the next frame's network waiting (1500 candidates per frame: 603 -> 667
// frames/s in alternating runs with the post-processing moved off it).  The post-processing is enqueued by whichever
// comes first of: fm_frame_upload_next (behind the next frame's copy), the next pass, a collection -- in a pipelined
// run that is the collection of the PREVIOUS pass, so it sits in its stream waiting for its network (enqueueing it
// with the pass itself: 837 against 863 frames/s and a wider spread).  Which HIP streams share a hardware queue decides a lot here (the
// context drives more streams than the runtime has queues): one more stream for this work measured 612 -> 430, the
// idle streams of the extra ReID instances 400 / 215 / 215, the ReID stream itself 480, s_up at high priority 450
// (profiles/r03_pipeline_order_ab.txt).
// A batched pass leaves its n images pending together: one wait for the pass's decode, then each image's post-processing.
static int flush_post(fm_ctx* ctx, DetState* d) {
    const int first = d->post_pending, n = d->post_pending_n;
    if (first < 0) return 0;
    d->post_pending = -1;
    d->post_pending_n = 0;
    hipStream_t sp = ctx->s_up;
    FM_HIP(hipStreamWaitEvent(sp, d->ev_dec[first], 0));
    for (int i = 0; i < n; ++i) {
        const int slot = (first + i) % d->nslot;
        fm_trace_mark(ctx, sp, 20);
        int rc_p = (d->general_post || ctx->opt_nms_general) ? enqueue_general_post(ctx, d, slot, sp) : enqueue_greedy_post(ctx, d, slot, sp);
        if (rc_p) return rc_p;
        // (The counters and a bounded prefix of the detections -- they are few; the rest, rare, is fetched at collection
        // time -- are written to page-locked host memory by the scan kernel itself.  As two hipMemcpyAsync they were handed
        // to a copy engine as soon as they were enqueued, i.e. while the pass they wait for still had a millisecond to run,
        // and every later device-to-host copy that landed on that engine -- the embeddings of the frame being tracked, the
        // KLT results -- waited behind them: scripts/trace_pipeline.py showed the main thread receiving its embeddings
        // 0.6 ms after the ReID network had finished, exactly when the NEXT pass's post-processing ended.  Whether it
        // happened depended on the engine the runtime picked: runs of the same binary fell into 650 or 860 frames/s.)
        FM_HIP(hipEventRecord(d->ev_done[slot], sp));
        fm_trace_mark(ctx, sp, 21);
    }
    return 0;
}

// the candidates of the n slots from d->wr on are complete on stream `s` (real path: decode on the detector stream; test
// hook: the row filter): book the pass and leave its post-processing pending
int enqueue_post(fm_ctx* ctx, DetState* d, hipStream_t s, int n = 1) {
    int rc = flush_post(ctx, d);              // (a pass whose post-processing nobody flushed yet: keep the order)
    if (rc) return rc;
    while (d->pending + n > d->nslot) {      // never collected (a caller that only ever enqueues): drop the oldest
        const int drop = d->n_tiles > 1 ? d->n_tiles : 1;       // (a tiled frame is its n_tiles slots: all or none)
        d->rd = (d->rd + drop) % d->nslot;
        d->pending -= drop;
    }
    const int slot = d->wr;
    FM_HIP(hipEventRecord(d->ev_dec[slot], s));
    d->post_pending = slot;
    d->post_pending_n = n;
    for (int i = 0; i < n; ++i) d->used[(slot + i) % d->nslot] = true;
    d->wr = (slot + n) % d->nslot;
    d->pending += n;
    return 0;
}

// a pass is about to write the candidate buffers of the n slots from d->wr on, on stream `s`: the post-processing of
// the passes that used them before must be through with them
static int acquire_slots(fm_ctx* ctx, DetState* d, hipStream_t s, int n = 1) {
    // (a pending pass among them -- only when a batched pass follows a batched pass nobody collected: enqueue its
    // post-processing first, so that its ev_done is the event waited for below)
    if (d->post_pending >= 0 && d->post_pending_n + n > d->nslot) {
        int rc = flush_post(ctx, d);
        if (rc) return rc;
    }
    for (int i = 0; i < n; ++i) {
        const int slot = (d->wr + i) % d->nslot;
        // (in steady state that post-processing ended a step ago: the host can see it, and a wait that is not enqueued is
        // one packet fewer on the stream whose period is the step -- every packet there costs microseconds,
        // r06_net_timing_events_ab.txt)
        if (d->used[slot] && hipEventQuery(d->ev_done[slot]) != hipSuccess) {
            (void)hipGetLastError();                     // (hipErrorNotReady is not an error)
            FM_HIP(hipStreamWaitEvent(s, d->ev_done[slot], 0));
        }
    }
    return 0;
}

int collect(fm_ctx* ctx, DetState* d, hipStream_t s, fm_det48* out, int cap_out, int* n) {
    if (d->pending == 0) {
        fm_set_error("no detector pass in flight (fm_detect_async first)");
        return FM_ERR_STATE;
    }
    const int slot = d->rd;
    // (With front-ahead on the post-processing stream a LATER pass's pending post-processing stays pending: it waits for
    // that pass's decode, and the front of the pass after it, enqueued with the next look-ahead upload, belongs in front
    // of it -- behind it the front starts when the running pass ends, which is no look-ahead at all.  Not when that later
    // pass is complete already: the detector stream is not what bounds the step then, the next pass will not find it
    // busy, and its post-processing should not wait for the next upload.)
    bool later = d->post_pending >= 0 && (slot - d->post_pending + d->nslot) % d->nslot >= d->post_pending_n && fm_det_defers_flush(ctx);
    if (later && hipEventQuery(d->ev_dec[d->post_pending]) == hipSuccess) later = false;
    (void)hipGetLastError();                // (hipErrorNotReady is not an error)
    if (!later) {
        int rc_f = flush_post(ctx, d);
        if (rc_f) return rc_f;
    }
    FM_HIP(hipEventSynchronize(d->ev_done[slot]));
    if (d->counters_host[slot][3] != 0 && !d->counters_host[slot][1]) {
        // the greedy kernel did not take the pass -- more candidates than it was given LDS for (1), or more survivors than
        // its round budget (2: most candidates survive, the bit matrix + scan is the cheaper tool): the pass (sorted
        // already, candidates untouched) goes through the general path now, and so do the following ones -- for good
        // beyond NG_KMAX candidates, otherwise until the greedy kernel is tried again GREEDY_RETRY passes later
        const int why = d->counters_host[slot][3];
        // on a stream of its own: s_up may already hold the NEXT pass's post-processing, which waits for that pass's whole
        // detector network (ev_dec) -- behind it this redo would stall for a network pass.  Every buffer it
        // touches belongs to `slot`, whose earlier work is complete (ev_done above).
        if (!d->s_fallback) FM_HIP(hipStreamCreateWithFlags(&d->s_fallback, hipStreamNonBlocking));
        hipStream_t sp = d->s_fallback;
        int rc_g = enqueue_general_post(ctx, d, slot, sp, d->sorted_valid[slot]);
        if (rc_g) return rc_g;
        FM_HIP(hipStreamSynchronize(sp));
        if (why == 2 || d->counters_host[slot][0] > NG_KMAX) {
            d->general_post = true;
            d->general_passes = 0;
        }
    } else if (d->general_post && d->counters_host[slot][0] <= NG_KMAX * 3 / 4 && ++d->general_passes >= DetState::GREEDY_RETRY) {
        d->general_post = false;
    }
    {   // LDS of the next greedy launches: room for 1.25 x the largest of the recent counts, in steps of 512
        const int k = d->counters_host[slot][0];
        int want = ((k + k / 4 + 511) / 512) * 512;
        if (want < 512) want = 512;
        if (want > NG_KMAX) want = NG_KMAX;
        if (want > d->greedy_kmax) d->greedy_kmax = want;
        else if (want < d->greedy_kmax && ++d->greedy_shrink >= 64) { d->greedy_kmax = want; d->greedy_shrink = 0; }
        else if (want == d->greedy_kmax) d->greedy_shrink = 0;
    }
    d->rd = (slot + 1) % d->nslot;
    --d->pending;
    d->last = slot;
    if (d->counters_host[slot][1]) {
        fm_set_error("candidate list overflow (%d > %d): raise max_candidates", d->counters_host[slot][0], d->cap);
        return FM_ERR_STATE;
    }
    const int nd = d->counters_host[slot][2];
    if (nd > DetState::PREFIX) {
        // (the slot's device list is not reused before the pass after next is enqueued, i.e. not before this returns)
        FM_HIP(hipMemcpy(d->dets_host[slot], d->dets[slot], sizeof(fm_det48) * nd, hipMemcpyDeviceToHost));
    }
    if (nd > cap_out) {
        fm_set_error("output capacity %d < %d detections", cap_out, nd);
        return FM_ERR_ARG;
    }
    memcpy(out, d->dets_host[slot], sizeof(fm_det48) * nd);
    *n = nd;
    return 0;
}

// A frame of a tiled detector: its n_tiles slots are collected in tile order, each exactly like a frame of a batched pass,
// and their union goes through the cross-tile merge (fm_detect_merge_tiles, host: the walk over the groups is serial and
// the rows are on the host in any case).  The frame's slots are consumed whatever happens in one of them, so that the
// ring stays in step: a candidate-list overflow in any tile is this frame's error, reported once all tiles are collected.
int collect_tiles(fm_ctx* ctx, DetState* d, hipStream_t s, fm_det48* out, int cap_out, int* n) {
    const int nt = d->n_tiles;
    if (d->pending < nt) {
        fm_set_error("no detector pass in flight (fm_detect_async first)");
        return FM_ERR_STATE;
    }
    const int first = d->rd, pending = d->pending;
    d->tile_stage.resize((size_t)d->cap);
    d->tile_dets.clear();
    d->tile_ids.clear();
    d->tile_sum[0] = d->tile_sum[1] = 0;
    int rc_first = 0;
    std::string err;
    for (int t = 0; t < nt; ++t) {
        const int slot = (first + t) % d->nslot;
        int k = 0;
        d->rd = slot;                                       // (collect() takes the slot at d->rd)
        const int rc = collect(ctx, d, s, d->tile_stage.data(), d->cap, &k);
        d->tile_count[t] = rc ? 0 : k;
        if (rc) {
            if (!rc_first) { rc_first = rc; err = fm_last_error(); }
            if (rc == FM_ERR_HIP) break;                    // (the device is gone: nothing more to wait for)
            continue;
        }
        d->tile_sum[0] += d->counters_host[slot][0];
        d->tile_sum[1] += k;
        d->tile_dets.insert(d->tile_dets.end(), d->tile_stage.begin(), d->tile_stage.begin() + k);
        d->tile_ids.insert(d->tile_ids.end(), (size_t)k, (int32_t)t);
    }
    d->rd = (first + nt) % d->nslot;
    d->pending = pending - nt;
    d->last = first;                                        // (the pass's network time lies in its first slot)
    if (rc_first) {
        d->tile_dets.clear();
        d->tile_ids.clear();
        for (int t = 0; t < nt; ++t) d->tile_count[t] = 0;
        fm_set_error("%s", err.c_str());
        return rc_first;
    }
    const int total = (int)d->tile_dets.size();
    if (total > cap_out) {                                  // (the merge never returns more rows than it is given)
        d->tile_stage.resize((size_t)std::max(total, d->cap));
        int nm = 0;
        int rc = fm_detect_merge_tiles(d->tile_dets.data(), d->tile_ids.data(), total, nt, d->merge_thresh, d->tile_stage.data(), &nm);
        if (rc) return rc;
        if (nm > cap_out) {
            fm_set_error("output capacity %d < %d detections", cap_out, nm);
            return FM_ERR_ARG;
        }
        memcpy(out, d->tile_stage.data(), sizeof(fm_det48) * nm);
        *n = nm;
        return 0;
    }
    return fm_detect_merge_tiles(d->tile_dets.data(), d->tile_ids.data(), total, nt, d->merge_thresh, out, n);
}

}  // namespace

// the look-ahead uploads of frames.hip call this once their copy is enqueued (see flush_post); nothing without a detector
int fm_det_flush_post(fm_ctx* ctx) { return ctx->det ? flush_post(ctx, ctx->det) : 0; }
hipStream_t fm_det_front_stream(fm_ctx* ctx) { return ctx->det_net ? ctx->det_net->front_stream : nullptr; }

// ---------------------------------------------------------------------------------------- detector
extern "C" int fm_detect_configure(fm_ctx* ctx, const fm_yolo_cfg* cfg) {
    FM_CHECK_ARG(ctx && cfg);
    FM_CHECK_ARG(cfg->n_heads >= 0 && cfg->n_heads <= FM_MAX_HEADS && cfg->num_classes > 0 && cfg->num_classes <= 128);
    {
        // the candidate sort packs a row's original index into FM_SORT_INDEX_BITS bits of its key
        long long rows = 0;
        for (int i = 0; i < cfg->n_heads; ++i) {
            FM_CHECK_ARG(cfg->n_anchors[i] > 0 && cfg->n_anchors[i] <= FM_MAX_ANCHORS && cfg->grid_w[i] > 0 && cfg->grid_h[i] > 0);
            rows += (long long)cfg->grid_w[i] * cfg->grid_h[i] * cfg->n_anchors[i];
        }
        FM_CHECK_ARG(rows < (1ll << FM_SORT_INDEX_BITS));
    }
    int rc = ensure_det(ctx);
    if (rc) return rc;
    DetState* d = ctx->det;
    FM_HIP(hipStreamSynchronize(ctx->s_det));
    FM_HIP(hipStreamSynchronize(ctx->s_up));
    if (int rc_n = fm_net_sync(ctx->det_net)) return rc_n;      // (a front on another stream)
    d->set_slot[0] = d->set_slot[1] = -1;
    d->post_pending = -1;
    d->post_pending_n = 0;
    d->rd = d->wr;            // a new detector: nothing of the previous one is collected any more
    d->pending = 0;
    d->cfg = *cfg;
    d->dfl = false;           // (fm_detect_configure_dfl sets it behind this call)
    d->general_post = ctx->opt_nms_general != 0;
    d->n_tiles = 0;           // (untiled until fm_detect_configure_tiles says otherwise)
    d->tile_dets.clear();
    d->tile_ids.clear();
    if ((rc = alloc_post(d, cfg->max_candidates > 0 ? cfg->max_candidates : 8192, DetState::NSLOT_UNTILED))) return rc;
    FM_HIP(hipMemcpy(d->label_mask, cfg->label_mask, 128, hipMemcpyHostToDevice));
    d->configured = true;
    return 0;
}

// Anchor-free heads with a DFL box branch (dfl_decode.h).  Everything but the decode kernel is the detector above: the
// same DetState, slots, post-processing and tiling.
extern "C" int fm_detect_configure_dfl(fm_ctx* ctx, const fm_yolo_cfg* cfg, const fm_dfl_heads* heads) {
    FM_CHECK_ARG(ctx && cfg && heads);
    FM_CHECK_ARG(cfg->n_heads >= 1 && cfg->n_heads <= FM_MAX_HEADS && heads->n_levels == cfg->n_heads);
    for (int i = 0; i < heads->n_levels; ++i)
        FM_CHECK_ARG(heads->box_tensor[i] >= 0 && heads->cls_tensor[i] >= 0 && heads->box_coff[i] >= 0 && heads->cls_coff[i] >= 0 &&
                     heads->box_coff[i] % 4 == 0 && heads->cls_coff[i] % 4 == 0 && heads->stride[i] > 0.f);
    fm_yolo_cfg c = *cfg;
    for (int i = 0; i < FM_MAX_HEADS; ++i) {      // (the anchor fields are not read: one row per cell)
        c.n_anchors[i] = i < c.n_heads ? 1 : 0;
        c.head_tensor[i] = -1;
    }
    c.new_coords = 0;
    int rc = fm_detect_configure(ctx, &c);
    if (rc) return rc;
    ctx->det->dfl_heads = *heads;
    ctx->det->dfl = true;
    return 0;
}

extern "C" int fm_detect_configure_tiles(fm_ctx* ctx, int n_tiles, const int32_t* origins, int region_w, int region_h,
                                         const double* offsets, double merge_thresh) {
    FM_CHECK_ARG(ctx && ctx->det && ctx->det->configured);
    FM_CHECK_ARG(n_tiles == 0 || (n_tiles >= 2 && n_tiles <= FM_MAX_DET_BATCH));
    DetState* d = ctx->det;
    if (n_tiles) {
        FM_CHECK_ARG(origins && offsets && region_w > 0 && region_h > 0 && merge_thresh >= 0. && merge_thresh <= 1.);
        // every pixel of every tile lies inside the tiling region (det_input_pixel is called with an ROI of that size)
        for (int t = 0; t < n_tiles; ++t)
            FM_CHECK_ARG(origins[2 * t] >= 0 && origins[2 * t + 1] >= 0 && origins[2 * t] + d->cfg.in_w <= region_w &&
                         origins[2 * t + 1] + d->cfg.in_h <= region_h);
    }
    FM_HIP(hipStreamSynchronize(ctx->s_det));
    FM_HIP(hipStreamSynchronize(ctx->s_up));
    if (int rc_n = fm_net_sync(ctx->det_net)) return rc_n;      // (a front on another stream)
    d->set_slot[0] = d->set_slot[1] = -1;
    d->post_pending = -1;
    d->post_pending_n = 0;
    d->rd = d->wr;            // (passes of the previous geometry are not collected any more)
    d->pending = 0;
    d->tile_dets.clear();
    d->tile_ids.clear();
    d->n_tiles = n_tiles;
    for (int t = 0; t < n_tiles; ++t) {
        d->tile_x[t] = origins[2 * t]; d->tile_y[t] = origins[2 * t + 1];
        d->tile_offset[t][0] = offsets[2 * t]; d->tile_offset[t][1] = offsets[2 * t + 1];
        d->tile_count[t] = 0;
    }
    if (n_tiles) {
        d->region_w = region_w; d->region_h = region_h;
        d->merge_thresh = merge_thresh;
    }
    d->last = -1;             // (nothing of the previous geometry is reported any more: fm_detect_last_counts, _last_tiles)
    d->tile_sum[0] = d->tile_sum[1] = 0;
    for (int t = 0; t < FM_MAX_DET_BATCH; ++t) d->tile_count[t] = 0;
    return alloc_post(d, d->cap, n_tiles ? 3 * n_tiles : DetState::NSLOT_UNTILED);
}

// the detector's frame source for the n images of a pass: frame i (tiled: tile i of frames[0]), the candidate counters of
// slot d->wr + i
static StemSrc det_source(fm_ctx* ctx, DetState* d, const uint8_t* const* frames, int n) {
    const fm_yolo_cfg& c = d->cfg;
    StemSrc src{};
    src.kind = 1; src.fw = ctx->frame_w; src.fh = ctx->frame_h;
    const bool tiled = d->n_tiles > 1;      // (n = n_tiles then, and frames[0] is the frame of all of them)
    src.roi_w = tiled ? d->region_w : c.roi_w; src.roi_h = tiled ? d->region_h : c.roi_h;
    for (int i = 0; i < FM_MAX_DET_BATCH; ++i) {
        src.roi_x[i] = tiled && i < n ? -d->tile_x[i] : c.roi_x;
        src.roi_y[i] = tiled && i < n ? -d->tile_y[i] : c.roi_y;
    }
    for (int i = 0; i < n; ++i) {
        src.frame[i] = tiled ? frames[0] : frames[i];
        src.zero4[i] = d->counters[(d->wr + i) % d->nslot];
    }
    return src;
}

static int enqueue_preprocess(fm_ctx* ctx, DetState* d, NetState* net, const StemSrc& src, int n) {
    const fm_yolo_cfg& c = d->cfg;
    for (int i = 0; i < n; ++i) FM_CHECK_ARG(src.frame[i] != nullptr);
    FM_CHECK_ARG(c.input_tensor >= 0 && c.input_tensor < (int)net->tensors.size());
    const fm_tensor& t = net->tensors[c.input_tensor];
    FM_CHECK_ARG(t.h == c.in_h && t.w == c.in_w && !t.f32);
    hipLaunchKernelGGL(preprocess_kernel, dim3((c.in_w + 255) / 256, c.in_h, n), dim3(256), 0, ctx->s_det,
                       src, (f16*)net->bufs[c.input_tensor], c.in_w, c.in_h, t.c);
    FM_HIP(hipGetLastError());
    return 0;
}

extern "C" int fm_detect_preprocess_only(fm_ctx* ctx) {
    FM_CHECK_ARG(ctx && ctx->det && ctx->det->configured && ctx->det_net);
    const uint8_t* f = ctx->frame_cur;
    const int n = ctx->det->n_tiles > 1 ? ctx->det->n_tiles : 1;
    FM_CHECK_ARG(n <= ctx->det_net->max_batch);
    return enqueue_preprocess(ctx, ctx->det, ctx->det_net, det_source(ctx, ctx->det, &f, n), n);
}

static int detect_pass(fm_ctx* ctx, const uint8_t* const* frames, const hipEvent_t* uploads, int n, bool look_ahead);
static int launch_decode(fm_ctx* ctx, DetState* d, NetState* net, int n, hipStream_t s);

extern "C" int fm_detect_async(fm_ctx* ctx) {
    FM_CHECK_ARG(ctx);
    const uint8_t* f = ctx->frame_cur;
    const hipEvent_t none = nullptr;
    return detect_pass(ctx, &f, &none, 1, false);     // (strictly sequential: never in two parts)
}

// detector on the prefetched next frame (fm_frame_upload_next / fm_frame_ring_select_next)
static int detect_ahead(fm_ctx* ctx, int n);

extern "C" int fm_detect_async_next(fm_ctx* ctx) {
    FM_CHECK_ARG(ctx && ctx->frame_next);
    return detect_ahead(ctx, 1);
}

extern "C" int fm_detect_async_ahead(fm_ctx* ctx, int n) {
    FM_CHECK_ARG(ctx);
    if (ctx->det && ctx->det->n_tiles > 1) {
        fm_set_error("fm_detect_async_ahead: the detector is tiled, its passes take the tiles of one frame");
        return FM_ERR_STATE;
    }
    return detect_ahead(ctx, n);
}

static int detect_ahead(fm_ctx* ctx, int n) {
    FM_CHECK_ARG(ctx && ctx->det_net && n >= 1 && n <= FM_MAX_DET_BATCH);
    if (n > ctx->det_net->max_batch) {
        fm_set_error("detector look-ahead of %d frames > the detector network's max_batch %d", n, ctx->det_net->max_batch);
        return FM_ERR_ARG;
    }
    const uint8_t* frames[FM_MAX_DET_BATCH];
    hipEvent_t uploads[FM_MAX_DET_BATCH];
    for (int k = 1; k <= n; ++k) {
        frames[k - 1] = fm_ahead_frame(ctx, k);
        if (!frames[k - 1]) {
            fm_set_error("look-ahead slot %d holds no frame (fm_frame_upload_ahead / fm_frame_ring_select_ahead)", k);
            return FM_ERR_ARG;
        }
        // a frame in its upload slot: the pass waits for that copy
        uploads[k - 1] = frames[k - 1] == fm_ahead_buf(ctx, k) ? fm_ahead_event(ctx, k) : nullptr;
    }
    return detect_pass(ctx, frames, uploads, n, true);
}

// One network pass at batch n over frames[0..n-1] (n = 1: the single-frame pass), decode of every image into slots
// d->wr .. d->wr + n - 1, their post-processing left pending (flush_post).  A tiled detector takes ONE frame and runs the
// pass at batch n_tiles over its tiles: from here on the tiles are the images of a batched pass.
static int detect_pass(fm_ctx* ctx, const uint8_t* const* frames, const hipEvent_t* uploads, int n, bool look_ahead) {
    FM_CHECK_ARG(ctx && ctx->det && ctx->det->configured && ctx->det_net);
    DetState* d = ctx->det;
    NetState* net = ctx->det_net;
    const fm_yolo_cfg& c = d->cfg;
    const bool tiled = d->n_tiles > 1;
    const int n_frames = n;
    if (tiled) {
        FM_CHECK_ARG(n_frames == 1);
        n = d->n_tiles;
        if (n > net->max_batch) {
            fm_set_error("%d tiles > the detector network's max_batch %d", n, net->max_batch);
            return FM_ERR_ARG;
        }
    }
    FM_CHECK_ARG(n >= 1 && n <= FM_MAX_DET_BATCH && n <= net->max_batch);
    hipStream_t s = ctx->s_det;
    int rc = 0;
    // Round 6: when the network begins with a stem convolution over its input tensor, that convolution computes the
    // resized / normalised pixels itself while it stages its patch (stemconv.hip, pixel_source.h): the preprocess launch
    // (15 us inside the pipeline, between two passes of the stream whose period is the step) and the input tensor's
    // write + read disappear.  Same functions, same values (tests/test_detect_gpu.py compares the head tensors).
    const bool fused = ctx->opt_fused_input && fm_net_stem_fusable(net, c.input_tensor);
    // Front-ahead: nothing at the start of a pass depends on the previous pass, and the start is the part of a pass with
    // more tiles than CUs while the end leaves most of the chip empty.  A single-frame pass that finds the
    // previous one still in flight therefore runs its first K layers on another stream, behind its frame's copy only,
    // and the detector stream carries the rest behind one event.  K = 0: the pass as it always was.
    int K = 0;
    if (ctx->det_flush_deferred && !(look_ahead && fused && n == 1 && !tiled)) {
        ctx->det_flush_deferred = false;
        if ((rc = flush_post(ctx, d))) return rc;
    }
    if (look_ahead && fused && n == 1 && !tiled && ctx->opt_det_front_ahead && ctx->opt_det_front_layers) {
        bool busy = ctx->opt_det_front_ahead == 2;
        if (!busy && d->pending > 0 && hipEventQuery(d->ev_dec[(d->wr + d->nslot - 1) % d->nslot]) != hipSuccess) {
            (void)hipGetLastError();            // (hipErrorNotReady is not an error)
            busy = true;
        }
        if (busy && (rc = fm_net_front_prepare(ctx, net, ctx->opt_det_front_layers, &K))) return rc;
    }
    if (ctx->det_flush_deferred && !K) {        // (what the upload would have done, in today's order)
        ctx->det_flush_deferred = false;
        if ((rc = flush_post(ctx, d))) return rc;
    }
    // the event pair around the network is measurement, not product: two more packets on the stream whose period is the
    // step cost 1.2 % of the frame rate (profiles/r06_net_timing_events_ab.txt) -- recorded on every N-th pass only when
    // a caller asked for it (option "net_timing" = N; bench.py samples every 4th pass).  A batched pass carries them in
    // its first image's slot.
    const bool timing = ctx->opt_net_timing > 0 && d->n_passes++ % ctx->opt_net_timing == 0;
    for (int i = 0; i < n; ++i) {
        d->timed[(d->wr + i) % d->nslot] = timing && i == 0;
        d->timed_front[(d->wr + i) % d->nslot] = timing && i == 0 && K > 0;
    }
    struct Restore {        // whatever happens, the network is left on its own stream with its whole table
        NetState* net;
        ~Restore() { net->first = net->last = 0; fm_net_select(net, nullptr, net->set); }
    } restore{net};
    fm_trace_mark(ctx, s, 10);
    if (K > 0) {
        hipStream_t se = ctx->opt_det_front_stream == 1 ? ctx->s_ext : ctx->s_up;
        const int set = net->set ^ 1;
        if (net->front_stream && net->front_stream != se) FM_HIP(hipStreamSynchronize(net->front_stream));
        net->front_stream = se;
        ++net->front_passes;
        // the frame: its copy was enqueued on s_ext (frames.hip into_ahead), in front of anything enqueued there now
        if (uploads[0] && se != ctx->s_ext) FM_HIP(hipStreamWaitEvent(se, uploads[0], 0));
        if ((rc = acquire_slots(ctx, d, se, 1))) return rc;    // (the first launch zeroes the slot's counters)
        // the set's tensors: the pass that used them last -- two passes ago in a pipelined run, long complete -- is
        // through with them behind its decode
        if (d->set_slot[set] >= 0 && hipEventQuery(d->ev_dec[d->set_slot[set]]) != hipSuccess) {
            (void)hipGetLastError();
            FM_HIP(hipStreamWaitEvent(se, d->ev_dec[d->set_slot[set]], 0));
        }
        const StemSrc src = det_source(ctx, d, frames, n);
        fm_net_select(net, se, set);
        if (timing) FM_HIP(hipEventRecord(d->evf0[d->wr], se));
        fm_trace_mark(ctx, se, 11);
        if ((rc = fm_net_run_stem_from(ctx, net, src, n))) return rc;
        fm_trace_mark(ctx, se, 15);
        if (K > 1) {
            net->first = 1;
            net->last = K;
            if ((rc = fm_net_run_internal(ctx, FM_NET_DETECTOR, n))) return rc;
        }
        if (timing) FM_HIP(hipEventRecord(d->evf1[d->wr], se));
        fm_trace_mark(ctx, se, 16);
        FM_HIP(hipEventRecord(d->ev_front[set], se));
        // the previous pass's post-processing, which waits for that pass's decode, goes BEHIND the front when they share
        // a stream (the look-ahead upload left it to this pass: frames.hip into_ahead)
        if (ctx->det_flush_deferred) {
            ctx->det_flush_deferred = false;
            if ((rc = flush_post(ctx, d))) return rc;
        }
        fm_net_select(net, nullptr, set);
        FM_HIP(hipStreamWaitEvent(s, d->ev_front[set], 0));     // (the only wait of the pass on the detector stream)
        fm_trace_mark(ctx, s, 14);
        if (timing) FM_HIP(hipEventRecord(d->ev0[d->wr], s));
        net->first = K;
        net->last = 0;
        if ((rc = fm_net_run_internal(ctx, FM_NET_DETECTOR, n))) return rc;
        net->first = 0;
    } else {
        for (int i = 0; i < n_frames; ++i)
            if (uploads[i]) FM_HIP(hipStreamWaitEvent(s, uploads[i], 0));
        if ((rc = acquire_slots(ctx, d, s, n))) return rc;
        fm_trace_mark(ctx, s, 14);
        const StemSrc src = det_source(ctx, d, frames, n);
        if (fused) {
            if (timing) FM_HIP(hipEventRecord(d->ev0[d->wr], s));
            fm_trace_mark(ctx, s, 11);
            if ((rc = fm_net_run_stem_from(ctx, net, src, n))) return rc;
            fm_trace_mark(ctx, s, 15);
            net->first = 1;
            rc = fm_net_run_internal(ctx, FM_NET_DETECTOR, n);
            net->first = 0;
            if (rc) return rc;
        } else {
            if ((rc = enqueue_preprocess(ctx, d, net, src, n))) return rc;
            if (timing) FM_HIP(hipEventRecord(d->ev0[d->wr], s));
            fm_trace_mark(ctx, s, 11);
            if ((rc = fm_net_run_internal(ctx, FM_NET_DETECTOR, n))) return rc;
        }
    }
    d->set_slot[net->set] = d->wr;
    if (timing) FM_HIP(hipEventRecord(d->ev1[d->wr], s));
    fm_trace_mark(ctx, s, 12);
    if ((rc = launch_decode(ctx, d, net, n, s))) return rc;      // (counters were zeroed by this pass's preprocess / stem kernel)
    fm_trace_mark(ctx, s, 13);
    return enqueue_post(ctx, d, s, n);
}

// the decode of the n images of a pass on stream s, into the candidate lists of slots d->wr .. d->wr + n - 1
static int launch_decode(fm_ctx* ctx, DetState* d, NetState* net, int n, hipStream_t s) {
    const fm_yolo_cfg& c = d->cfg;
    const bool tiled = d->n_tiles > 1;
    FilterArgs fa = filter_args(d, d->wr);
    HeadSet hs{};
    for (int i = 0; i < n; ++i) {
        const int slot = (d->wr + i) % d->nslot;
        hs.cand[i] = d->cand[slot];
        hs.counters[i] = d->counters[slot];
    }
    for (int i = 0; i < FM_MAX_DET_BATCH; ++i) {
        hs.off_x[i] = tiled && i < n ? d->tile_offset[i][0] : c.offset[0];
        hs.off_y[i] = tiled && i < n ? d->tile_offset[i][1] : c.offset[1];
    }
    int base = 0, blocks = 0;
    for (int i = 0; i < FM_MAX_HEADS + 1; ++i) hs.first_block[i] = 0x7fffffff;
    if (d->dfl) {
        const fm_dfl_heads& dh = d->dfl_heads;
        const bool per_cell = ctx->opt_dfl_decode_form == 1;
        const int cells_per_block = per_cell ? 256 : 16;
        DflSet ds{};
        for (int i = 0; i < FM_MAX_HEADS + 1; ++i) ds.first_block[i] = 0x7fffffff;
        for (int i = 0; i < c.n_heads; ++i) {
            FM_CHECK_ARG(dh.box_tensor[i] < (int)net->tensors.size() && dh.cls_tensor[i] < (int)net->tensors.size());
            const fm_tensor& tb = net->tensors[dh.box_tensor[i]];
            const fm_tensor& tc = net->tensors[dh.cls_tensor[i]];
            FM_CHECK_ARG(tb.f32 && tc.f32 && tb.h == c.grid_h[i] && tb.w == c.grid_w[i] && tc.h == c.grid_h[i] && tc.w == c.grid_w[i]);
            FM_CHECK_ARG(tb.c % 4 == 0 && tc.c % 4 == 0 && dh.box_coff[i] + 4 * FM_DFL_BINS <= tb.c && dh.cls_coff[i] + c.num_classes <= tc.c);
            DflHead& h = ds.h[i];
            h.box = (const float*)net->bufs[dh.box_tensor[i]];
            h.cls = (const float*)net->bufs[dh.cls_tensor[i]];
            h.box_cs = tb.c; h.box_coff = dh.box_coff[i]; h.cls_cs = tc.c; h.cls_coff = dh.cls_coff[i];
            h.gw = c.grid_w[i]; h.gh = c.grid_h[i]; h.base_index = base;
            h.stride = dh.stride[i];
            const int cnt = h.gw * h.gh;
            ds.first_block[i] = blocks;
            blocks += (cnt + cells_per_block - 1) / cells_per_block;
            base += cnt;
        }
        if (per_cell) hipLaunchKernelGGL(dfl_decode_cell_kernel, dim3(blocks, n), dim3(256), 0, s, ds, hs, fa, c.in_w, c.in_h);
        else hipLaunchKernelGGL(dfl_decode_kernel, dim3(blocks, n), dim3(256), 0, s, ds, hs, fa, c.in_w, c.in_h);
        FM_HIP(hipGetLastError());
        return 0;
    }
    for (int i = 0; i < c.n_heads; ++i) {
        FM_CHECK_ARG(c.head_tensor[i] >= 0 && c.head_tensor[i] < (int)net->tensors.size());
        const fm_tensor& t = net->tensors[c.head_tensor[i]];
        FM_CHECK_ARG(t.f32 && t.h == c.grid_h[i] && t.w == c.grid_w[i] && c.n_anchors[i] <= FM_MAX_ANCHORS);
        HeadArgs& h = hs.h[i];
        h.data = (const float*)net->bufs[c.head_tensor[i]];
        h.cs = t.c; h.gw = c.grid_w[i]; h.gh = c.grid_h[i]; h.na = c.n_anchors[i];
        h.base_index = base;
        memcpy(h.anchors, c.anchors[i], sizeof(float) * 2 * FM_MAX_ANCHORS);
        h.scale_xy = c.scale_xy[i];
        const int cnt = h.gw * h.gh * h.na;
        hs.first_block[i] = blocks;
        blocks += (cnt + 255) / 256;
        base += cnt;
    }
    if (blocks) hipLaunchKernelGGL(decode_kernel, dim3(blocks, n), dim3(256), 0, s, hs, fa, c.in_w, c.in_h, c.new_coords);
    FM_HIP(hipGetLastError());
    return 0;
}

// Measurement hook (scripts/yolov8_timing.py): the decode kernel alone, `iters` times over the head tensors the last pass
// left, each launch between two HIP events (the candidate counters are zeroed in front of each); -> the mean in us.
// Nothing may be in flight; the candidate lists it fills are not collected.
extern "C" int fm_detect_decode_us(fm_ctx* ctx, int iters, float* us) {
    FM_CHECK_ARG(ctx && ctx->det && ctx->det->configured && ctx->det_net && iters >= 1 && us);
    DetState* d = ctx->det;
    FM_CHECK_ARG(d->pending == 0 && d->post_pending < 0);
    hipStream_t s = ctx->s_det;
    const int n = d->n_tiles > 1 ? d->n_tiles : 1;
    FM_HIP(hipStreamSynchronize(s));
    FM_HIP(hipStreamSynchronize(ctx->s_up));
    double total = 0;
    for (int it = 0; it < iters; ++it) {
        for (int i = 0; i < n; ++i) FM_HIP(hipMemsetAsync(d->counters[(d->wr + i) % d->nslot], 0, sizeof(int32_t) * 4, s));
        FM_HIP(hipEventRecord(d->ev0[d->wr], s));
        if (int rc = launch_decode(ctx, d, ctx->det_net, n, s)) return rc;
        FM_HIP(hipEventRecord(d->ev1[d->wr], s));
        FM_HIP(hipEventSynchronize(d->ev1[d->wr]));
        float ms = 0.f;
        FM_HIP(hipEventElapsedTime(&ms, d->ev0[d->wr], d->ev1[d->wr]));
        total += ms;
    }
    *us = (float)(total * 1e3 / iters);
    return 0;
}

extern "C" int fm_detect_sync(fm_ctx* ctx, fm_det48* out, int cap, int* n) {
    FM_CHECK_ARG(ctx && ctx->det && ctx->det->configured && out && n);
    if (ctx->det->n_tiles > 1) return collect_tiles(ctx, ctx->det, ctx->s_det, out, cap, n);
    return collect(ctx, ctx->det, ctx->s_det, out, cap, n);
}

extern "C" int fm_filter_dets(fm_ctx* ctx, const float* rows, int n, fm_det48* out, int cap, int* n_out) {
    FM_CHECK_ARG(ctx && ctx->det && ctx->det->configured && n >= 0 && out && n_out);
    FM_CHECK_ARG(n < (1 << FM_SORT_INDEX_BITS));          // (the sort key's index field)
    DetState* d = ctx->det;
    hipStream_t s = ctx->s_det;
    FM_HIP(hipStreamSynchronize(s));
    FM_HIP(hipStreamSynchronize(ctx->s_up));
    if (int rc_n = fm_net_sync(ctx->det_net)) return rc_n;      // (a front on another stream)
    d->set_slot[0] = d->set_slot[1] = -1;
    d->post_pending = -1;
    d->post_pending_n = 0;
    d->rd = d->wr;            // (test hook: passes nobody collected are dropped; the streams are idle here)
    d->pending = 0;
    if (n > d->rows_cap) {
        if (d->rows_in) FM_HIP(hipFree(d->rows_in));
        d->rows_in = nullptr;
        FM_HIP(hipMalloc(&d->rows_in, sizeof(float) * 7 * (size_t)n));
        d->rows_cap = n;
    }
    if (n) FM_HIP(hipMemcpyAsync(d->rows_in, rows, sizeof(float) * 7 * (size_t)n, hipMemcpyHostToDevice, s));
    FM_HIP(hipMemsetAsync(d->counters[d->wr], 0, sizeof(int32_t) * 4, s));
    if (n) hipLaunchKernelGGL(rows_filter_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d->rows_in, n, filter_args(d, d->wr));
    int rc = enqueue_post(ctx, d, s);
    if (rc) return rc;
    return collect(ctx, d, s, out, cap, n_out);
}

// candidates that passed the confidence threshold / detections that survived NMS and the box filters in the pass that
// fm_detect_sync collected last (what the sort + NMS kernels of that pass worked on)
extern "C" int fm_detect_last_counts(fm_ctx* ctx, int* n_candidates, int* n_detections) {
    FM_CHECK_ARG(ctx && ctx->det && n_candidates && n_detections);
    const DetState* d = ctx->det;
    if (d->last < 0) {
        *n_candidates = *n_detections = 0;
        return 0;
    }
    if (d->n_tiles > 1) {                   // (a tiled frame: the sums over its tiles, before the cross-tile merge)
        *n_candidates = d->tile_sum[0];
        *n_detections = d->tile_sum[1];
        return 0;
    }
    *n_candidates = d->counters_host[d->last][0];
    *n_detections = d->counters_host[d->last][2];
    return 0;
}

// the per-tile detections of the frame fm_detect_sync collected last, before the merge: tile-major, counts[t] rows of tile t
extern "C" int fm_detect_last_tiles(fm_ctx* ctx, fm_det48* out, int cap, int32_t* counts, int* n_tiles) {
    FM_CHECK_ARG(ctx && ctx->det && out && counts && n_tiles);
    const DetState* d = ctx->det;
    FM_CHECK_ARG(d->n_tiles > 1 && (int)d->tile_dets.size() <= cap);
    if (!d->tile_dets.empty()) memcpy(out, d->tile_dets.data(), sizeof(fm_det48) * d->tile_dets.size());
    for (int t = 0; t < d->n_tiles; ++t) counts[t] = d->tile_count[t];
    *n_tiles = d->n_tiles;
    return 0;
}

extern "C" int fm_detect_raw_candidates(fm_ctx* ctx, float* rows, int cap, int* n) {
    FM_CHECK_ARG(ctx && ctx->det && rows && n);
    DetState* d = ctx->det;
    int rc_f = flush_post(ctx, d);
    if (rc_f) return rc_f;
    FM_HIP(hipStreamSynchronize(ctx->s_det));
    FM_HIP(hipStreamSynchronize(ctx->s_up));
    if (int rc_n = fm_net_sync(ctx->det_net)) return rc_n;
    const int slot = (d->wr + d->nslot - 1) % d->nslot;       // the pass enqueued last
    int32_t cnt[4];
    FM_HIP(hipMemcpy(cnt, d->counters[slot], sizeof(cnt), hipMemcpyDeviceToHost));
    const int k = cnt[0] < d->cap ? cnt[0] : d->cap;
    FM_CHECK_ARG(k <= cap);
    FM_HIP(hipMemcpy(rows, d->sorted[slot], sizeof(float) * 8 * k, hipMemcpyDeviceToHost));
    *n = k;
    return 0;
}

// HIP-event time (ms) of the network launches of the last fm_detect_async, measured on the
// detector stream itself (bench.py roofline: conv FLOPs / this time).
extern "C" int fm_detect_net_ms(fm_ctx* ctx, float* ms) {
    FM_CHECK_ARG(ctx && ctx->det && ms && ctx->det->last >= 0);      // the pass collected last
    const int slot = ctx->det->last;
    if (!ctx->det->timed[slot]) { *ms = -1.f; return 0; }       // (this pass was not timed: option "net_timing")
    FM_HIP(hipEventSynchronize(ctx->det->ev1[slot]));
    FM_HIP(hipEventElapsedTime(ms, ctx->det->ev0[slot], ctx->det->ev1[slot]));
    if (ctx->det->timed_front[slot]) {
        // a pass in two parts: the time of its launches is the sum of the two brackets -- the span from the front's first
        // launch to the back's last would contain the wait for the previous pass
        float front = 0.f;
        FM_HIP(hipEventElapsedTime(&front, ctx->det->evf0[slot], ctx->det->evf1[slot]));
        *ms += front;
    }
    return 0;
}
