// SSD detector front and back end on the device (fm_ssd_*): what the reference's SSDDetector does on the host before
// its TensorRT engine (fastmot/detector.py:94-120: resize to the tiling region, tile crops, normalisation) and what the
// engine's NMS_TRT plugin does behind the network (reference models/ssd.py:136-150).
//
//   ssd_preprocess_kernel   [n_tiles][H][W][8] fp16 network input from the context's current BGR frame: pixel (x, y) of
//                           tile t = pixel (x + tile_x, y + tile_y) of the frame resized to the tiling region with
//                           cv2.resize's arithmetic (crop_u8_pixel over the whole frame, pixel_source.h: INTER_LINEAR
//                           fixed point, an exact 2x decimation as INTER_AREA), BGR -> RGB, float32(u8 * (2 / 255.) - 1.).
//   ssd_class_nms_kernel    one workgroup per (tile, class != 0): score = sigmoid(logit) of every anchor, those above 1e-8
//                           sorted (bitonic, LDS) by score descending / anchor ascending, the first topk decoded (TF centre
//                           coding: t / BOX_SCALES, cy = ty ha + cya, h = exp(th) ha, corners clipped to [0, 1]) and run
//                           through greedy NMS (IoU without +1, dropped when > nms_thresh against a kept, higher-scored
//                           box); survivors in order to a per-(tile, class) list.
//   ssd_topk_kernel         one workgroup per tile: topk-step merge of the (sorted) class lists, ties by (class, anchor)
//                           ascending; rows (tile, label, conf, xmin, ymin, xmax, ymax) written to page-locked memory,
//                           unused rows (tile, -1, 0, 0, 0, 0, 0).
// Keys are 64 bits: the score's float bits above the bitwise complement of the tie-break index, so one unsigned compare
// orders both (scores are positive floats: their bit patterns order like their values).
#include "pixel_source.h"
#include <memory>

namespace {

constexpr int SSD_MAX_ANCHORS = 4096;    // per tile (bitonic sort of that many 64-bit keys: 32 KB of LDS)
constexpr int SSD_MAX_TOPK = 256;
constexpr int SSD_MAX_CLASSES = 256;
constexpr int SSD_MAX_HEADS = FM_MAX_SSD_HEADS;

struct SsdHeads {
    const float* data[SSD_MAX_HEADS];    // [n_tiles][h * w][cs] f32, channels [A * 4 | A * num_classes]
    int cs[SSD_MAX_HEADS], hw[SSD_MAX_HEADS], na[SSD_MAX_HEADS];
};

struct SsdPost {
    SsdHeads heads;
    const float4* anchors;       // [n_anchors] (cy, cx, h, w)
    const int4* src;             // [n_anchors] (head, cell, anchor within the cell, 0)
    int n_anchors, np2;          // np2: next power of two >= n_anchors
    int num_classes, topk;
    float nms_thresh;
    float scale[4];              // BOX_SCALES (y, x, h, w)
    unsigned long long* surv;    // [n_tiles][num_classes][topk] keys of the per-class survivors, descending
    int32_t* surv_n;             // [n_tiles][num_classes]
    float* rows;                 // [n_tiles][topk][7], page-locked
};

template <typename T>
__device__ __forceinline__ T pick_head(const T (&a)[SSD_MAX_HEADS], int i) {
    T r = a[0];
#pragma unroll
    for (int k = 1; k < SSD_MAX_HEADS; ++k) r = i == k ? a[k] : r;
    return r;
}

__device__ __forceinline__ const float* head_cell(const SsdHeads& h, const int4 s, int tile) {
    const float* base = pick_head(h.data, s.x);
    const int cs = pick_head(h.cs, s.x), hw = pick_head(h.hw, s.x);
    return base + ((size_t)tile * hw + s.y) * cs;
}

// (xmin, ymin, xmax, ymax) of anchor `a` in tile `tile`
__device__ __forceinline__ float4 ssd_decode_box(const SsdPost& p, int tile, int a) {
    const int4 s = p.src[a];
    const float4 an = p.anchors[a];
    const float* loc = head_cell(p.heads, s, tile) + s.z * 4;
    const float ty = loc[0] / p.scale[0], tx = loc[1] / p.scale[1], th = loc[2] / p.scale[2], tw = loc[3] / p.scale[3];
    const float cy = ty * an.z + an.x, cx = tx * an.w + an.y;
    const float h = __expf(th) * an.z, w = __expf(tw) * an.w;
    float4 b;
    b.x = fminf(fmaxf(cx - 0.5f * w, 0.f), 1.f);
    b.y = fminf(fmaxf(cy - 0.5f * h, 0.f), 1.f);
    b.z = fminf(fmaxf(cx + 0.5f * w, 0.f), 1.f);
    b.w = fminf(fmaxf(cy + 0.5f * h, 0.f), 1.f);
    return b;
}

__device__ __forceinline__ float ssd_iou(const float4 a, const float4 b) {
    const float iw = fminf(a.z, b.z) - fmaxf(a.x, b.x), ih = fminf(a.w, b.w) - fmaxf(a.y, b.y);
    if (iw <= 0.f || ih <= 0.f) return 0.f;
    const float inter = iw * ih;
    const float uni = (a.z - a.x) * (a.w - a.y) + (b.z - b.x) * (b.w - b.y) - inter;
    return uni > 0.f ? inter / uni : 0.f;
}

__global__ __launch_bounds__(256) void ssd_preprocess_kernel(const uint8_t* __restrict__ frame, int fw, int fh,
                                                             f16* __restrict__ out, int W, int H, int cs, int region_w,
                                                             int region_h, const int* __restrict__ tile_xy) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, t = blockIdx.z;
    if (x >= W) return;
    const double whole[4] = {0., 0., (double)(fw - 1), (double)(fh - 1)};
    int bgr[3] = {0, 0, 0};
    crop_u8_pixel(frame, fw, fh, whole, x + tile_xy[2 * t], y + tile_xy[2 * t + 1], region_w, region_h, bgr);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[2 - c] = (f16)(float)((double)bgr[c] * (2. / 255.) - 1.);      // BGR -> RGB
    f16* dst = out + (((size_t)t * H + y) * W + x) * cs;
    *reinterpret_cast<f16x8*>(dst) = o;
    for (int c = 8; c < cs; c += 8) *reinterpret_cast<f16x8*>(dst + c) = f16x8{};
}

__global__ __launch_bounds__(256) void ssd_class_nms_kernel(const SsdPost p) {
    __shared__ unsigned long long keys[SSD_MAX_ANCHORS];
    __shared__ float4 box[SSD_MAX_TOPK];
    __shared__ int keep[SSD_MAX_TOPK];
    const int tid = threadIdx.x, cls = blockIdx.x + 1, tile = blockIdx.y;
    // ---- scores -> keys
    for (int i = tid; i < p.np2; i += 256) {
        unsigned long long key = 0;
        if (i < p.n_anchors) {
            const int4 s = p.src[i];
            const int na = pick_head(p.heads.na, s.x);
            const float logit = head_cell(p.heads, s, tile)[na * 4 + s.z * p.num_classes + cls];
            const float score = act_logistic(logit);
            if (score > 1e-8f) key = ((unsigned long long)__float_as_uint(score) << 32) | (0xffffffffu - (unsigned)i);
        }
        keys[i] = key;
    }
    __syncthreads();
    // ---- bitonic sort, descending
    for (int k = 2; k <= p.np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < p.np2; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = keys[i], b = keys[l];
                    const bool desc = (i & k) == 0;
                    if (desc ? a < b : a > b) { keys[i] = b; keys[l] = a; }
                }
            }
            __syncthreads();
        }
    // ---- the first topk candidates: decode, greedy NMS
    const int K = min(p.topk, p.np2);
    for (int i = tid; i < K; i += 256) {
        const unsigned long long key = keys[i];
        keep[i] = key != 0;
        if (key != 0) box[i] = ssd_decode_box(p, tile, (int)(0xffffffffu - (unsigned)(key & 0xffffffffu)));
    }
    __syncthreads();
    for (int i = 0; i < K; ++i) {
        if (!keep[i]) continue;                  // (uniform: read behind the barrier that ended the last writing round)
        const float4 bi = box[i];
        for (int j = i + 1 + tid; j < K; j += 256)
            if (keep[j] && ssd_iou(bi, box[j]) > p.nms_thresh) keep[j] = 0;
        __syncthreads();
    }
    // ---- survivors, in order; the tie-break index becomes (class, anchor)
    if (tid == 0) {
        unsigned long long* dst = p.surv + ((size_t)tile * p.num_classes + cls) * p.topk;
        int n = 0;
        for (int i = 0; i < K; ++i)
            if (keep[i]) {
                const unsigned long long key = keys[i];
                const unsigned anchor = 0xffffffffu - (unsigned)(key & 0xffffffffu);
                dst[n++] = (key & 0xffffffff00000000ull) | (0xffffffffu - (((unsigned)cls << 16) | anchor));
            }
        p.surv_n[tile * p.num_classes + cls] = n;
    }
}

__global__ __launch_bounds__(SSD_MAX_CLASSES) void ssd_topk_kernel(const SsdPost p) {
    __shared__ unsigned long long red[SSD_MAX_CLASSES];
    const int tid = threadIdx.x, tile = blockIdx.x;
    const bool mine = tid >= 1 && tid < p.num_classes;      // thread c walks the list of class c
    const unsigned long long* list = p.surv + ((size_t)tile * p.num_classes + (mine ? tid : 0)) * p.topk;
    const int cnt = mine ? p.surv_n[tile * p.num_classes + tid] : 0;
    int pos = 0;
    for (int r = 0; r < p.topk; ++r) {
        const unsigned long long key = pos < cnt ? list[pos] : 0;
        red[tid] = key;
        __syncthreads();
        for (int off = SSD_MAX_CLASSES / 2; off > 0; off >>= 1) {
            if (tid < off) red[tid] = red[tid] > red[tid + off] ? red[tid] : red[tid + off];
            __syncthreads();
        }
        const unsigned long long best = red[0];
        __syncthreads();
        float* row = p.rows + ((size_t)tile * p.topk + r) * 7;
        if (best == 0) {
            if (tid == 0) { row[0] = (float)tile; row[1] = -1.f; row[2] = row[3] = row[4] = row[5] = row[6] = 0.f; }
        } else if (key == best) {                // (keys are unique: the class is part of them)
            const unsigned idx = 0xffffffffu - (unsigned)(best & 0xffffffffu);
            const float4 b = ssd_decode_box(p, tile, (int)(idx & 0xffffu));
            row[0] = (float)tile; row[1] = (float)(idx >> 16); row[2] = __uint_as_float((unsigned)(best >> 32));
            row[3] = b.x; row[4] = b.y; row[5] = b.z; row[6] = b.w;
            ++pos;
        }
    }
}

}  // namespace

struct SsdState {
    fm_ssd_cfg cfg{};
    int n_anchors = 0, np2 = 0;
    float4* anchors = nullptr;
    int4* src = nullptr;
    int* tile_xy = nullptr;
    unsigned long long* surv = nullptr;
    int32_t* surv_n = nullptr;
    float* rows = nullptr;               // page-locked [n_tiles][topk][7]
    float* host_heads[SSD_MAX_HEADS] = {};   // device staging of fm_ssd_postprocess_host_heads
    hipEvent_t done = nullptr;
    bool pending = false;
    hipEvent_t ev[4] = {};               // option "net_timing" > 0: around the preprocess, network and decode / NMS stages
    bool timed = false;
};

void fm_ssd_free(fm_ctx* ctx) {
    SsdState* s = ctx->ssd;
    if (!s) return;
    for (void* p : {(void*)s->anchors, (void*)s->src, (void*)s->tile_xy, (void*)s->surv, (void*)s->surv_n})
        if (p) (void)hipFree(p);
    for (float* p : s->host_heads)
        if (p) (void)hipFree(p);
    if (s->rows) (void)hipHostFree(s->rows);
    if (s->done) (void)hipEventDestroy(s->done);
    for (hipEvent_t e : s->ev)
        if (e) (void)hipEventDestroy(e);
    delete s;
    ctx->ssd = nullptr;
}

// what the kernels' LDS arrays and the index fields of their keys hold, checked on the host: -> 0 and the anchors per tile
static int ssd_check_cfg(const fm_ssd_cfg* c, long* total_out) {
    FM_CHECK_ARG(c && c->anchors);
    FM_CHECK_ARG(c->n_heads >= 1 && c->n_heads <= SSD_MAX_HEADS && c->num_classes >= 2 && c->num_classes <= SSD_MAX_CLASSES);
    FM_CHECK_ARG(c->topk >= 1 && c->topk <= SSD_MAX_TOPK && c->nms_thresh >= 0.f && c->nms_thresh <= 1.f);
    FM_CHECK_ARG(c->n_tiles >= 1 && c->n_tiles <= FM_MAX_SSD_TILES && c->in_w > 0 && c->in_h > 0 && c->region_w > 0 && c->region_h > 0);
    for (int i = 0; i < 4; ++i) FM_CHECK_ARG(c->box_scales[i] > 0.f);
    for (int t = 0; t < c->n_tiles; ++t)       // every pixel of every tile lies inside the tiling region
        FM_CHECK_ARG(c->tile_x[t] >= 0 && c->tile_y[t] >= 0 && c->tile_x[t] + c->in_w <= c->region_w && c->tile_y[t] + c->in_h <= c->region_h);
    long total = 0;
    for (int k = 0; k < c->n_heads; ++k) {
        FM_CHECK_ARG(c->map_w[k] > 0 && c->map_h[k] > 0 && c->n_anchors[k] > 0 && c->n_anchors[k] <= 64);
        total += (long)c->map_w[k] * c->map_h[k] * c->n_anchors[k];
    }
    FM_CHECK_ARG(total == c->n_anchor_rows && total <= SSD_MAX_ANCHORS);
    *total_out = total;
    return 0;
}

// A refused configuration leaves the context without an SSD state, as a failed allocation does: whoever goes on after
// the error cannot launch with the configuration this call was to replace.
extern "C" int fm_ssd_configure(fm_ctx* ctx, const fm_ssd_cfg* c) {
    FM_CHECK_ARG(ctx);
    long total = 0;
    if (const int bad = ssd_check_cfg(c, &total)) {
        if (ctx->ssd) {
            (void)hipStreamSynchronize(ctx->s_det);
            fm_ssd_free(ctx);
        }
        return bad;
    }
    FM_HIP(hipStreamSynchronize(ctx->s_det));
    fm_ssd_free(ctx);
    std::unique_ptr<SsdState> s(new SsdState());
    s->cfg = *c;
    s->cfg.anchors = nullptr;
    s->n_anchors = (int)total;
    s->np2 = 2;
    while (s->np2 < s->n_anchors) s->np2 <<= 1;
    std::vector<int4> src((size_t)total);
    size_t a = 0;
    for (int k = 0; k < c->n_heads; ++k)
        for (int cell = 0; cell < c->map_w[k] * c->map_h[k]; ++cell)
            for (int j = 0; j < c->n_anchors[k]; ++j) src[a++] = make_int4(k, cell, j, 0);
    std::vector<int> xy(2 * FM_MAX_SSD_TILES, 0);
    for (int t = 0; t < c->n_tiles; ++t) { xy[2 * t] = c->tile_x[t]; xy[2 * t + 1] = c->tile_y[t]; }
    // a failed allocation frees the half-built state and leaves ctx->ssd null: no later call can launch with it
    ctx->ssd = s.release();
    SsdState* d = ctx->ssd;
    auto allocate = [&]() -> int {
        FM_HIP(hipMalloc(&d->anchors, sizeof(float4) * total));
        FM_HIP(hipMemcpy(d->anchors, c->anchors, sizeof(float4) * total, hipMemcpyHostToDevice));
        FM_HIP(hipMalloc(&d->src, sizeof(int4) * total));
        FM_HIP(hipMemcpy(d->src, src.data(), sizeof(int4) * total, hipMemcpyHostToDevice));
        FM_HIP(hipMalloc(&d->tile_xy, sizeof(int) * xy.size()));
        FM_HIP(hipMemcpy(d->tile_xy, xy.data(), sizeof(int) * xy.size(), hipMemcpyHostToDevice));
        FM_HIP(hipMalloc(&d->surv, sizeof(unsigned long long) * (size_t)c->n_tiles * c->num_classes * c->topk));
        FM_HIP(hipMalloc(&d->surv_n, sizeof(int32_t) * (size_t)c->n_tiles * c->num_classes));
        FM_HIP(hipHostMalloc(&d->rows, sizeof(float) * 7 * (size_t)c->n_tiles * c->topk, hipHostMallocDefault));
        FM_HIP(hipEventCreateWithFlags(&d->done, hipEventDisableTiming));
        return 0;
    };
    const int rc = allocate();
    if (rc) fm_ssd_free(ctx);
    return rc;
}

static int ssd_input(fm_ctx* ctx, SsdState* s, NetState** net_out) {
    NetState* net = ctx->det_net;
    FM_CHECK_ARG(net && s->cfg.n_tiles <= net->max_batch && s->cfg.input_tensor >= 0 && s->cfg.input_tensor < (int)net->tensors.size());
    const fm_tensor& t = net->tensors[s->cfg.input_tensor];
    FM_CHECK_ARG(t.h == s->cfg.in_h && t.w == s->cfg.in_w && !t.f32 && t.c >= 8);
    *net_out = net;
    return 0;
}

static int ssd_enqueue_preprocess(fm_ctx* ctx, SsdState* s, NetState* net) {
    FM_CHECK_ARG(ctx->frame_cur != nullptr && ctx->frame_w > 0 && ctx->frame_h > 0);
    const fm_ssd_cfg& c = s->cfg;
    const fm_tensor& t = net->tensors[c.input_tensor];
    hipLaunchKernelGGL(ssd_preprocess_kernel, dim3((c.in_w + 255) / 256, c.in_h, c.n_tiles), dim3(256), 0, ctx->s_det,
                       ctx->frame_cur, ctx->frame_w, ctx->frame_h, (f16*)net->bufs[c.input_tensor], c.in_w, c.in_h, t.c,
                       c.region_w, c.region_h, s->tile_xy);
    FM_HIP(hipGetLastError());
    return 0;
}

static int ssd_enqueue_post(fm_ctx* ctx, SsdState* s, const SsdHeads& heads) {
    const fm_ssd_cfg& c = s->cfg;
    SsdPost p{};
    p.heads = heads;
    p.anchors = s->anchors; p.src = s->src; p.n_anchors = s->n_anchors; p.np2 = s->np2;
    p.num_classes = c.num_classes; p.topk = c.topk; p.nms_thresh = c.nms_thresh;
    for (int i = 0; i < 4; ++i) p.scale[i] = c.box_scales[i];
    p.surv = s->surv; p.surv_n = s->surv_n; p.rows = s->rows;
    hipLaunchKernelGGL(ssd_class_nms_kernel, dim3(c.num_classes - 1, c.n_tiles), dim3(256), 0, ctx->s_det, p);
    FM_HIP(hipGetLastError());
    hipLaunchKernelGGL(ssd_topk_kernel, dim3(c.n_tiles), dim3(SSD_MAX_CLASSES), 0, ctx->s_det, p);
    FM_HIP(hipGetLastError());
    FM_HIP(hipEventRecord(s->done, ctx->s_det));
    s->pending = true;
    return 0;
}

extern "C" int fm_ssd_preprocess_only(fm_ctx* ctx) {
    FM_CHECK_ARG(ctx && ctx->ssd);
    NetState* net = nullptr;
    int rc = ssd_input(ctx, ctx->ssd, &net);
    if (rc) return rc;
    return ssd_enqueue_preprocess(ctx, ctx->ssd, net);
}

extern "C" int fm_ssd_detect_async(fm_ctx* ctx) {
    FM_CHECK_ARG(ctx && ctx->ssd);
    SsdState* s = ctx->ssd;
    const fm_ssd_cfg& c = s->cfg;
    NetState* net = nullptr;
    int rc = ssd_input(ctx, s, &net);
    if (rc) return rc;
    SsdHeads heads{};
    for (int k = 0; k < c.n_heads; ++k) {
        FM_CHECK_ARG(c.head_tensor[k] >= 0 && c.head_tensor[k] < (int)net->tensors.size());
        const fm_tensor& t = net->tensors[c.head_tensor[k]];
        FM_CHECK_ARG(t.f32 && t.h == c.map_h[k] && t.w == c.map_w[k] && t.c >= c.n_anchors[k] * (4 + c.num_classes));
        heads.data[k] = (const float*)net->bufs[c.head_tensor[k]];
        heads.cs[k] = t.c; heads.hw[k] = t.h * t.w; heads.na[k] = c.n_anchors[k];
    }
    // measurement, not product: with option "net_timing" > 0 the three stages are bracketed by events (fm_ssd_stage_ms)
    s->timed = ctx->opt_net_timing > 0;
    if (s->timed) {
        for (hipEvent_t& e : s->ev)
            if (!e) FM_HIP(hipEventCreate(&e));
        FM_HIP(hipEventRecord(s->ev[0], ctx->s_det));
    }
    if ((rc = ssd_enqueue_preprocess(ctx, s, net))) return rc;
    if (s->timed) FM_HIP(hipEventRecord(s->ev[1], ctx->s_det));
    if ((rc = fm_net_run_internal(ctx, FM_NET_DETECTOR, c.n_tiles))) return rc;
    if (s->timed) FM_HIP(hipEventRecord(s->ev[2], ctx->s_det));
    if ((rc = ssd_enqueue_post(ctx, s, heads))) return rc;
    if (s->timed) FM_HIP(hipEventRecord(s->ev[3], ctx->s_det));
    return 0;
}

// HIP-event times (ms) of the stages of the last fm_ssd_detect_async that ran with option "net_timing" > 0 and has been
// collected: ms[0] preprocess, ms[1] network, ms[2] decode / NMS / top-K; -1 each when that pass was not timed
extern "C" int fm_ssd_stage_ms(fm_ctx* ctx, float ms[3]) {
    FM_CHECK_ARG(ctx && ctx->ssd && ms);
    SsdState* s = ctx->ssd;
    ms[0] = ms[1] = ms[2] = -1.f;
    if (!s->timed || s->pending) return 0;
    FM_HIP(hipEventSynchronize(s->ev[3]));
    for (int i = 0; i < 3; ++i) FM_HIP(hipEventElapsedTime(&ms[i], s->ev[i], s->ev[i + 1]));
    return 0;
}

extern "C" int fm_ssd_detect_sync(fm_ctx* ctx, float* rows, int cap, int* n) {
    FM_CHECK_ARG(ctx && ctx->ssd && rows && n);
    SsdState* s = ctx->ssd;
    if (!s->pending) {
        fm_set_error("no SSD pass in flight (fm_ssd_detect_async first)");
        return FM_ERR_STATE;
    }
    const int total = s->cfg.n_tiles * s->cfg.topk;
    FM_CHECK_ARG(cap >= total);
    FM_HIP(hipEventSynchronize(s->done));
    memcpy(rows, s->rows, sizeof(float) * 7 * (size_t)total);
    *n = total;
    s->pending = false;
    return 0;
}

// decode + NMS + top-K on caller-provided head tensors: heads[k] = [n_tiles][map_h * map_w][n_anchors * (4 + num_classes)] f32
extern "C" int fm_ssd_postprocess_host_heads(fm_ctx* ctx, const float* const* heads, float* rows, int cap, int* n) {
    FM_CHECK_ARG(ctx && ctx->ssd && heads && rows && n);
    SsdState* s = ctx->ssd;
    const fm_ssd_cfg& c = s->cfg;
    FM_HIP(hipStreamSynchronize(ctx->s_det));
    SsdHeads h{};
    for (int k = 0; k < c.n_heads; ++k) {
        FM_CHECK_ARG(heads[k] != nullptr);
        const int cs = c.n_anchors[k] * (4 + c.num_classes), hw = c.map_h[k] * c.map_w[k];
        const size_t bytes = sizeof(float) * (size_t)c.n_tiles * hw * cs;
        if (!s->host_heads[k]) FM_HIP(hipMalloc(&s->host_heads[k], bytes));
        FM_HIP(hipMemcpy(s->host_heads[k], heads[k], bytes, hipMemcpyHostToDevice));
        h.data[k] = s->host_heads[k]; h.cs[k] = cs; h.hw[k] = hw; h.na[k] = c.n_anchors[k];
    }
    int rc = ssd_enqueue_post(ctx, s, h);
    if (rc) return rc;
    return fm_ssd_detect_sync(ctx, rows, cap, n);
}
