/*
 * fastmot_hip.h -- C ABI of libfastmot_hip.so, the MI355X (gfx950) implementation of the
 * FastMOT per-frame hot path (MOT.step and everything under it).
 *
 * The reference (GeekAlexis/FastMOT) is Python; its only native boundary is a TensorRT
 * plugin loaded with ctypes (fastmot/utils/inference.py:49-53).  TensorRT does not exist
 * on ROCm, so this header DEFINES the boundary: every entry point below replaces the
 * numeric body of one reference routine (cited as file:line, relative to /root/reference)
 * and is bound from Python with ctypes (fastmot_amd/_lib.py; INTEGRATION.md shows the stub
 * a reference maintainer would add).
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; fm_last_error() gives the message.
 *   - the caller owns every host pointer it passes; the library owns all device memory.
 *   - a ctx is bound to one GPU and is NOT thread safe (one video stream = one ctx = one
 *     process, mirroring the reference's single-threaded MOT.step, mot.py:125-168).
 *   - "slot" = index of a track in the device-resident track table (state mean f64[8],
 *     covariance f64[8][8], running-mean ReID feature f32[512]); slot bookkeeping (which
 *     slot belongs to which track id) stays in Python, like the reference's dict of Tracks.
 *   - boxes are tlbr f64[4] with inclusive corners (utils/rect.py:17-57).
 */
#ifndef FASTMOT_HIP_H
#define FASTMOT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fm_ctx fm_ctx;

/* ---------------------------------------------------------------- runtime ------------- */
/* replaces TRTInference.__init__ stream/buffer setup (utils/inference.py:44-94) */
int fm_ctx_create(int device, fm_ctx** out);
int fm_ctx_destroy(fm_ctx* ctx);
const char* fm_last_error(void);
/* number of visible HIP devices (<0 on error) */
int fm_device_count(void);
/* PCI address ("0000:c1:00.0") of HIP device `device`: the host side uses it to find the GPU's NUMA node
 * (/sys/bus/pci/devices/<id>/numa_node) and binds the stream's process to it before any page-locked memory is
 * allocated (fastmot_amd/runtime.py) -- the per-frame H2D copy of 6.2 MB reads that memory. */
int fm_device_pci_bus_id(int device, char* buf, int buflen);
/* blocks until every stream of the ctx is idle (TRTInference.synchronize, inference.py:119-121) */
int fm_ctx_synchronize(fm_ctx* ctx);
/* makes the context's device current for the calling host thread; every additional host thread that
 * drives the context calls it once (HIP's current device is per thread) */
int fm_ctx_bind_thread(fm_ctx* ctx);
/* tunables: "zero_copy_tracks" (default 2048; batches up to this many tracks / boxes exchange kernel
 * inputs and outputs through pinned device-mapped host memory instead of blit copies; 0 disables),
 * "host_lap_elems" (default 262144; LAP cost matrices up to this many elements are solved by the host
 * solver of the library, larger ones by the device kernels; 0 = always device), "nms_path" (default 0: the fused sort + greedy
 * DIoU-NMS kernel for up to 4096 candidates per frame, the three-kernel sort / bit-matrix / scan path beyond; 1 = always
 * the latter), "convd_cfg" (default 0 = chosen per layer; bm | bn << 8 | kg << 16 | ns << 20 | role << 24 | (spb == 2) << 25 forces
 * one tile / K-group / ring depth (0 = as deep as LDS allows, otherwise >= 2) / loader-wave / steps-per-barrier configuration
 * of FM_OP_CONVD for A/B measurements; read at every launch that is not a graph replay),
 * "fused_input" (default 1: a network that begins with a stem convolution lets that convolution compute its input pixels from the
 * frame -- detector resize / ReID crops -- instead of running the front-end kernel into the input tensor; 0 for A/B and tests),
 * "net_timing" (default 0; N > 0: every N-th detector pass carries the HIP-event pair fm_detect_net_ms reads),
 * "det_front_ahead" / "det_front_layers" / "det_front_stream" (front-ahead: a single-frame look-ahead pass -- fm_detect_async_next,
 * fm_detect_async_ahead(1) -- runs its first K layers on another stream, behind its frame's copy only, while the previous pass
 * still runs; results are bit-identical.  "det_front_ahead": 0 never, 1 when the previous pass is still in flight at enqueue
 * time, 2 always (tests).  "det_front_layers", the only option that takes -1: 0 never, k the first k layers, -1 the longest
 * prefix of layers that write maps of >= 8192 pixels; shortened to what 512 MB of second copies allow.
 * "det_front_stream": 0 the post-processing stream, 1 the ReID stream),
 * "use_graphs" (default 1;
 * 0 launches the network layers one by one instead of replaying hipGraphs), "lk_variant" (diagnostic builds only, include/fastmot_hip_diag.h;
 * 0 is the only value the shipped library accepts).  Initial values can be set with the environment
 * variables FASTMOT_ZERO_COPY / FASTMOT_HOST_LAP / FASTMOT_GRAPHS. */
int fm_ctx_set_option(fm_ctx* ctx, const char* key, int value);
/* the three front-ahead options as they stand */
int fm_ctx_get_option(fm_ctx* ctx, const char* key, int* value);
/* the detector network's front: the cut as prepared by the first pass that took it (0: none), the device memory its two
 * tensor sets and partial-sum buffer cost, the number of passes that ran a front so far */
int fm_net_front_info(fm_ctx* ctx, int* k, long long* bytes, long long* passes);
/* Event trace of a pipelined run (diagnostics; scripts/trace_pipeline.py).  fm_trace_start arms `cap` timed events and
 * returns the host's CLOCK_MONOTONIC time (ns) that corresponds to the trace's zero; from then on the library records
 * one event per stage boundary on the stage's own stream (tags: 10-13 detector pass reached / inputs ready / network done
 * / decode done, 20-21 post-processing, 30-31 next frame's H2D copy, 32-33 ReID network, 40-41 LK launch).
 * fm_trace_read synchronises the device, returns tags[i] / ms[i] (GPU time since the trace's zero) and disarms. */
int fm_trace_start(fm_ctx* ctx, int cap, int64_t* host_ns);
int fm_trace_read(fm_ctx* ctx, int cap, int32_t* tags, float* ms, int* n);
/* writes "name:gcnArch:CUs:clockMHz:hbmBytes" of the ctx device */
int fm_device_info(fm_ctx* ctx, char* buf, int buflen);

/* ---------------------------------------------------------------- Kalman filter ------- */
/* KalmanFilter.__init__/reset_dt tunables (kalman_filter.py:13-94, _init_mat :294-306) */
typedef struct fm_kf_params {
    double dt;
    double std_factor_acc, std_offset_acc;
    double std_factor_det[2], std_factor_klt[2];
    double min_std_det[2], min_std_klt[2];
    double init_pos_weight, init_vel_weight;
    double vel_coupling, vel_half_life;
} fm_kf_params;

int fm_kf_configure(fm_ctx* ctx, const fm_kf_params* p);
/* frame rectangle used for the "ios(box, frame) < 0.5 => lost" test (tracker.py:180,263) */
int fm_set_frame_rect(fm_ctx* ctx, const double tlbr[4]);

/* KalmanFilter.create for n new tracks (kalman_filter.py:96-126): state written to slots */
int fm_trk_create(fm_ctx* ctx, int n, const int32_t* slots, const double* det_tlbr);

/* MultiTracker.apply_kalman body for n tracks in ONE launch (tracker.py:164-183):
 *   warp(H) -> predict -> [update(klt box, FLOW, mult)] -> as_tlbr -> ios(frame) test.
 * H: 3x3 row-major homography.  klt_tlbr[n][4], has_klt[n], mult[n] (std multiplier,
 * tracker.py:175).  Outputs: tlbr_out[n][4] (rounded half-even), lost_out[n] (ios<0.5). */
int fm_trk_step(fm_ctx* ctx, int n, const int32_t* slots, const double* H,
                const double* klt_tlbr, const uint8_t* has_klt, const double* mult,
                double* tlbr_out, uint8_t* lost_out);

/* Same kernel with an explicit stage mask, so that KalmanFilter.warp / predict / update(FLOW)
 * (kalman_filter.py:128-204,227-292) remain individually callable through the mirror class. */
enum { FM_KF_WARP = 1, FM_KF_PREDICT = 2, FM_KF_UPDATE_KLT = 4 };
int fm_trk_step_ops(fm_ctx* ctx, int ops, int n, const int32_t* slots, const double* H,
                    const double* klt_tlbr, const uint8_t* has_klt, const double* mult,
                    double* tlbr_out, uint8_t* lost_out);

/* KalmanFilter.update(..., MeasType.DETECTOR) for n matched (slot, detection box) pairs
 * (tracker.py:259-262).  Same outputs as fm_trk_step. */
int fm_trk_update_det(fm_ctx* ctx, int n, const int32_t* slots, const double* det_tlbr,
                      double* tlbr_out, uint8_t* lost_out);

/* Track.state accessors (track.py:134) -- off the hot path (tests, visualisation). */
int fm_trk_get_state(fm_ctx* ctx, int n, const int32_t* slots, double* mean, double* cov);
int fm_trk_set_state(fm_ctx* ctx, int n, const int32_t* slots, const double* mean, const double* cov);
/* state[dst] = state[src]  (Track.merge_continuation, track.py:204-208) */
int fm_trk_copy_state(fm_ctx* ctx, int dst_slot, int src_slot);

/* ---------------------------------------------------------------- ReID features ------- */
/* embedding dimension of the running-mean feature table (default 512) */
int fm_feat_configure(fm_ctx* ctx, int dim);
/* upload this frame's L2-normalised embeddings [n][dim] f32 (FeatureExtractor.postprocess
 * output, feature_extractor.py:62-74) so that association can use them on the device.
 * If emb == NULL the embeddings already produced on the device by fm_extract_* are used. */
int fm_emb_upload(fm_ctx* ctx, int n, const float* emb);
/* AverageFeature.update for n (slot, embedding row) pairs (track.py:106-112,119-126) */
int fm_feat_update(fm_ctx* ctx, int n, const int32_t* slots, const int32_t* emb_rows);
/* AverageFeature.merge: dst absorbs src (track.py:114-117) */
int fm_feat_merge(fm_ctx* ctx, int dst_slot, int src_slot);
/* clears the feature state of n slots (new Track, track.py:142-143) */
int fm_feat_reset(fm_ctx* ctx, int n, const int32_t* slots);
int fm_feat_get(fm_ctx* ctx, int slot, float* sum, float* avg, int32_t* count);
/* batched read / seed of the running-mean features (cross-stream gallery exchange; not in the
 * reference, opt-in, see fastmot_amd/gallery.py) */
int fm_feat_read(fm_ctx* ctx, int n, const int32_t* slots, float* avg_out, int32_t* count_out);
int fm_feat_write(fm_ctx* ctx, int n, const int32_t* slots, const float* avg, const int32_t* count);

/* ---------------------------------------------------------------- association --------- */
enum { FM_METRIC_EUCLIDEAN = 0, FM_METRIC_COSINE = 1 }; /* utils/distance.py:12-14 */

/* find_occluded (utils/rect.py:143-157) */
int fm_find_occluded(fm_ctx* ctx, int n, const double* tlbr, double thresh, uint8_t* out);

/* All pairwise terms of MultiTracker.update in one launch, kept on the device:
 *   feat[t][d]  cdist(avg_feat[slot t], emb[d])            (utils/distance.py:17-87)
 *   maha[t][d]  KalmanFilter.motion_distance               (kalman_filter.py:206-225,347-353)
 *   iou [t][d]  iou_dist(track box, det box)               (utils/distance.py:91-108)
 * rows = nT tracks (slots[], rounded boxes trk_tlbr[], labels), cols = nD detections
 * (boxes, labels, occluded mask).  Rows without a valid feature use the fill value at
 * stage time (tracker.py:328-330).  trk_feat_f32[t]=1 marks rows whose feature enters cdist as
 * float32 (history tracks in _reid_cost, tracker.py:360-362) instead of the float64 copy used by
 * _matching_cost (tracker.py:321-326): the products are then formed in f32 like the reference. */
int fm_assoc_prepare(fm_ctx* ctx, int metric,
                     int nT, const int32_t* slots, const double* trk_tlbr, const int64_t* trk_label,
                     int nD, const double* det_tlbr, const int64_t* det_label,
                     const uint8_t* det_occluded, const uint8_t* trk_feat_f32);

/* downloads the prepared [nT][nD] f64 matrices (any pointer may be NULL); KalmanFilter.
 * motion_distance / cdist / iou_dist parity tests read them. */
int fm_assoc_get_pairwise(fm_ctx* ctx, double* feat, double* maha, double* iou);

enum {
    FM_STAGE_MATCHING = 0, /* _matching_cost: 0.8 feat + 0.2 maha/chi2, gates (tracker.py:314-341) */
    FM_STAGE_IOU      = 1, /* _iou_cost: gate 1-iou_thresh                     (tracker.py:343-353) */
    FM_STAGE_REID     = 2  /* _reid_cost: feat, label gate only                (tracker.py:355-366) */
};

/* One association stage on its own, the device way of fm_assoc_cascade's stage solver (the cascade itself calls that
 * solver directly; this entry point serves the parity tests and tools): builds the gated cost matrix from the prepared
 * pairwise terms for the given row / column subsets (indices into the fm_assoc_prepare arrays) with stage_cost_kernel,
 * then solves it:
 *   solver 0 = rectangular LAP (scipy.optimize.linear_sum_assignment semantics incl.
 *              tie-breaking; utils/matching.py:10-30) followed by the INF_COST un-matching
 *              of utils/matching.py:58-70: match_gated[k]=1 when cost>=1e5.  Device kernels, or the host solver on
 *              the matrix the kernel wrote into pinned memory when nr * nc <= host_lap_elems.
 *   solver 1 = greedy argmin matching while cost <= max_cost (utils/matching.py:74-97), device kernel.
 * row_label_override: _reid_cost quirk (tracker.py:364) -- labels used for the rows; NULL
 * = labels given to fm_assoc_prepare.
 * Outputs: m_rows/m_cols (local indices into rows[]/cols[], in the solver's output order),
 * n_match.  cost_out (optional, may be NULL): the [nr][nc] f64 cost matrix. */
int fm_assoc_stage(fm_ctx* ctx, int stage, int solver,
                   int nr, const int32_t* rows, int nc, const int32_t* cols,
                   double motion_weight, double max_cost, double fill_val,
                   const int64_t* row_label_override,
                   int32_t* m_rows, int32_t* m_cols, uint8_t* match_gated, int* n_match,
                   double* cost_out);

/* fm_assoc_prepare with two additions.  after_extractor = 1: the embeddings are the batch fm_extract_async is still
 * computing -- the pairwise kernel is ordered behind the ReID network's last launch on the device, so
 * MultiTracker.update_begin can enqueue it while that network runs and the terms are complete a kernel's length after
 * the embeddings (no host wake-up in between).  *host_cascade = 1 when the problem is small enough (nT * nD <=
 * host_lap_elems, zero_copy_tracks > 0) for the terms to be written to page-locked host memory as well, where
 * fm_assoc_cascade reads them. */
int fm_assoc_prepare2(fm_ctx* ctx, int metric,
                      int nT, const int32_t* slots, const double* trk_tlbr, const int64_t* trk_label,
                      int nD, const double* det_tlbr, const int64_t* det_label,
                      const uint8_t* det_occluded, const uint8_t* trk_feat_f32, int after_extractor, int* host_cascade);

/* The association cascade of MultiTracker.update (tracker.py:198-248) in one call, on the terms of the last
 * fm_assoc_prepare / fm_assoc_prepare2.  Where those reached page-locked host memory (host_cascade) every stage is
 * filled and solved on the host; otherwise, or with FM_CASCADE_PER_STAGE in `flags`, each stage runs the device way
 * (fm_assoc_stage).  Same bookkeeping and same results either way; an empty side (no rows or no detections) is valid.  The three
 * linear-assignment stages -- _matching_cost depth by depth (tracker.py:205-218,314-341), _iou_cost for the remaining
 * active and then for the unconfirmed tracks (:220-231,343-353) -- with the unmatched lists in the order of
 * utils/matching.py:58-70 under Numba's set iteration, the confidence / occlusion split of the remaining detections
 * (:233-235) and the greedy re-identification against the history (:236-240,355-366, utils/matching.py:74-97).
 * Rows are indices into the fm_assoc_prepare arrays.  `out` (int32, capacity out_cap >= FM_CASCADE_HEADER +
 * 3 * (n_conf + n_unconf) + 3 * nD): header [n1, n2, n3, nu1, nu2, nu3, n_reid, n_invalid, n_rest, used], then
 * (row, det) pairs of the three stages, the unmatched rows of the three stages (stage 1: its inactive tracks, :221),
 * (index into hist_rows, det) pairs of the re-identification, the occluded unmatched detections, the others. */
#define FM_CASCADE_HEADER 16
#define FM_CASCADE_PER_STAGE 1     /* fm_cascade_in.flags: solve every stage the device way even if the terms reached the host */
typedef struct fm_cascade_in {
    int32_t n_groups;              /* depth groups of the confirmed tracks (tracker.py:219-233: age // 2) */
    int32_t n_unconf, n_hist;
    int32_t flags;                 /* FM_CASCADE_PER_STAGE or 0 */
    const int32_t* group_off;      /* [n_groups + 1] offsets into conf_rows */
    const int32_t* conf_rows;      /* rows of the confirmed tracks, group by group */
    const uint8_t* conf_active;    /* Track.active of each of them */
    const int32_t* unconf_rows;
    const int32_t* hist_rows;      /* history rows (then foreign gallery rows) */
    const int64_t* hist_labels;    /* labels used for them (tracker.py:364 takes the first n of ALL history tracks) */
    const double* det_conf;        /* [nD] */
    double motion_weight, max_assoc_cost, fill_val, max_iou_cost, conf_thresh, max_reid_cost;
} fm_cascade_in;
int fm_assoc_cascade(fm_ctx* ctx, const fm_cascade_in* in, int32_t* out, int out_cap);
/* The host way of fm_assoc_cascade on caller-provided pairwise terms ([nT][nD] f64 each; row_has_feat, labels and the
 * occlusion mask as fm_assoc_prepare takes them): no context, no device -- what the CPU test suite checks against the
 * oracle's restatement of utils/matching.py (tests/test_cascade_host.py).  Not a fallback: the terms themselves only
 * ever come from pairwise_kernel. */
int fm_cascade_host(int nT, int nD, const double* feat, const double* maha, const double* iou,
                    const uint8_t* row_has_feat, const int64_t* trk_label, const int64_t* det_label,
                    const uint8_t* det_occluded, const fm_cascade_in* in, int32_t* out, int out_cap);
/* Context-free pieces of that cascade, for the CPU tests: the [nr][nc] cost matrix its host fill produces for one stage
 * (the rule stage_cost_kernel applies; row_labels[nr] as fm_assoc_stage's override), and the order of
 * list(set(range(n)) - set(matched)) under Numba's set iteration (utils/matching.py:58-60) -- returns the count. */
int fm_stage_cost_host(int stage, int nT, int nD, const double* feat, const double* maha, const double* iou,
                       const uint8_t* row_has_feat, const int64_t* det_label, const uint8_t* det_occluded,
                       int nr, const int32_t* rows, int nc, const int32_t* cols, const int64_t* row_labels,
                       double motion_weight, double max_cost, double fill_val, double* cost);
int fm_unmatched_order(int n, const int32_t* matched, int n_matched, int32_t* out);

/* Stand-alone solvers on a host cost matrix [nr][nc] f64 (device kernels; used by
 * _rectify_matches' greedy_match, tracker.py:384, and by the parity tests). */
int fm_lap(fm_ctx* ctx, const double* cost, int nr, int nc,
           int32_t* m_rows, int32_t* m_cols, int* n_match);
int fm_greedy(fm_ctx* ctx, const double* cost, int nr, int nc, double max_cost,
              int32_t* m_rows, int32_t* m_cols, int* n_match);
/* iou_dist on host boxes (utils/distance.py:91-108) -- used by _rectify_matches */
int fm_iou_dist(fm_ctx* ctx, int na, const double* a, int nb, const double* b, double* out);

/* ---------------------------------------------------------------- conv engine --------- */
/* Replaces the TensorRT engines (fastmot/utils/inference.py:39-125; engine build
 * fastmot/models/yolo.py:106-151, fastmot/models/reid.py:48-92).  A network is a layer table over
 * NHWC fp16 tensors (channels padded to 8); Conv+BN+activation(+shortcut) layers run on the MFMA
 * implicit-GEMM kernel, concat/route is expressed by channel offsets into shared tensors. */
enum { FM_NET_DETECTOR = 0, FM_NET_EXTRACTOR = 1,
       FM_NET_EXTRACTOR_B = 2 /* 2, 3, 4: optional further instances of the ReID network (same layer table, own
                               * buffers and streams): fm_extract_async then runs a batch as 2-4 concurrent parts */ };
#define FM_MAX_EXTRA_EXTRACTORS 3
enum {
    FM_OP_CONV = 0,      /* conv k x k, stride, pad + bias + act (+ residual)                    */
    FM_OP_DWCONV3 = 1,   /* depthwise 3x3 s1 p1 + bias + act (OSNet LightConv3x3)                */
    FM_OP_MAXPOOL = 2,   /* k, stride, pad (yolo2onnx.py:838-863; OSNet k3 s2 p1)               */
    FM_OP_AVGPOOL = 3,   /* k = stride (OSNet transition 2x2)                                   */
    FM_OP_UPSAMPLE2 = 4, /* nearest x2 (yolo2onnx.py:806-836)                                   */
    FM_OP_COPY = 5,      /* channel-slice copy                                                  */
    FM_OP_GATE = 6,      /* OSNet channel gate: GAP -> fc1 -> ReLU -> fc2 -> sigmoid -> gate[0] */
    FM_OP_GATE_SUM = 7,  /* out = sum_i in[i] * gate[i]                                         */
    FM_OP_HEAD = 8,      /* GAP -> Linear(+BN1d) -> ReLU -> L2 normalise -> ctx embeddings      */
    FM_OP_SPP = 10,      /* darknet SPP block: stride-1 max pools k = 13, 9, 5 of in[0] (cin channels)
                          * written to out at channel offsets out_coff + {0, cin, 2 cin}; one launch,
                          * pool9 = pool5 o pool5, pool13 = pool5 o pool9, separable, in LDS      */
    FM_OP_LITECONV = 9,  /* fused OSNet LightConv3x3: 1x1 linear (w_off, no bias) -> depthwise 3x3
                          * (w2_off) + bias (b_off) + act; cin == cout <= 128.  n_in = G <= 4
                          * independent LightConvs of equal geometry in one launch: group g reads
                          * in[g]/in_coff[g], writes out channels [out_coff + g*cin, +cin) and uses
                          * the g-th slab of the stacked weights                                */
    FM_OP_STEMCONV = 12, /* k x k conv (k,stride in {3/1, 3/2, 7/2}) of an input with <= 4 real channels,
                          * cout <= 32, + bias + act: w = fp16 [32][ceil16(k*k*4)] (K order kh,kw,c<4),
                          * b = f32[32]; patch staged in LDS (stemconv.hip)                     */
    FM_OP_ADD = 13,      /* out = in[0] + in[1] (stand-alone [shortcut])                          */
    FM_OP_RESBLOCK = 14, /* fused darknet residual unit (1x1 conv, 3x3 conv, [shortcut] from=-3;
                          * yolo2onnx.py:558-760): out = in[0] + act(conv3x3(act(conv1x1(in[0]))));
                          * cin = cout in {64,128,256} channels, hid = mid channels (% 32, <= 256);
                          * w_off/b_off = the 1x1 conv, w2_off/b2_off = the 3x3 conv; weights in MFMA
                          * fragment order [cout/32][K/16][lane = (k/8%2)*32 + cout%32][k%8], K order
                          * (kh, kw, cin) (resblock.hip)                                          */
    FM_OP_CONVS = 15,    /* FM_OP_CONV for layers with few output pixels and a long reduction (19 x 19 YOLO
                          * levels): K split across the waves of a workgroup, no workspace / reduce launch
                          * (convs.hip).  Same fields and semantics as FM_OP_CONV; cin % 64 == 0; weights in
                          * MFMA fragment order [ceil32(cout)/32][k*k*cin/16][lane][8] as FM_OP_RESBLOCK   */
    FM_OP_LITECHAIN = 16,/* the four streams of an OSNet block (chains of 1..4 FM_OP_LITECONV over in[0]) in one
                          * launch (litechain.hip): stream s writes out channels [out_coff + s*cin, +cin);
                          * w_off / w2_off / b_off = the 10 parameter sets stacked in (stream, level) order,
                          * each laid out as for FM_OP_LITECONV; gate[s] = GAP partial slot of stream s       */
    FM_OP_CONVD = 17,    /* FM_OP_CONV with both operands moved global -> LDS by the DMA path and up to 2 x 2 MFMA accumulators
                          * per wavefront, K optionally split across wave groups of the workgroup (convd.hip).  Same fields
                          * and semantics as FM_OP_CONV; 3x3: cin % 64 == 0; 1x1: cin % 8 == 0 and cin >= 16 (ragged K: the
                          * image is zero-padded to ceil64(K), chunks of a step beyond cin are not fetched); weights as LDS
                          * tile images: [ceil32(cout)/32][ceil64(k*k*cin)/64][32 rows][8 slots][8 halfs], K order (kh, kw, cin),
                          * slot s of row r holding K chunk s ^ ((r / 2) % 8) of that row's 64-wide K step              */
    FM_OP_STEM2 = 18,    /* the first two layers of a Darknet YOLO backbone in one launch (stem2.hip): conv 3x3 s1 (<= 4 real input
                          * channels -> hid = 32, activation gate[0]) then conv 3x3 s2 pad 1 (32 -> cout in {64, 128}, activation act);
                          * in[0] = the network input; w_off / b_off = the first conv as for FM_OP_STEMCONV, w2_off / b2_off = the second
                          * in MFMA fragment order [cout/32][288/16][lane][8] (K order kh, kw, cin) + f32 bias                          */
    FM_OP_PAIR11 = 19,   /* two 1x1 convs around a concat in one launch (pair11.hip): t = act_gate[0](W1 in[0] + b1) (64 -> hid = 64), out =
                          * act(W2 [t | in[1]] + b2) (64 + 64 -> cout in {64, 128}); weights in MFMA fragment order (w_off / b_off, w2_off / b2_off) */
    FM_OP_OSTAIL = 20,   /* OSNet x0.25's last stage and head in one launch, one workgroup per sample (ostail.hip): AvgPool2d(2, 2) of
                          * in[0] (32 x 16 x cin = 96) -> OSBlock (96 -> k = 128, hid = 32 mid channels, with downsample) -> OSBlock
                          * (128 -> 128) -> conv5 -> GAP -> fc (cout = 512, BN folded) -> ReLU -> L2 normalise -> ctx embeddings (as
                          * FM_OP_HEAD).  w_off: the fp16 parameters (`stride` halfs), b_off: the fp32 ones (`pad` floats) in the
                          * order ostail.hip documents (pointwise weights in MFMA fragment order)                                      */
    FM_OP_DWCONV = 21,   /* depthwise 3x3, stride 1 or 2, TF "SAME" padding (out = ceil(in / stride); total = max((out - 1) * stride +
                          * 3 - in, 0), before = total / 2: an even map at stride 2 pads (0, 1)) + bias + act; any cin % 8 == 0;
                          * weights as FM_OP_DWCONV3.  The unfused form of FM_OP_SEPCONV's first stage                              */
    FM_OP_SEPCONV = 22,  /* MobileNet separable block in one launch (sepconv.hip): out = act(W_pw act_gate[0](dw3x3(in[0]) + b_dw) + b_pw),
                          * depthwise stage as FM_OP_DWCONV (w_off = fp16 [9][cin], b_off = f32 [cin]), rounded to fp16 in LDS and never
                          * stored; pointwise stage cin -> cout: w2_off in MFMA fragment order [ceil32(cout)/32][ceil16(cin)/16][lane][8],
                          * b2_off = f32 [ceil32(cout)]; cin, cout % 8 == 0 (fm_sepconv_supported)                                    */
    FM_OP_POOLHEAD = 23, /* pooled embedding head of a classification-style ReID backbone in one launch, one workgroup per sample
                          * (reidhead.hip): global average pool of in[0] (cin channels, cin % 8 == 0, <= 4096) in fp32 -> gate[0] > 0:
                          * per-channel affine, the BN neck folded to w2_off = f32 scale [cin], b2_off = f32 shift [cin] -> gate[1] > 0:
                          * FC cin -> cout (w_off = fp16 [cout][cin], b_off = f32 [cout] with any BatchNorm folded in, act = linear or
                          * ReLU), one wavefront per output row; otherwise cout == cin -> L2 normalise -> ctx embeddings and their
                          * page-locked mirror (as FM_OP_HEAD).  gate[2] > 0: GeM pooling -- gate[2] = the IEEE-754 bits of the fp32
                          * exponent p (0.5 <= p <= 16), gate[3] = the bits of the clamp eps (0 < eps <= 1): the pool sums
                          * max(x, eps)^p and the mean takes the p-th root before the neck (p == 3: two multiplies and cbrtf,
                          * otherwise powf); gate[2] <= 0 (a plain head leaves -1): the average pool                          */
    FM_OP_STEMPOOL = 24, /* the ResNet stem with its max pool in one launch (stempool.hip): conv 7x7 stride 2 pad 3 of in[0] = the network
                          * input (<= 4 real channels) -> cout <= 64 (% 8), + bias + ReLU, rounded to fp16 in LDS and never stored, then
                          * max pool 3x3 stride 2 with gate[0] = 1: pads 1, gate[0] = 0: pads 0 and ceil_mode (windows clipped at the far
                          * edge); w_off = fp16 [ceil32(cout)][208] (K order kh, kw, c < 4), b_off = f32 [ceil32(cout)].  As
                          * FM_OP_STEMCONV, the extractor front end lets it compute the crops from the frame itself            */
    FM_OP_INSTNORM = 25, /* instance normalisation of a channel view in one launch (instnorm.hip; IBN-Net layers): the first hid = cn
                          * channels of in[0]'s view (cin channels; cn % 8 == 0, 8 <= cn <= cin = cout) are normalised per sample and
                          * channel over h x w with the biased variance, y = act((x - mean) * (1 / sqrt(var + eps)) * gamma + beta),
                          * w_off / b_off = f32 gamma [cn] / beta [cn], statistics in fp32 (variance from centred squares); channels
                          * [cn, cin) get the activation only; act = linear or ReLU; eps is a per-op extra: gate[0] = the IEEE-754
                          * bits of the fp32 value (0 <= eps < 1; 1e-5 is 0x3727C5AC).  in_coff / out_coff % 8 == 0, any channel
                          * strides; out is another tensor than in[0] (never in place), fp16 both.  Optional residual: res_mode
                          * FM_RES_BEFORE_ACT adds the view res / res_coff (cin channels, same map) to every channel behind the
                          * affine and in front of the activation (the unfused tail of an OSNet-AIN block)                      */
    FM_OP_CONVIN = 26,   /* the tail of an OSNet-IBN / -AIN block in one launch (convin.hip): pointwise conv of in[0]'s view (cin = K
                          * channels) to cout channels, instance normalisation of the fp32 result per sample and channel over
                          * h x w (biased variance, centred squares), residual, act (linear or ReLU), one fp16 store:
                          *   v = W x + b (+ res: FM_RES_BEFORE_NORM);  y = act((v - mean) / sqrt(var + eps) * gamma + beta (+ res:
                          *   FM_RES_BEFORE_ACT)).  w_off = fp16 weights in MFMA fragment order [ceil32(cout)/32][ceil16(K)/16][lane][8],
                          * b_off / w2_off / b2_off = f32 bias / gamma / beta [ceil32(cout)], gate[0] = the IEEE-754 bits of eps as
                          * FM_OP_INSTNORM; k = 1, stride 1, pad 0; K, cout % 8 == 0 and h * w <= 2048 (fm_convin_supported: a
                          * workgroup keeps one sample's whole map of 32 channels in registers); out is another tensor than
                          * in[0] and than res                                                                               */
    FM_OP_NONLOCAL = 27, /* fast-reid's Non_local block (AGW / SBS models; dot-product form, ONE inner channel) over in[0]'s view in one
                          * launch, a workgroup per sample with up to four sharing its apply pass (nonlocal.hip): theta_i, phi_i, g_i = three dot products over the cin
                          * channels of pixel i plus their biases, s = mean_i(phi_i g_i) per sample, out[i, c] = in[i, c] +
                          * a[c] theta_i s + b[c]; all of it fp32 between the fp16 load and the one fp16 store.  w_off = f32 [3][cin]
                          * (theta, phi, g), b_off = f32 [4]: their biases (the fourth unused), w2_off / b2_off = f32 a [cin] / b [cin]
                          * (the 1 -> cin conv W with its BatchNorm folded).  cin = cout, cin % 8 == 0, 8 <= cin <= 2048 and
                          * h * w <= 4096 (fm_nonlocal_supported: theta of one map stays in LDS); in_coff / out_coff % 8 == 0; no
                          * residual view, no activation; out is another tensor than in[0].  A sample's sum is taken in an order
                          * that depends on (cin, h * w) alone                                                               */
    FM_OP_GATED_SUM = 11 /* OSNet unified aggregation gate in one launch: out = sum_i in[i] *
                          * sigmoid(fc2(relu(fc1(GAP(in[i]))))) with shared fc weights
                          * (w_off, b_off, w2_off, b2_off, hid) -- FM_OP_GATE x n_in + FM_OP_GATE_SUM */
};
enum { FM_ACT_LINEAR = 0, FM_ACT_LEAKY = 1, FM_ACT_MISH = 2, FM_ACT_RELU = 3, FM_ACT_LOGISTIC = 4,
       FM_ACT_SWISH = 5, FM_ACT_RELU6 = 6 /* min(max(x, 0), 6) */ };
enum { FM_RES_NONE = 0, FM_RES_AFTER_ACT = 1, FM_RES_BEFORE_ACT = 2,
       FM_RES_BEFORE_NORM = 3 /* FM_OP_CONVIN only: part of the value that is normalised */ };

typedef struct fm_tensor {
    int32_t h, w, c;     /* per-sample geometry, c = channel stride (multiple of 8) */
    int32_t f32;         /* 1: fp32 storage (YOLO head outputs), 0: fp16 */
    int64_t offset;      /* byte offset in the network's activation arena (256 B aligned), or -1 for a
                          * private buffer.  Tensors whose live ranges do not overlap may share bytes:
                          * keeping the working set small keeps it resident in the 256 MB Infinity Cache */
} fm_tensor;

typedef struct fm_layer {
    int32_t op;
    int32_t n_in;
    int32_t in[4], in_coff[4];
    int32_t out, out_coff;
    int32_t res, res_coff, res_mode;
    int32_t cin, cout, k, stride, pad, act;
    int32_t hid;
    int32_t up;          /* CONV: nearest-neighbour upsampling factor of the stored output (1 or 2):
                          * the [upsample] layer of yolo2onnx.py:806-836 folded into its producer */
    int32_t gate[4];     /* gate slots / per-op extras; -1 = unused.  FM_OP_CONV / FM_OP_CONVS: gate[0] MUST be -1 unless the layer is a
                          * 3x3 stride-2 conv whose column padding differs from `pad` (TF "SAME" over a map with one even and one odd
                          * side), in which case it holds that column padding (0 or 1); any other value >= 0 is FM_ERR_ARG */
    int64_t w_off, b_off, w2_off, b2_off;   /* byte offsets into the weight blob (16 B aligned) */
} fm_layer;

/* weights: CONV  w = fp16 [ceil32(cout)][ceil64(k*k*cin)] (K order kh,kw,cin), b = f32[ceil32(cout)]
 *          DWCONV3 w = fp16 [9][c], b = f32[c];  GATE w=[hid][c] b=[hid] w2=[c][hid] b2=[c];
 *          HEAD  w = fp16 [cout][cin], b = f32[cout]  (BN folded everywhere). */
int fm_net_create(fm_ctx* ctx, int which, int max_batch, int n_tensors, const fm_tensor* tensors,
                  int n_layers, const fm_layer* layers, const void* weights, size_t weight_bytes,
                  int n_gates, int gate_channels, size_t arena_bytes);
int fm_net_destroy(fm_ctx* ctx, int which);
/* enqueues every layer for `batch` samples on the network's stream (no host sync) */
int fm_net_run(fm_ctx* ctx, int which, int batch);
/* host <-> tensor copies (synchronous; tests and weight-free smoke runs) */
int fm_net_tensor_write(fm_ctx* ctx, int which, int tensor, const void* host, size_t bytes);
int fm_net_tensor_read(fm_ctx* ctx, int which, int tensor, void* host, size_t bytes);
/* copies the embeddings produced by FM_OP_HEAD ([n][feat_dim] f32, L2-normalised) to the host
 * after synchronising the extractor stream (FeatureExtractor.postprocess, feature_extractor.py:62-74) */
int fm_net_read_embeddings(fm_ctx* ctx, int n, float* host);
/* the same rows from the page-locked mirror that the network's last layer (FM_OP_HEAD, FM_OP_OSTAIL, FM_OP_POOLHEAD) writes
 * beside the device matrix: what fm_extract_sync hands out without a copy launch */
int fm_net_read_embeddings_mirror(fm_ctx* ctx, int n, float* host);
/* total FLOPs (2*MAC) and minimal HBM bytes of one run at the given batch: the numbers the
 * bench's roofline uses (SURVEY.md section 8d formulas) */
int fm_net_cost(fm_ctx* ctx, int which, int batch, double* flops, double* bytes);
/* average duration in ms of the conv (MFMA) launches of the last fm_net_run measured with HIP
 * events on the network's own stream; enable != 0 switches per-layer timing on (slow path). */
int fm_net_profile(fm_ctx* ctx, int which, int batch, int iters, double* conv_ms, double* other_ms,
                   int* n_conv, int* n_other);

/* per-layer HIP-event times in ms (out[n_layers]); tuning aid */
int fm_net_profile_layers(fm_ctx* ctx, int which, int batch, int iters, double* out);

/* ---------------------------------------------------------------- frames -------------- */
/* Frames are BGR u8 HxWx3, C-contiguous (what VideoIO.read() hands to MOT.step, app.py:85).
 * fm_frame_upload copies a host frame to the ctx's current device frame (pinned staging + async
 * H2D on the detector stream; replaces cp.asarray(frame), detector.py:292).  A ring of frames can
 * also be made resident in HBM up front (bench: inputs resident before the timed region). */
int fm_frame_configure(fm_ctx* ctx, int width, int height, int ring_size);
int fm_frame_upload(fm_ctx* ctx, const uint8_t* bgr);
/* Page-locked host buffers for frames (the reference preallocates pinned HostDeviceMem buffers,
 * utils/inference.py:7-36, flow.py:100-118).  A frame that lies inside a buffer obtained from
 * fm_host_alloc is copied to the device straight from where it is (no staging copy); it must stay
 * unmodified until the step that uses it has returned (next-frame prefetch: until it has been the
 * current frame).  Any other host pointer is staged through the ctx's own pinned buffer first. */
int fm_host_alloc(size_t bytes, void** out);
int fm_host_free(void* p);
/* Next-frame prefetch (no counterpart in the reference, whose detector is synchronous per step): the
 * detector network can be started on frame t+1 while frame t is still in the ReID / association stages.
 * fm_frame_upload_next copies a host frame into the second upload slot (asynchronously; the detector pass on it waits
 * for the copy's event),
 * fm_frame_ring_select_next points at a resident frame; fm_detect_async_next = fm_detect_async on that
 * frame; fm_frame_promote_next makes it the current frame of the next step without another upload. */
int fm_frame_upload_next(fm_ctx* ctx, const uint8_t* bgr);
int fm_frame_ring_select_next(fm_ctx* ctx, int index);
/* Promotes the frame of look-ahead slot 1 to the current frame and moves slot k to k - 1 (k = 2..FM_MAX_DET_BATCH). */
int fm_frame_promote_next(fm_ctx* ctx);
int fm_detect_async_next(fm_ctx* ctx);
/* Detector look-ahead over several frames (no counterpart in the reference).  Slot k (1 <= k <= FM_MAX_DET_BATCH) holds
 * the frame that the step k steps ahead will receive; k = 1 is the slot of fm_frame_upload_next /
 * fm_frame_ring_select_next, and the two calls below with k = 1 are exactly those.
 * fm_frame_upload_ahead copies a host frame into upload slot k (asynchronously, on the ReID stream; one completion
 * event per slot).  Slots k >= 2 and their page-locked staging buffers are allocated on first use.
 * fm_frame_ring_select_ahead points slot k at a resident ring frame. */
#define FM_MAX_DET_BATCH 4
int fm_frame_upload_ahead(fm_ctx* ctx, int k, const uint8_t* bgr);
int fm_frame_ring_select_ahead(fm_ctx* ctx, int k, int index);
/* One detector network pass at batch n over the frames of look-ahead slots 1..n, then decode, sort, NMS and box
 * filters for each image on its own.  Queues n results: each following fm_detect_sync returns one frame's detections,
 * in frame order.  Every image's head tensors equal those of a batch-1 pass over that frame bit for bit (the detector
 * network takes every reduction-order choice from the batch-1 geometry).  n = 1 is fm_detect_async_next.
 * FM_ERR_ARG when n exceeds the detector network's max_batch or a slot 1..n holds no frame.  A candidate-list
 * overflow is reported by the fm_detect_sync of the frame that overflowed. */
int fm_detect_async_ahead(fm_ctx* ctx, int n);
int fm_frame_ring_store(fm_ctx* ctx, int index, const uint8_t* bgr);
int fm_frame_ring_select(fm_ctx* ctx, int index);
int fm_frame_read(fm_ctx* ctx, uint8_t* bgr);   /* current device frame -> host (tests) */
/* NV12 frames (what hardware decoders, capture cards and cameras deliver): a Y plane of `height` rows at `y` and a plane
 * of height / 2 rows of interleaved U, V bytes at `uv`, rows `pitch` >= width bytes apart in both planes (`uv` is a
 * pointer of its own because decoders align the Y plane's height).  The three calls mirror fm_frame_upload,
 * fm_frame_upload_ahead and fm_frame_ring_store one for one: same slots, same streams, same events.  The rows are
 * packed to `width` on the way into the page-locked staging buffer (planes with pitch == width inside a buffer from
 * fm_host_alloc are copied from where they are), 1.5 * width * height bytes cross to the device -- into an NV12 staging
 * buffer per entry point / look-ahead slot, allocated on its first NV12 use and freed by fm_frame_configure and
 * fm_ctx_destroy -- and a kernel on the copy's stream (csrc/nv12.hip) writes the BGR frame where the BGR call would
 * have put it; a look-ahead slot's completion event follows that kernel.  From there on the frame is an ordinary BGR
 * frame.  The conversion is integer and exact, limited range, chroma sample of a 2 x 2 block used for its four pixels:
 *   y = max(Y - 16, 0) * CY, u = U - 128, v = V - 128, h = 1 << 19
 *   R = sat8((y + h + CVR v) >> 20), G = sat8((y + h + CVG v + CUG u) >> 20), B = sat8((y + h + CUB u) >> 20)
 *   FM_NV12_BT601 (OpenCV's COLOR_YUV2BGR_NV12): CY 1220542, CVR 1673527, CUB 2116026, CUG -409993, CVG -852492
 *   FM_NV12_BT709 (round(coef * 2^20)):          CY 1220945, CVR 1879825, CUB 2215014, CUG -223607, CVG -558796
 * FM_ERR_ARG for pitch < width, an unknown matrix, a bad k / index, or a frame size that is not even in both
 * directions; nothing is copied or launched then. */
#define FM_NV12_BT601 0
#define FM_NV12_BT709 1
int fm_frame_upload_nv12(fm_ctx* ctx, const uint8_t* y, const uint8_t* uv, int pitch, int matrix);
int fm_frame_upload_ahead_nv12(fm_ctx* ctx, int k, const uint8_t* y, const uint8_t* uv, int pitch, int matrix);
int fm_frame_ring_store_nv12(fm_ctx* ctx, int index, const uint8_t* y, const uint8_t* uv, int pitch, int matrix);

/* Baseline JPEG frames (an image sequence 'seq/img1/%06d.jpg', the MOTChallenge layout): replaces the decode of
 * fastmot_amd/videoio.py's image-sequence source (Pillow: libjpeg-turbo on the capture thread, then two array copies)
 * and, in the reference, what cv2.VideoCapture / cv2.imread do for such a sequence (fastmot/videoio.py:60-75).  The host
 * keeps the serial part of the format -- marker parsing and Huffman decoding, the two functions below --, the device
 * does the rest while the frame is uploaded (csrc/jpeg.hip): dequantisation, the 8 x 8 inverse DCT, chroma upsampling,
 * YCbCr -> BGR and the store into the frame slot that every stage reads.  The arithmetic is libjpeg-turbo's default
 * decode path (integer "ISLOW" inverse DCT, "fancy" triangle-filter chroma upsampling, 16-bit fixed-point colour
 * conversion; fastmot_amd/utils/jpeg.py states it in numpy), so the BGR frame equals Pillow's / OpenCV's decode of the
 * same file bit for bit.
 *
 * Supported: baseline sequential DCT (SOF0 / 8-bit SOF1), Huffman coding with any tables, one interleaved scan, any
 * restart interval; one component (greyscale: B = G = R = Y) or three YCbCr components (JFIF, or Adobe transform 1) with
 * luma sampling 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0) and chroma 1x1.  Anything else -- progressive, arithmetic,
 * lossless, 12-bit, CMYK / YCCK, RGB-coded, other sampling factors, several scans -- returns FM_ERR_UNSUPPORTED with
 * fm_jpeg_info::unsupported saying which (the caller decodes such a file some other way); nothing else happens.
 * Malformed data (truncated, corrupt, Huffman codes that do not exist, runs past coefficient 63) returns FM_ERR_ARG;
 * no input bytes make either function read outside [data, data + n) or write outside the buffers described below.
 * Both functions need no fm_ctx and no GPU and may be called from any number of threads at once. */
#define FM_ERR_UNSUPPORTED (-4)
#define FM_JPEG_UNSUPPORTED_PROGRESSIVE 1
#define FM_JPEG_UNSUPPORTED_ARITHMETIC 2
#define FM_JPEG_UNSUPPORTED_PROCESS 3      /* lossless / hierarchical */
#define FM_JPEG_UNSUPPORTED_PRECISION 4    /* samples that are not 8-bit */
#define FM_JPEG_UNSUPPORTED_COMPONENTS 5   /* not 1 or 3 components (CMYK / YCCK) */
#define FM_JPEG_UNSUPPORTED_COLORSPACE 6   /* three components that are not YCbCr */
#define FM_JPEG_UNSUPPORTED_SAMPLING 7
#define FM_JPEG_UNSUPPORTED_SCANS 8        /* more than one scan */
struct fm_jpeg_info {
    int32_t width, height;          /* of the image, and of the BGR frame it becomes */
    int32_t ncomp;                  /* 1 or 3 */
    int32_t hsamp[3], vsamp[3];     /* sampling factors per component */
    int32_t mcu_w, mcu_h;           /* MCU size in pixels: 8 * the luma's sampling factors (8 x 8 for one component) */
    int32_t mcus_x, mcus_y;         /* MCU grid: ceil(width / mcu_w), ceil(height / mcu_h) */
    int32_t restart_interval;       /* MCUs between RSTn markers, 0: none */
    int32_t blocks_w[3], blocks_h[3]; /* 8 x 8 blocks per component over the MCU-padded grid */
    int32_t unsupported;            /* FM_JPEG_UNSUPPORTED_* when fm_jpeg_info returned FM_ERR_UNSUPPORTED, else 0 */
    int64_t coef_offset[3];         /* first coefficient of each component in the coefficient buffer (int16 elements) */
    int64_t coef_count;             /* size of the coefficient buffer in int16 elements: 64 * the sum of all blocks */
};
/* (The struct shares its name with the function that fills it in: write `struct fm_jpeg_info` in C and C++ alike.)
 * Parses SOI, APPn, DQT, SOF, DHT, DRI, SOS of the file at [data, data + n) and describes its frame. */
int fm_jpeg_info(const uint8_t* data, size_t n, struct fm_jpeg_info* out);
/* Huffman-decodes the file's scan (table-driven: a 9-bit look-ahead table per Huffman table, canonical decoding for
 * longer codes; 0xFF00 stuffing, RSTn markers, DC prediction per component, EOB / ZRL).  `info`: what fm_jpeg_info
 * returned for the same bytes.  coef[info->coef_count]: the quantised coefficients, per component (at coef_offset[c])
 * as [block_row][block_col][64] over the MCU-padded grid, a block in row-major (de-zigzagged) order; blocks of the
 * padding hold what the file codes for them.  qt[3 * 64]: the quantisation table of each component, row-major; zero
 * for components the file does not have. */
int fm_jpeg_entropy_decode(const uint8_t* data, size_t n, const struct fm_jpeg_info* info, int16_t* coef, uint16_t* qt);
/* The three host-frame entry points for an entropy-decoded JPEG frame; they mirror fm_frame_upload,
 * fm_frame_upload_ahead and fm_frame_ring_store (and their _nv12 forms) one for one: same slots, same streams, same
 * events.  2 * coef_count + 384 bytes cross to the device -- into a staging buffer per entry point / look-ahead slot,
 * allocated on its first JPEG use for the largest layout of the configured frame size and freed by fm_frame_configure
 * and fm_ctx_destroy --; `coef` and `qt` inside a buffer from fm_host_alloc are copied from where they are (one copy
 * when qt == coef + coef_count), otherwise through a page-locked staging buffer allocated likewise.  Two kernels on
 * the copy's stream (csrc/jpeg.hip) then write the BGR frame where the BGR call would have put it; a look-ahead slot's
 * completion event follows them.  From there on the frame is an ordinary BGR frame.
 * FM_ERR_ARG when info's width x height is not the configured frame size, when info is not a supported layout that
 * fm_jpeg_info could have returned, or for a bad k / index; nothing is copied or launched then.  The kernels read no
 * address that depends on a coefficient's value: no coefficient values make them fault (the pixels of streams that no
 * 8-bit encoder produces are unspecified). */
int fm_frame_upload_jpeg(fm_ctx* ctx, const struct fm_jpeg_info* info, const int16_t* coef, const uint16_t* qt);
int fm_frame_upload_ahead_jpeg(fm_ctx* ctx, int k, const struct fm_jpeg_info* info, const int16_t* coef, const uint16_t* qt);
int fm_frame_ring_store_jpeg(fm_ctx* ctx, int index, const struct fm_jpeg_info* info, const int16_t* coef, const uint16_t* qt);

/* Frames at capture resolution (the reference's VideoIO resizes every captured frame to `size` with cv2.resize before
 * the tracker sees it, fastmot/videoio.py; its default configuration is 1280 x 720 from 1920 x 1080 sources).  One
 * described-source family: `src` says what the host frame is -- packed BGR, NV12 planes or an entropy-decoded JPEG, the
 * arguments of the calls above -- and how large it is.  The three calls mirror fm_frame_upload, fm_frame_upload_ahead and
 * fm_frame_ring_store one for one: same slots, same streams, same syncs, same events.
 * width x height equal to the configured frame size: the call IS its counterpart above (it forwards to it).
 * Otherwise the frame crosses to the device at its own resolution -- into buffers per entry point / look-ahead slot
 * (the source's BGR frame of width * height * 3 bytes, NV12 / JPEG staging and page-locked staging sized by the SOURCE
 * size, separate from the staging of the calls above), allocated on first use, regrown when a larger source arrives and
 * freed by fm_frame_configure and fm_ctx_destroy --, the NV12 / JPEG kernels write the BGR frame at that resolution, and
 * a kernel on the same stream (csrc/resize.hip) writes the configured-size BGR frame where the BGR call would have
 * put it; a look-ahead slot's completion event follows that last kernel.  From there on the frame is an ordinary BGR
 * frame: every stage reads the resized frame, as the reference's stages do.
 * The resize is cv2.resize's 8-bit INTER_LINEAR, integer and exact (fastmot_amd/videoio.py resize_bgr states it in
 * numpy).  Per axis, for output index d:
 *   f = float((d + 0.5) * (ssize / dsize) - 0.5), s = floor(f), f -= s; s < 0: s = 0, f = 0; s >= ssize - 1: s = ssize - 1, f = 0
 *   a0 = rint((1 - f) * 2048), a1 = rint(f * 2048), s' = min(s + 1, ssize - 1)
 * and per channel  S0 = p[y][x] ax0 + p[y][x'] ax1,  S1 = p[y'][x] ax0 + p[y'][x'] ax1,
 *   v = clamp((((ay0 * (S0 >> 4)) >> 16) + ((ay1 * (S1 >> 4)) >> 16) + 2) >> 2, 0, 255);
 * a source of exactly twice the frame size in both axes gives the rounded 2 x 2 mean (a + b + c + d + 2) >> 2 instead.
 * FM_ERR_ARG for a null ctx / src / plane pointer, an unknown kind, a width or height outside 1..16384, NV12 with an odd
 * source size, pitch < width or an unknown matrix, a JPEG info that is not a supported layout of width x height, or a
 * bad k / index; nothing is copied, allocated or launched then. */
#define FM_SRC_BGR 0
#define FM_SRC_NV12 1
#define FM_SRC_JPEG 2
#define FM_SRC_MAX_DIM 16384
struct fm_frame_src {
    int32_t kind, width, height;          /* FM_SRC_*; the SOURCE's size */
    const uint8_t* bgr;                   /* FM_SRC_BGR: packed, width * height * 3 bytes */
    const uint8_t *y, *uv;                /* FM_SRC_NV12: as fm_frame_upload_nv12's */
    int32_t pitch, matrix;
    const struct fm_jpeg_info* info;      /* FM_SRC_JPEG: as fm_frame_upload_jpeg's; info->width / height == width / height */
    const int16_t* coef;
    const uint16_t* qt;
};
int fm_frame_upload_src(fm_ctx* ctx, const struct fm_frame_src* src);
int fm_frame_upload_ahead_src(fm_ctx* ctx, int k, const struct fm_frame_src* src);
int fm_frame_ring_store_src(fm_ctx* ctx, int index, const struct fm_frame_src* src);

/* Planar YCbCr frames (what software decoders -- libavcodec, libvpx, dav1d -- hand out, and the payload of a YUV4MPEG2
 * '.y4m' frame): replaces, for a video file or pipe, the reference's cv2.VideoCapture with its `videoconvert` stage
 * (fastmot/videoio.py:73-75,156-170), whose decoder output is converted to BGR on the host.  A Y plane of `height` rows
 * of `width` samples at `y`, rows `pitch_y` >= width bytes apart, and U and V planes at `u`, `v`, rows `pitch_c` apart,
 * of     FM_YUV_420: ceil(width / 2) x ceil(height / 2)      FM_YUV_422: ceil(width / 2) x height
 *        FM_YUV_444: width x height                          FM_YUV_MONO: none (u, v may be null; U = V = 128)
 * samples; odd sizes are legal.  Pixel (r, c) uses the chroma sample (r >> sv, c >> sh): nearest replication, no siting
 * filter, as fm_frame_upload_nv12; the per-pixel arithmetic, the two limited-range matrices and their ids
 * (FM_NV12_BT601 / FM_NV12_BT709) are that call's.
 * The three calls mirror fm_frame_upload_nv12, fm_frame_upload_ahead_nv12 and fm_frame_ring_store_nv12 one for one:
 * same slots, same streams, same syncs, same events.  The rows are packed to their width on the way into page-locked
 * staging (one surface -- pitch_y == width, pitch_c == the chroma width, U right behind Y and V right behind U -- inside
 * a buffer from fm_host_alloc is copied from where it lies, in one copy); the device staging per entry point /
 * look-ahead slot is allocated on its first planar use and freed by fm_frame_configure and fm_ctx_destroy; a kernel on
 * the copy's stream (csrc/yuv.hip) writes the BGR frame where the BGR call would have put it.  width x height other than
 * the configured frame size: the frame takes the route of fm_frame_upload_src -- that family's buffers, grown and freed
 * by its rules; the kernel writes the source-size BGR frame and csrc/resize.hip the frame.
 * FM_ERR_ARG for a null ctx / f / plane pointer, an unknown chroma or matrix, a pitch below the plane's width, a width or
 * height outside 1..FM_SRC_MAX_DIM, or a bad k / index; nothing is copied, allocated or launched then. */
#define FM_YUV_420 0
#define FM_YUV_422 1
#define FM_YUV_444 2
#define FM_YUV_MONO 3
struct fm_frame_planar {
    int32_t width, height, chroma, matrix;    /* FM_YUV_*, FM_NV12_BT601 / FM_NV12_BT709 */
    const uint8_t *y, *u, *v;
    int32_t pitch_y, pitch_c;
};
int fm_frame_upload_planar(fm_ctx* ctx, const struct fm_frame_planar* f);
int fm_frame_upload_ahead_planar(fm_ctx* ctx, int k, const struct fm_frame_planar* f);
int fm_frame_ring_store_planar(fm_ctx* ctx, int index, const struct fm_frame_planar* f);

/* Packed frames: packed 4:2:2 (the raw format of every UVC / V4L2 camera and of most capture cards) and packed RGB in
 * any channel order with or without a fourth byte (what image libraries hand out; BGRx is what `nvvidconv` / `appsink`
 * do): replaces the host `videoconvert` of the reference's V4L2 and CSI pipelines (fastmot/videoio.py) and the channel
 * shuffle an application does on its capture thread.  `height` rows at `data`, `pitch` bytes apart, each of
 *   FM_PACKED_RGB / _BGR: 3 width bytes, R (B) first      FM_PACKED_RGBX / _BGRX: 4 width bytes, the fourth byte ignored
 *   FM_PACKED_XRGB / _XBGR: 4 width bytes, the first byte ignored
 *   FM_PACKED_YUY2 / _UYVY / _YVYU: 4 ceil(width / 2) bytes, macropixels Y0 U Y1 V / U Y0 V Y1 / Y0 V Y1 U
 * The RGB family is a byte permutation into B, G, R (`matrix` is checked but not used).  A macropixel carries two
 * horizontally adjacent pixels; an odd width is legal, the last macropixel's second luma byte is then no pixel.  Pixel
 * (r, c) uses luma sample c of its row and the U, V of macropixel c >> 1 (nearest replication, as FM_YUV_422), with
 *   FM_PACKED_BT601 / FM_PACKED_BT709: fm_frame_upload_nv12's limited-range arithmetic and constants
 *   FM_PACKED_BT601_FULL / _BT709_FULL: y = Y << 20, u = U - 128, v = V - 128, h = 1 << 19,
 *     R = sat8((y + h + CVR v) >> 20)   G = sat8((y + h + CVG v + CUG u) >> 20)   B = sat8((y + h + CUB u) >> 20)
 *     BT.601: CVR 1470104, CUB 1858077, CUG -360853, CVG -748826      (round(c * 2^20) of 1.402, 1.772, -0.344136, -0.714136)
 *     BT.709: CVR 1651297, CUB 1945738, CUG -196423, CVG -490864      (of 1.5748, 1.8556, -0.187324, -0.468124)
 * integer and exact (fastmot_amd/utils/packed.py packed_to_bgr states it in numpy).  The matrix ids are this family's
 * own; the NV12 / planar / src calls accept theirs as before.
 * The three calls mirror fm_frame_upload_planar, fm_frame_upload_ahead_planar and fm_frame_ring_store_planar one for
 * one: same slots, same streams, same syncs, same events.  The rows are packed to their byte width on the way into
 * page-locked staging (a surface with pitch == that width inside a buffer from fm_host_alloc is copied from where it
 * lies); the device staging per entry point / look-ahead slot is allocated on its first packed use and freed by
 * fm_frame_configure and fm_ctx_destroy (the page-locked staging is fm_frame_upload_src's, with its rules); a kernel
 * on the copy's stream (csrc/packed.hip) writes the BGR frame where the BGR call would have put it, and a look-ahead
 * slot's completion event follows it.  width x height other than the configured frame size: the frame takes the route
 * of fm_frame_upload_src -- that family's buffers, grown and freed by its rules; the kernel writes the source-size BGR
 * frame and csrc/resize.hip the frame.
 * FM_ERR_ARG for a null ctx / f / data pointer, an unknown format or matrix (2..15 are none), a pitch below the row's
 * byte width, a width or height outside 1..FM_SRC_MAX_DIM, or a bad k / index; nothing is copied, allocated or
 * launched then. */
#define FM_PACKED_RGB 0
#define FM_PACKED_BGR 1
#define FM_PACKED_RGBX 2
#define FM_PACKED_BGRX 3
#define FM_PACKED_XRGB 4
#define FM_PACKED_XBGR 5
#define FM_PACKED_YUY2 6
#define FM_PACKED_UYVY 7
#define FM_PACKED_YVYU 8
#define FM_PACKED_BT601 0
#define FM_PACKED_BT709 1
#define FM_PACKED_BT601_FULL 16
#define FM_PACKED_BT709_FULL 17
struct fm_frame_packed {
    int32_t format, width, height, pitch, matrix;    /* FM_PACKED_* layout, FM_PACKED_BT* */
    const uint8_t* data;
};
int fm_frame_upload_packed(fm_ctx* ctx, const struct fm_frame_packed* f);
int fm_frame_upload_ahead_packed(fm_ctx* ctx, int k, const struct fm_frame_packed* f);
int fm_frame_ring_store_packed(fm_ctx* ctx, int index, const struct fm_frame_packed* f);

/* Bayer frames: the raw colour-filter mosaic of an industrial or embedded camera (GigE Vision / USB3 Vision BayerRG8 /
 * BayerRG12, V4L2 SRGGB8 / SRGGB10, CSI sensors), one sample per pixel: replaces the demosaicing an application does on
 * its capture thread (the reference's pipelines get BGR from `videoconvert` / `nvvidconv`) and the 3 bytes per pixel
 * it uploads afterwards.  `height` rows of `width` samples at `data`, `pitch` BYTES apart; a sample is one byte for
 * `depth` 8 and a little-endian 16-bit word with the value in its low bits for `depth` 10, 12, 14 and 16 (the unpacked
 * form of SRGGB10 / BayerRG12; `data` and `pitch` need no alignment).
 *   pattern: where R sits in the 2 x 2 tile -- bit 0 its column parity, bit 1 its row parity; B sits at the opposite
 *     parity in both directions, G at the other two positions: FM_BAYER_RGGB 0, _GRBG 1, _GBRG 2, _BGGR 3
 *   sample preparation, before any interpolation: v = max(s - black, 0), p = min(255, (v * gain + (1 << (depth - 1))) >> depth)
 *     with the gain (1/256 units: 256 is 1.0) of the colour the sample's position carries; p == s for black 0, gains 256
 *     and depth 8
 *   borders: reflect-101 on the index in both directions (m = 2 (n - 1), i <- i mod m, i <- m - i where i >= n): m is
 *     even, so a reflected index keeps its colour -- which takes two samples each way, hence width, height >= 2; odd
 *     sizes are legal
 *   a position's own colour is p; with c the centre, card = N + S + E + W, hor = E + W, ver = N + S, diag the four
 *   diagonals, h2 / v2 the two samples at distance 2 horizontally / vertically:
 *   FM_BAYER_BILINEAR: G at R / B (card + 2) >> 2; R / B at G (a + b + 1) >> 1 of that colour's two neighbours; R at B and
 *     B at R (diag + 2) >> 2
 *   FM_BAYER_MHC (Malvar-He-Cutler, gradient-corrected, in sixteenths): sat8((sum + 8) >> 4) of
 *     G at R / B: 8 c + 4 card - 2 (h2 + v2)              R at B, B at R: 12 c + 4 diag - 3 (h2 + v2)
 *     R / B at G, that colour left and right: 10 c + 8 hor - 2 diag - 2 h2 + v2;  above and below: 10 c + 8 ver - 2 diag - 2 v2 + h2
 * integer and exact (fastmot_amd/utils/bayer.py bayer_to_bgr states it in numpy).
 * The three calls mirror fm_frame_upload_packed, fm_frame_upload_ahead_packed and fm_frame_ring_store_packed one for
 * one: same slots, same streams, same syncs, same events.  The rows cross as they lie, width or 2 width bytes each,
 * packed to that width on the way -- through page-locked staging (fm_frame_upload_src's, with its rules) only when the
 * source is pageable or pitched: a surface with pitch == its row bytes inside a buffer from fm_host_alloc is copied from
 * where it lies; the device staging per entry point / look-ahead slot is allocated on its first Bayer use and freed by
 * fm_frame_configure and fm_ctx_destroy; a kernel on the copy's stream (csrc/bayer.hip) writes the BGR frame where the BGR
 * call would have put it, and a look-ahead slot's completion event follows it.  width x height other than the
 * configured frame size: the frame takes the route of fm_frame_upload_src -- that family's buffers; the kernel writes
 * the source-size BGR frame and csrc/resize.hip the frame.
 * FM_ERR_ARG for a null ctx / f / data pointer, a pattern, method or depth outside their sets, a width or height outside
 * 2..FM_SRC_MAX_DIM, a pitch below the row's bytes, a gain outside 1..4096, a black level outside 0..2^depth - 1, or a
 * bad k / index; nothing is copied, allocated or launched then. */
#define FM_BAYER_RGGB 0
#define FM_BAYER_GRBG 1
#define FM_BAYER_GBRG 2
#define FM_BAYER_BGGR 3
#define FM_BAYER_BILINEAR 0
#define FM_BAYER_MHC 1
struct fm_frame_bayer {
    int32_t pattern, width, height, pitch, depth, method, black, gain_r, gain_g, gain_b;   /* FM_BAYER_*; pitch in bytes */
    const uint8_t* data;
};
int fm_frame_upload_bayer(fm_ctx* ctx, const struct fm_frame_bayer* f);
int fm_frame_upload_ahead_bayer(fm_ctx* ctx, int k, const struct fm_frame_bayer* f);
int fm_frame_ring_store_bayer(fm_ctx* ctx, int index, const struct fm_frame_bayer* f);

/* Deep YCbCr frames, 9 to 16 bits per sample in 16-bit little-endian words: what a hardware HEVC / AV1 Main10 decoder
 * delivers (P010 / P012 / P016), what libavcodec's yuv420p10le and a YUV4MPEG2 'C420p10' frame hold, the rule for 4K
 * cameras and HDR material: replaces the narrowing to 8 bits and the conversion to BGR that an application does in
 * host arithmetic on its capture thread (the reference's pipelines get 8-bit BGR from `videoconvert` / `nvvidconv`,
 * fastmot/videoio.py) and the 3 bytes per pixel it uploads afterwards.
 *   FM_DEEP_PLANAR: fm_frame_planar's planes and chroma layouts (FM_YUV_*) with 16-bit samples, the value in the LOW
 *     `depth` bits; the bits above them are masked off.  Any size from 1 x 1.
 *   FM_DEEP_SEMIPLANAR: a Y plane and, at `u`, a plane of height / 2 rows of width words, U and V interleaved (`v` is
 *     null, `chroma` is FM_YUV_420, width and height are even); the value in the HIGH `depth` bits, sample =
 *     word >> (16 - depth), the low bits are ignored.
 * Rows are `pitch_y` / `pitch_c` BYTES apart: even, and at least 2 x the plane's width in samples (for the semi-planar
 * UV plane: 2 width).  The planes need no alignment.  Pixel (r, c) uses the chroma sample (r >> sv, c >> sh) as
 * fm_frame_upload_planar.  With d = depth, s = d - 8, limited range:
 *   y = max(Y - (16 << s), 0) CY, u = U - (128 << s), v = V - (128 << s), h = 1 << (19 + s)
 *   R = sat8((y + h + CVR v) >> (20 + s))   G = sat8((y + h + CVG v + CUG u) >> (20 + s))   B = sat8((y + h + CUB u) >> (20 + s))
 * in 64-bit integers (the sums reach 2^37.2 at depth 16), arithmetic shifts, integer and exact
 * (fastmot_amd/utils/deep.py deep_to_bgr states it in numpy).  For samples that are 8-bit samples shifted left by s it
 * is fm_frame_upload_nv12's result bit for bit.  The matrix ids are this family's own:
 *   FM_DEEP_BT601 / FM_DEEP_BT709: fm_frame_upload_nv12's constants
 *   FM_DEEP_BT2020 (non-constant luminance, Kr 0.2627, Kb 0.0593): CY 1220945, CVR 1760217, CUB 2245811, CUG -196426, CVG -682019
 * Full range, transfer functions (PQ / HLG), big-endian samples, P210 / P410 and packed 10-bit words are not read.
 * The three calls mirror fm_frame_upload_planar, fm_frame_upload_ahead_planar and fm_frame_ring_store_planar one for
 * one: same slots, same streams, same syncs, same events, same trace marks, the same rule while a correction map is
 * set.  The rows are packed to their width on the way into page-locked staging (one surface -- every pitch twice the
 * plane's width, U right behind Y and V right behind U -- inside a buffer from fm_host_alloc is copied from where it
 * lies, in one copy).  A deep frame is up to 6 bytes per pixel (4:4:4), more than the BGR-sized staging of the slots
 * holds, so this family has staging of its own per entry point / look-ahead slot, on the device and page-locked,
 * allocated on first use, regrown when a larger frame arrives (after the stream that uses it is idle) and freed by
 * fm_frame_configure and fm_ctx_destroy; a kernel on the copy's stream (csrc/deep.hip) writes the BGR frame where the
 * BGR call would have put it, and a look-ahead slot's completion event follows it.  width x height other than the
 * configured frame size: the kernel writes the source-size BGR frame into fm_frame_upload_src's buffer and
 * csrc/resize.hip -- csrc/remap.hip while a correction map is set -- the frame.
 * FM_ERR_ARG for a null ctx / f / plane pointer, a depth outside 9..16, an unknown layout, chroma or matrix, a pitch
 * that is odd or below twice the plane's width, a width or height outside 1..FM_SRC_MAX_DIM, a semi-planar frame that
 * is not FM_YUV_420 or has an odd width or height, or a bad k / index; nothing is copied, allocated or launched then. */
#define FM_DEEP_PLANAR 0
#define FM_DEEP_SEMIPLANAR 1
#define FM_DEEP_BT601 0
#define FM_DEEP_BT709 1
#define FM_DEEP_BT2020 2
struct fm_frame_deep {
    int32_t width, height, chroma, matrix, depth, layout;    /* FM_YUV_*, FM_DEEP_BT*, 9..16, FM_DEEP_PLANAR / _SEMIPLANAR */
    const uint8_t *y, *u, *v;                                 /* FM_DEEP_SEMIPLANAR: u is the UV plane, v null */
    int32_t pitch_y, pitch_c;                                 /* bytes */
};
int fm_frame_upload_deep(fm_ctx* ctx, const struct fm_frame_deep* f);
int fm_frame_upload_ahead_deep(fm_ctx* ctx, int k, const struct fm_frame_deep* f);
int fm_frame_ring_store_deep(fm_ctx* ctx, int index, const struct fm_frame_deep* f);

/* Frames that already lie in GPU memory: a hardware decoder's NV12 surface (VCN / rocDecode), the output of
 * torchvision.io.decode_jpeg(device='cuda'), a torch / CuPy preprocessing pipeline, a GPU ISP, another model's output.
 * Every call above takes host pointers; these three take DEVICE pointers, copy nothing across PCIe and make no host
 * copy: a kernel of csrc/devsrc.hip reads the caller's memory where it lies and writes the BGR frame.
 *   FM_DEV_HWC, FM_DEV_U8: plane[0] holds `height` rows, pitch[0] bytes apart, of `width` pixels of 3 or 4 bytes;
 *     `format` is one of the RGB-family ids of fm_frame_packed (FM_PACKED_RGB .. FM_PACKED_XBGR) and the frame equals
 *     fm_frame_upload_packed's of the same bytes.
 *   FM_DEV_CHW: plane[0..2] hold one channel each, `height` rows of `width` elements, pitch[c] bytes apart, in the
 *     order `format` names (FM_DEV_ORDER_RGB: R, G, B; FM_DEV_ORDER_BGR: B, G, R).  FM_DEV_U8: a channel permutation.
 *     FM_DEV_F16 / FM_DEV_F32: v = (float)x * scale in float32 -- one multiply, not fused with anything --,
 *     rintf(v) (half to even), NaN -> 0, clamped to 0..255; `scale` is 255.0f for values in [0, 1] and 1.0f for values
 *     in [0, 255].
 *   FM_DEV_NV12, FM_DEV_U8: plane[0] is the Y plane, plane[1] the interleaved UV plane of height / 2 rows, each with a
 *     pitch of its own; fm_frame_upload_nv12's arithmetic and `matrix` ids; width and height even.
 * Unused planes are NULL, an unused `format` (NV12) is 0; `matrix` is read for NV12 only, `scale` for the float types
 * only.  The kernels assume nothing about the source's alignment beyond the element size -- a view of a larger tensor
 * starts at any element and has any pitch --: they take 4- to 16-byte accesses where an address allows them and
 * elements otherwise.  fastmot_amd/utils/devarray.py to_bgr states the four conversions in numpy; the frame equals it
 * bit for bit.
 * The three calls mirror fm_frame_upload_packed, fm_frame_upload_ahead_packed and fm_frame_ring_store_packed one for
 * one: same slots, same streams, same syncs, same slot events, same rules under a correction map.  width x height equal
 * to the configured size: the kernel writes the frame itself; any other: it writes the source-size BGR frame of
 * fm_frame_upload_src's buffers and csrc/resize.hip (csrc/remap.hip) the frame.
 * Checks, all before anything is enqueued (FM_ERR_ARG, nothing recorded, waited for or launched):
 *   fm_frame_device_check (host only, no HIP call; the entry points call it first): width and height in
 *     1..FM_SRC_MAX_DIM, even for NV12; a known layout, a dtype and a format that go with it; used planes non-null,
 *     unused ones null; every pitch at least the row's bytes and at most 2^40; pointers and pitches multiples of the
 *     element size; scale 1 or 255 for the float types; no flag but FM_DEV_READY.
 *   per plane: hipPointerGetAttributes must say device memory of the context's device -- host, page-locked, managed and
 *     other-device pointers are refused (hand those to the host calls above) --, and where hipMemGetAddressRange answers
 *     the plane's whole extent, pitch * (rows - 1) + row bytes, must lie inside that allocation.  Where it cannot answer
 *     (memory of a virtual-memory allocator: hipMemCreate / hipMemMap, torch's expandable segments) the attributes alone
 *     decide, and the extent is the caller's word.
 * Ordering: unless FM_DEV_READY is set, the call records a per-slot event on `stream` -- the stream the producer's work
 * was enqueued on, NULL for the null stream -- and the library's stream waits for it before the kernel reads (no wait is
 * enqueued when the host already sees the event complete).  FM_DEV_READY: the data is complete, e.g. after a
 * synchronise; nothing is recorded.
 * Lifetime: the caller's memory is read by the conversion kernel only, not by the resize.  fm_frame_upload_device and
 * fm_frame_ring_store_device are synchronous like their siblings: the source is consumed on return.
 * fm_frame_upload_ahead_device returns a ticket (> 0) in *ticket (which may be null); fm_frame_device_done(ctx, ticket,
 * wait) says whether that frame's source has been consumed -- 1: yes, the memory may be overwritten or freed; 0: still
 * being read (never with `wait` != 0, which blocks until it is) --, FM_ERR_ARG for a ticket never handed out.  The
 * context keeps the last FM_DEV_TICKETS tickets' events; older ones are consumed by construction (a ticket's event is
 * waited for before its place is reused), and fm_ctx_destroy waits for all of them. */
#define FM_DEV_HWC 0
#define FM_DEV_CHW 1
#define FM_DEV_NV12 2
#define FM_DEV_U8 0
#define FM_DEV_F16 1
#define FM_DEV_F32 2
#define FM_DEV_ORDER_RGB 0
#define FM_DEV_ORDER_BGR 1
#define FM_DEV_READY 1
#define FM_DEV_TICKETS 16
struct fm_frame_device {
    const void* plane[3];   /* device pointers; unused planes NULL */
    int64_t     pitch[3];   /* bytes between rows of each plane */
    int32_t     width, height;
    int32_t     layout;     /* FM_DEV_HWC | FM_DEV_CHW | FM_DEV_NV12 */
    int32_t     dtype;      /* FM_DEV_U8 | FM_DEV_F16 | FM_DEV_F32 (F16/F32: CHW only) */
    int32_t     format;     /* HWC: the RGB-family ids of fm_frame_packed (bgr, rgb, bgrx, rgbx, xrgb, xbgr);
                               CHW: FM_DEV_ORDER_RGB | FM_DEV_ORDER_BGR */
    int32_t     matrix;     /* NV12: the matrix ids of fm_frame_upload_nv12 */
    float       scale;      /* float dtypes: 255.0f for values in [0,1], 1.0f for values in [0,255] */
    void*       stream;     /* producer's hipStream_t (NULL = the null stream) */
    int32_t     flags;      /* FM_DEV_READY: the data is complete, wait for nothing */
};
int fm_frame_upload_device(fm_ctx* ctx, const struct fm_frame_device* f);
int fm_frame_upload_ahead_device(fm_ctx* ctx, int k, const struct fm_frame_device* f, uint64_t* ticket);
int fm_frame_ring_store_device(fm_ctx* ctx, int index, const struct fm_frame_device* f);
int fm_frame_device_done(fm_ctx* ctx, uint64_t ticket, int wait);  /* 1 consumed, 0 still being read, <0 error */
int fm_frame_device_check(const struct fm_frame_device* f);        /* host-only geometry check, no HIP call */

/* Geometry between sensor and tracker: lens undistortion, or any fixed correction that is one map (a rotation by 90
 * degrees, a mirror, a perspective crop), applied by the gather that already ends every described-source call.  A map
 * holds, for every pixel of the configured width x height frame, a source coordinate in fixed point with 5 fractional
 * bits: `xy` is int32 [height][width][2], X = rint(32 x), Y = rint(32 y), X in [-64, 32 (src_w + 1)], Y in
 * [-64, 32 (src_h + 1)] (-64: fully outside).  With ix = X >> 5 (arithmetic), fx = X & 31 and the same for y, the four
 * taps are (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1); a tap outside [0, src_w) x [0, src_h) contributes the
 * channel of `border_bgr`, chosen per tap, and per channel
 *   v = ((32 - fy) ((32 - fx) p00 + fx p01) + fy ((32 - fx) p10 + fx p11) + 512) >> 10
 * -- exact in 32 bits, the float64 bilinear value of the quantised coordinate rounded half up (csrc/remap_pixel.h: one
 * text for the kernel of csrc/remap.hip and for fm_remap_bgr_host; fastmot_amd/utils/lens.py remap_bgr in numpy).  It
 * is NOT the resize's arithmetic: an identity-geometry map gives pixels near fm_frame_upload_src's, not equal to them.
 * fm_frame_remap_set is set-up work: it checks every entry's range on the host, waits for the detector stream, the
 * ReID stream and the null stream (those whose queued kernels may still read the previous map) and uploads a copy of
 * the map for the configured frame size.  FM_ERR_ARG, with the previous map untouched, for a null pointer, no configured
 * frame, src_w / src_h outside 1..FM_SRC_MAX_DIM or an entry out of range.  fm_frame_remap_clear, fm_frame_configure
 * and fm_ctx_destroy drop the map.
 * While a map is set the described-source calls -- fm_frame_upload_src / _ahead_src / _ring_store_src and their
 * _planar, _packed, _bayer, _deep and _device forms -- take sources of src_w x src_h only (FM_ERR_ARG for any other, nothing copied or
 * launched), stage them at that size even when it is the configured one, and end in the remap kernel where they end in
 * the resize kernel without a map: same slots, streams, syncs, events and trace marks.  Every other call, and every
 * call while no map is set, is untouched.  A per-stream setting: it may change, it should not alternate per frame.
 * fm_remap_bgr_host: the same arithmetic on host pixels (src_w x src_h packed BGR -> width x height packed BGR, both
 * within 1..FM_SRC_MAX_DIM), compiled from the kernel's text; no context, no GPU, any number of threads.  FM_ERR_ARG for
 * a null pointer, a size out of range or a map entry out of range. */
int fm_frame_remap_set(fm_ctx* ctx, int src_w, int src_h, const int32_t* xy, const uint8_t border_bgr[3]);
int fm_frame_remap_clear(fm_ctx* ctx);
int fm_remap_bgr_host(const uint8_t* src, int src_w, int src_h, const int32_t* xy, uint8_t* dst, int width, int height,
                      const uint8_t border_bgr[3]);

/* Frames OUT as baseline JPEG (an output 'out/%06d.jpg' or 'out.mjpeg'): replaces the Pillow save of
 * fastmot_amd/videoio.py's writer and, in the reference, cv2.VideoWriter (fastmot/videoio.py).  The device does
 * everything that is per pixel or per coefficient (csrc/jpegenc.hip): BGR -> YCbCr, edge replication to the 16 x 16 MCU
 * grid, 2 x 2 chroma averaging, forward DCT, quantisation, Huffman coding and 0xFF byte stuffing; the host writes the
 * marker segments and concatenates the entropy-coded segments (csrc/jpegenc_host.hip).  Only compressed bytes cross to
 * the host.
 * The file: JFIF, 8-bit, three components YCbCr 4:2:0, the Annex-K quantisation tables scaled by `quality` with
 * libjpeg's rule (s = quality < 50 ? 5000 / quality : 200 - 2 quality; (base s + 50) / 100 clamped to 1..255), the
 * Annex-K Huffman tables, one interleaved scan, a restart interval of ONE MCU ROW (DRI = ceil(width / 16)): each MCU row
 * is an independent, byte-aligned segment, which is what lets the device code all of them at once.  Marker order: SOI,
 * APP0, DQT x 2, SOF0, DHT x 4, DRI, SOS -- Pillow's.  The arithmetic is libjpeg's, integer and exact (tests/jpegenc_ref.py
 * states it in numpy): the file equals the one Pillow (libjpeg-turbo) writes with subsampling 4:2:0, the same quality and
 * restart_marker_rows = 1 byte for byte, at sizes that are no multiple of 16 as well (the padded blocks).
 *   Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *   Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,  Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
 *   chroma sample = (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2 ... along the output columns; pixels right of the image
 *     repeat the last column, chroma rows below it repeat the last averaged row (luma rows the last pixel row)
 *   forward DCT: jfdctint's "islow" on samples - 128, rows first; quantised value = sign(c) ((|c| + 4 q) / (8 q))
 *   a luma block wholly right of / below the last block column / row that holds image pixels: AC 0, DC of the block before it
 *
 * fm_jpeg_encode_bound: the largest file a width x height frame can become (every byte of the scan stuffed), 0 for a
 * size outside 1..FM_SRC_MAX_DIM.  fm_jpeg_encode_tables: qt[128], the luminance then the chrominance table of a quality,
 * row-major.  fm_jpeg_encode_header: the marker segments SOI .. SOS.  fm_jpeg_encode_assemble: the whole file from the
 * ceil(height / 16) entropy-coded segments -- seg_len[r] bytes each, stuffed, segment r at the sum of the lengths before
 * it each rounded up to 16 inside segs[0, segs_bytes) -- with RST0..7 between them and EOI behind.  These four need no
 * fm_ctx and no GPU and may be called from any number of threads at once.
 * fm_frame_encode_jpeg: the frame the context currently holds on the device (whatever it was uploaded as: BGR, NV12,
 * JPEG, a resized source, a ring frame); nothing is uploaded.  fm_jpeg_encode_bgr: host pixels (width x height, `pitch`
 * bytes between rows; e.g. a frame with overlays drawn on it), through a device staging buffer; pixels inside a buffer
 * from fm_host_alloc with pitch = 3 width are copied from where they are, others through page-locked staging.
 * Both run on a stream of the encoder's own and wait for no pipeline stream, nor does any pipeline stream wait for the
 * encoder: the current frame is complete on the device when the call that made it current returned (the upload calls
 * and fm_frame_promote_next synchronise the stream that carried its copy / conversion / resize).
 * Both return when the file is complete in out[0, *length).  Working buffers (worst case: 208 bytes per 8 x 8 block
 * before stuffing, twice that after, the latter once more in page-locked memory) are allocated on first use, regrown for a
 * larger frame and freed by fm_ctx_destroy.  The caller must not upload the next current frame while fm_frame_encode_jpeg
 * runs (MOT.step and MOT.encode_frame are called from one thread).
 * FM_ERR_ARG for a quality outside 1..100, a width or height outside 1..FM_SRC_MAX_DIM, pitch < 3 width, no current
 * frame, a null pointer, or a capacity smaller than the file -- *length then says what it needs and nothing is written
 * past out + capacity.
 * fm_jpeg_encode_stream_ms: HIP-event time of the kernels (and, for fm_jpeg_encode_bgr, not the copy) of the last
 * encode of this context, -1 before the first. */
size_t fm_jpeg_encode_bound(int width, int height);
int fm_jpeg_encode_tables(int quality, uint16_t* qt);
int fm_jpeg_encode_header(int width, int height, int quality, uint8_t* out, size_t capacity, size_t* length);
int fm_jpeg_encode_assemble(int width, int height, int quality, const uint32_t* seg_len, const uint8_t* segs, size_t segs_bytes,
                            uint8_t* out, size_t capacity, size_t* length);
int fm_frame_encode_jpeg(fm_ctx* ctx, int quality, uint8_t* out, size_t capacity, size_t* length);
int fm_jpeg_encode_bgr(fm_ctx* ctx, const uint8_t* pixels, int width, int height, size_t pitch, int quality, uint8_t* out,
                       size_t capacity, size_t* length);
int fm_jpeg_encode_stream_ms(fm_ctx* ctx, float* ms);

/* Overlays ON the device frame (boxes, labels, trajectories, flow matches, covariance ellipses, the caption): replaces
 * Visualizer.render (fastmot_amd/utils/visualization.py; in the reference fastmot/utils/visualization.py on cv2) for a
 * frame whose pixels never were on the host.  The caller states the picture as a COMMAND LIST in painter's order -- a
 * later command paints over an earlier one --, a kernel (csrc/overlay.hip) applies the list to a COPY of the current
 * device frame, and that copy, the context's overlay buffer, is what fm_overlay_read downloads and
 * fm_overlay_encode_jpeg encodes.  The tracker's frame is never written: the next step's KLT and the ReID crops read it.
 * The rasterisation is Pillow's (ImageDraw of 12.2.0, which visualization.py draws with), restated in integers in
 * csrc/overlay_pixel.h -- one text for the kernel and for fm_overlay_render_host -- and in numpy in tests/overlay_ref.py:
 *   FM_OVL_RECT_FILL     every pixel of [x0, x1] x [y0, y1], corners inclusive; nothing when x1 < x0 or y1 < y0.
 *   FM_OVL_RECT_OUTLINE  `thickness` t rings growing INWARD: rows y0 + i and y1 - i over [x0, x1], and columns x0 + i and
 *                        x1 - i (i < t) over the rows y0 + t .. y1 - t, or, when that range is empty (a box lower than
 *                        2 t), over y1 - t + 2 .. y0 + t: Pillow draws those columns as lines without their last point
 *                        from y0 + t towards y1 - t + 1, which is what makes a degenerate box spill past its corners.
 *   FM_OVL_LINE          Bresenham from (x0, y0) to (x1, y1), both ends drawn: x-major when |dx| > |dy|, else y-major;
 *                        i steps along the major axis from the START the minor offset is (2 minor i + major) / (2 major)
 *                        in integer division (the closed form of the error term e = 2 minor - major, step when e >= 0).
 *   FM_OVL_DOT           the five pixels (x0, y0), (x0 +- 1, y0), (x0, y0 +- 1): Pillow's ellipse of radius 1.
 *   FM_OVL_MASK          an 8-bit alpha mask of x1 columns by y1 rows (row-major at masks + mask_off) with its top left
 *                        pixel at (x0, y0), blended per channel: t = m ink + (255 - m) bg + 128, (t + (t >> 8)) >> 8.
 *                        Text arrives this way (the glyph mask of the caller's font): the library knows no font.
 * Colours are B, G, R.  Coordinates may lie anywhere in +-FM_OVERLAY_MAX_COORD, inside the frame or not; pixels
 * outside it are clipped, intermediate products are 64-bit.
 *
 * fm_overlay_check: 0 when the list is well formed for a width x height frame; FM_ERR_ARG for a null list with n > 0, a
 * null blob with mask_bytes > 0, n > FM_OVERLAY_MAX_CMDS, mask_bytes > FM_OVERLAY_MAX_MASK_BYTES, a width or height
 * outside 1..FM_SRC_MAX_DIM, an unknown kind, a thickness outside 1..8 (FM_OVL_RECT_OUTLINE), a coordinate outside
 * +-FM_OVERLAY_MAX_COORD, a mask whose columns or rows are negative or above FM_OVERLAY_MAX_COORD or whose x1 * y1 bytes
 * do not lie inside [mask_off, mask_bytes).  It reads the list only, needs no context and no GPU and may be called from
 * any number of threads; every entry point below calls it first and does nothing else when it fails.
 * fm_overlay_render_host: applies the list IN PLACE to host pixels (width x height BGR, `pitch` >= 3 width bytes between
 * rows) with the functions of overlay_pixel.h: the CPU statement of the kernel's arithmetic.  No context, no GPU.
 * fm_frame_render_overlay: current device frame + list -> the context's overlay buffer (n == 0: a copy).  One kernel:
 * a workgroup owns a 64 x 16 tile, bins the list against it 256 commands at a time in list order and applies the hits
 * to its pixels in registers; every pixel is read once and written once.  The list and the masks travel through
 * page-locked staging of the context; staging, device copies and the overlay buffer (3 width height bytes) are allocated
 * on first use, regrown on demand and freed by fm_ctx_destroy.  Everything runs on the JPEG encoder's stream (created on
 * first use, as by fm_frame_encode_jpeg), so a following fm_overlay_encode_jpeg is ordered behind it; no pipeline
 * stream waits or is waited for -- fm_frame_encode_jpeg's argument for why the current frame is complete holds
 * unchanged.  Returns when the buffer is complete.  FM_ERR_ARG without a current frame.
 * fm_overlay_read: the overlay buffer -> out[3 width height]; FM_ERR_ARG before the first render at the current frame
 * size.  fm_overlay_encode_jpeg: fm_frame_encode_jpeg's contract with the overlay buffer as the source.
 * fm_overlay_stream_ms: HIP-event time of the last render's kernel (not the copies of list and masks), -1 before the
 * first.  The caller must not upload the next current frame while fm_frame_render_overlay runs. */
#define FM_OVL_RECT_FILL 0
#define FM_OVL_RECT_OUTLINE 1
#define FM_OVL_LINE 2
#define FM_OVL_DOT 3
#define FM_OVL_MASK 4
#define FM_OVERLAY_MAX_CMDS 65536
#define FM_OVERLAY_MAX_MASK_BYTES (4u << 20)
#define FM_OVERLAY_MAX_COORD (1 << 20)
typedef struct fm_overlay_cmd {   /* 32 bytes */
    int32_t kind;                 /* FM_OVL_* */
    int32_t x0, y0, x1, y1;       /* see above; FM_OVL_MASK: x1 columns, y1 rows */
    uint8_t b, g, r;              /* colour; FM_OVL_MASK: the ink */
    uint8_t thickness;            /* FM_OVL_RECT_OUTLINE: 1..8; others: ignored */
    uint32_t mask_off;            /* FM_OVL_MASK: offset of the mask's first byte in the blob */
    int32_t reserved;             /* 0 */
} fm_overlay_cmd;
int fm_overlay_check(const fm_overlay_cmd* cmds, int n, const uint8_t* masks, size_t mask_bytes, int width, int height);
int fm_overlay_render_host(uint8_t* pixels, int width, int height, size_t pitch, const fm_overlay_cmd* cmds, int n,
                           const uint8_t* masks, size_t mask_bytes);
int fm_frame_render_overlay(fm_ctx* ctx, const fm_overlay_cmd* cmds, int n, const uint8_t* masks, size_t mask_bytes);
int fm_overlay_read(fm_ctx* ctx, uint8_t* out);
int fm_overlay_encode_jpeg(fm_ctx* ctx, int quality, uint8_t* out, size_t capacity, size_t* length);
int fm_overlay_stream_ms(fm_ctx* ctx, float* ms);

/* Redaction of the frames that leave the GPU (no counterpart in the reference): tracked persons are pixelated, smoothed
 * or painted over in the overlay buffer, inside the pass that makes it, so that the pictures fm_overlay_read,
 * fm_overlay_encode_jpeg and fm_frame_export_i420(FM_EXPORT_OVERLAY) hand out do not show them.  The tracker's frame is
 * never written: fm_frame_read, the next step's KLT and the ReID crops see the unredacted picture, by design.
 * A frame is redacted by a list of REGIONS.  A region has inclusive corners x0, y0, x1, y1 (anywhere in
 * +-FM_OVERLAY_MAX_COORD; empty when x1 < x0 or y1 < y0; width and height at most FM_SRC_MAX_DIM), a mode, a shape, a cell
 * side c in 2..256 and a fill colour.  Its pixels are the rectangle, cut by the frame and by the shape.  Everything is
 * integer and exact, stated once in csrc/redact_pixel.h -- one text for the kernels and for fm_redact_render_host -- and
 * in numpy in tests/redact_ref.py:
 *   cells   The grid is anchored at the UNCLIPPED corner: cell (i, j) covers the columns x0 + i c .. x0 + (i + 1) c - 1
 *           up to x1, and the rows likewise.  Its mean per channel is (sum + n / 2) / n in integer division over those n
 *           of its pixels that lie inside the frame -- the rectangle's pixels, whatever the shape.  Only cells with n > 0
 *           exist: indices imin..imax, jmin..jmax.
 *   FM_REDACT_PIXELATE  the pixel takes its cell's mean.
 *   FM_REDACT_SMOOTH    bilinear between the means of the four nearest cell centres: u = 2 (x - x0) + 1 - c,
 *                       i0 = floor(u / 2c), fx = u - 2c i0, the same in y for j0 and fy; i0, i0 + 1, j0, j0 + 1 clamped
 *                       into the existing range; value = ((2c - fx)(2c - fy) m00 + fx (2c - fy) m10 + (2c - fx) fy m01 +
 *                       fx fy m11 + 2c^2) / 4c^2 (below 2^27).  Only the cell means show, without the blocks.
 *   FM_REDACT_FILL      the colour (b, g, r).  Such a region has no cells.
 *   FM_REDACT_RECT      every pixel of the rectangle.
 *   FM_REDACT_ELLIPSE   a = x1 - x0 + 1, b = y1 - y0 + 1, dx = 2 (x - x0) + 1 - a, dy = 2 (y - y0) + 1 - b: inside iff
 *                       dx^2 b^2 + dy^2 a^2 <= a^2 b^2, in 64-bit integers.
 * Every region computes from the ORIGINAL frame, never from another region's output; a pixel that several regions cover
 * takes the value of the LAST of them in list order.  An overlay command list is applied on top of the redacted pixels.
 *
 * fm_redact_check: 0 when the list is well formed for a width x height frame; FM_ERR_ARG for a null list with n > 0,
 * n > FM_REDACT_MAX_REGIONS, a width or height outside 1..FM_SRC_MAX_DIM, an unknown mode or shape, a cell outside 2..256,
 * a non-empty region with a side above FM_SRC_MAX_DIM, a coordinate outside +-FM_OVERLAY_MAX_COORD, a non-zero reserved
 * field, or a list whose existing cells on that frame number more than FM_REDACT_MAX_CELLS in all (which sizes the device
 * buffer of the means).  Reads the list only; no context, no GPU, any number of threads.  Every entry point below calls
 * it first and does nothing else when it fails.
 * fm_redact_render_host: redacts host pixels (width x height BGR, `pitch` >= 3 width bytes between rows) IN PLACE, every
 * region reading a copy of the original taken first: the CPU statement of the kernels.  No context, no GPU.
 * fm_frame_render_redacted: current device frame -> the context's overlay buffer, redacted by the regions and then drawn
 * on by the command list (fm_frame_render_overlay's arguments and contract: the same stream, the same ordering, the same
 * buffer, which fm_overlay_read / fm_overlay_encode_jpeg / fm_frame_export_i420 then serve unchanged).  Two kernels: the
 * cell means of all regions in one launch (csrc/redact.hip) into a device buffer of one B, G, R, 0 word per cell behind
 * a per-region offset table, then the overlay tile pass, whose workgroup bins the regions against its tile as it bins
 * commands and replaces each pixel, read once, by its last covering region's value before the commands are applied.
 * With n_regions == 0 it is fm_frame_render_overlay, byte for byte.  List, table and means follow the overlay
 * buffers' rules: allocated on first use, regrown on demand, freed by fm_ctx_destroy.
 * fm_redact_stream_ms: HIP-event time of the last fm_frame_render_redacted's kernels, means and tile pass together
 * (fm_overlay_stream_ms: the tile pass alone); -1 before the first. */
#define FM_REDACT_PIXELATE 0
#define FM_REDACT_SMOOTH 1
#define FM_REDACT_FILL 2
#define FM_REDACT_RECT 0
#define FM_REDACT_ELLIPSE 1
#define FM_REDACT_MAX_REGIONS 4096
#define FM_REDACT_MAX_CELLS (1 << 20)
typedef struct fm_redact_region {   /* 32 bytes */
    int32_t x0, y0, x1, y1;         /* inclusive corners */
    int32_t mode;                   /* FM_REDACT_PIXELATE / SMOOTH / FILL */
    int32_t shape;                  /* FM_REDACT_RECT / ELLIPSE */
    int32_t cell;                   /* cell side c, 2..256 (checked for every mode) */
    uint8_t b, g, r;                /* FM_REDACT_FILL: the colour; others: ignored */
    uint8_t reserved;               /* 0 */
} fm_redact_region;
int fm_redact_check(const fm_redact_region* regions, int n, int width, int height);
int fm_redact_render_host(uint8_t* pixels, int width, int height, size_t pitch, const fm_redact_region* regions, int n);
int fm_frame_render_redacted(fm_ctx* ctx, const fm_redact_region* regions, int n_regions, const fm_overlay_cmd* cmds, int n_cmds,
                             const uint8_t* masks, size_t mask_bytes);
int fm_redact_stream_ms(fm_ctx* ctx, float* ms);

/* Frames OUT as planar I420 (a '.y4m' output, or the input of a software encoder): replaces, for such an output, the
 * reference's cv2.VideoWriter with its `autovideoconvert` stage (fastmot/videoio.py:99-103,222-232), which takes host
 * BGR pixels.  Output: width * height Y bytes, then ceil(width / 2) * ceil(height / 2) U bytes, then as many V bytes --
 * fm_i420_bound(width, height) in all (0 for a size outside 1..FM_SRC_MAX_DIM).  BT.601 limited range, integer and exact
 * (fastmot_amd/utils/yuv.py bgr_to_planar420 states it in numpy):
 *   Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16
 *   U = ((-38 R - 74 G + 112 B + 128) >> 8) + 128,  V = ((112 R - 94 G - 18 B + 128) >> 8) + 128   (arithmetic shifts)
 *   chroma sample = (the 2 x 2 block's four U (V) values + 2) >> 2; the column / row an odd size lacks is the last repeated.
 * fm_frame_export_i420: `which` = FM_EXPORT_FRAME, the frame the context currently holds on the device (whatever it was
 * uploaded as), or FM_EXPORT_OVERLAY, the context's overlay buffer after fm_frame_render_overlay; nothing is uploaded.
 * fm_i420_from_bgr: host pixels (`pitch` >= 3 width bytes between rows) through a device staging buffer, as
 * fm_jpeg_encode_bgr.  Both run on the JPEG encoder's stream (created on first use) under fm_frame_encode_jpeg's rules:
 * no pipeline stream waits or is waited for, the call returns when out[0, *length) is complete; the planes pass through
 * a device buffer and a page-locked buffer (skipped when `out` lies in fm_host_alloc memory), allocated on first use,
 * regrown for a larger frame, freed by fm_ctx_destroy.  The kernel (csrc/yuv.hip): one thread per 8 columns x 2 rows.
 * FM_ERR_ARG for a null pointer, an unknown `which`, no current frame / no overlay rendered at the current frame size,
 * a size outside 1..FM_SRC_MAX_DIM, pitch < 3 width, or capacity < the output -- *length then says what it needs and
 * nothing is written to out. */
#define FM_EXPORT_FRAME 0
#define FM_EXPORT_OVERLAY 1
size_t fm_i420_bound(int width, int height);
int fm_frame_export_i420(fm_ctx* ctx, int which, uint8_t* out, size_t capacity, size_t* length);
int fm_i420_from_bgr(fm_ctx* ctx, const uint8_t* pixels, int width, int height, size_t pitch, uint8_t* out, size_t capacity,
                     size_t* length);

/* Tracked OBJECTS out as JPEG crops (no counterpart in the reference): many rectangles of the picture the context holds,
 * each of its own size, become one baseline JPEG file each in ONE pass of the encoder -- the five launches of
 * fm_frame_encode_jpeg (csrc/jpegenc.hip: the same kernels, instantiated over a table of images where the whole frame is
 * one image found by index arithmetic), one small table upload and one prefix pass in front of the gather, one stream
 * synchronise, and only compressed bytes cross to the host.  The number of launches does not depend on n.
 * A rectangle has inclusive corners and lies inside the frame (the caller clips; utils/redact.py region_rect).  File i is
 * byte for byte what fm_jpeg_encode_bgr writes for the pixels [y0, y1] x [x0, x1] of the picture: the crop's own last
 * column / row is what pads it to the MCU grid, its own last averaged chroma row is what repeats below it, its dummy
 * blocks follow from its own size, and its restart markers start at RST0.
 * `shrink` s = 1, 2 or 4 reduces the crop first by an integer factor while the DCT kernel fetches its pixels (no reduced
 * picture is stored): output pixel (X, Y) of a w x h crop is, per channel, (sum + n / 2) / n in integer division over the
 * n crop pixels of [sX, sX + s) x [sY, sY + s) that lie inside the crop -- blocks at the right / lower edge average
 * fewer --, and the file is ceil(w / s) x ceil(h / s).
 * `which`: FM_EXPORT_FRAME, the current frame, or FM_EXPORT_OVERLAY, the overlay buffer after fm_frame_render_overlay /
 * fm_frame_render_redacted.
 *
 * fm_jpeg_encode_regions_plan (no context, no GPU, any number of threads): the layout of one call.  The index spaces of
 * the launches -- MCUs, 8 x 8 blocks (six per MCU) and MCU rows -- are the concatenation of all images' in list order;
 * plans[i] says where image i starts in each, where its first row lies in the row buffer (every row on a 16-byte
 * boundary of its own, sized for its own width, so that no two images share a word there) and what its file can take
 * at most; *totals sums them.  plans may be null.  FM_ERR_ARG, with fm_last_error naming the limit, for n < 0, a null
 * list with n > 0, a shrink other than 1 / 2 / 4, a rectangle with x0 < 0, y0 < 0, x1 < x0 or y1 < y0 or a side above
 * FM_SRC_MAX_DIM, n > FM_OBJENC_MAX_REGIONS, or more than FM_OBJENC_MAX_MCUS MCUs in all.  The latter bounds the working
 * memory of a call: about 7 KB per MCU (768 B coefficients, 24 B offsets, 1.25 KB unstuffed, 2.5 KB stuffed, 2.5 KB
 * page-locked), 16384 MCUs -- two 1080p frames' worth -- about 75 MB of device and 41 MB of page-locked memory, 116 MB together.
 * fm_jpeg_encode_regions_bound: the sum of the files' bounds (the capacity fm_frame_encode_regions asks for), 0 where
 * the plan fails.
 * fm_jpeg_encode_regions_assemble (no context, no GPU): the n files from the call's segments -- seg_len[r] bytes for
 * global MCU row r, segment r at the sum of the lengths before it each rounded up to 16 inside segs[0, segs_bytes) --
 * written one behind the other, file i at out[offsets[i], offsets[i + 1]).  Lengths that do not fit segs_bytes give
 * FM_ERR_ARG before anything is read; nothing is written past out + capacity.
 * fm_frame_encode_regions: plans, encodes and assembles.  Everything runs on the encoder's stream under
 * fm_frame_encode_jpeg's rules: no pipeline stream waits or is waited for, frames prefetched for later steps are
 * untouched, the call returns when the files are complete.  n == 0 succeeds with offsets[0] = 0 and enqueues nothing.
 * FM_ERR_ARG, before anything is enqueued, for what the plan refuses, a rectangle that reaches outside the frame, a
 * quality outside 1..100, an unknown `which`, no current frame / no overlay picture of the current frame size, a null
 * pointer, or a capacity below fm_jpeg_encode_regions_bound.  Buffers grow on demand as fm_frame_encode_jpeg's do
 * (they are the same buffers). */
#define FM_OBJENC_MAX_REGIONS 1024
#define FM_OBJENC_MAX_MCUS 16384
typedef struct fm_crop_rect {
    int32_t x0, y0, x1, y1;         /* inclusive corners, inside the frame */
} fm_crop_rect;
typedef struct fm_crop_plan {       /* 48 bytes */
    int32_t width, height;          /* of the file: ceil(w / shrink), ceil(h / shrink) */
    int32_t mcus_x, mcus_y;         /* its MCU grid */
    int32_t first_mcu, first_block, first_row;   /* where it starts in the call's index spaces */
    int32_t reserved;               /* 0 */
    uint64_t raw_offset;            /* of its first MCU row in the row buffer, bytes (a multiple of 16) */
    uint64_t bound;                 /* fm_jpeg_encode_bound(width, height) */
} fm_crop_plan;
typedef struct fm_crop_totals {     /* 32 bytes */
    int32_t mcus, blocks, rows;
    int32_t reserved;               /* 0 */
    uint64_t raw_bytes;             /* of the row buffer */
    uint64_t bound;                 /* sum of the files' bounds */
} fm_crop_totals;
size_t fm_jpeg_encode_regions_bound(const fm_crop_rect* rects, int n, int shrink);
int fm_jpeg_encode_regions_plan(const fm_crop_rect* rects, int n, int shrink, fm_crop_plan* plans, fm_crop_totals* totals);
int fm_jpeg_encode_regions_assemble(const fm_crop_plan* plans, int n, int quality, const uint32_t* seg_len, const uint8_t* segs,
                                    size_t segs_bytes, uint8_t* out, size_t capacity, size_t* offsets);
int fm_frame_encode_regions(fm_ctx* ctx, int which, const fm_crop_rect* rects, int n, int shrink, int quality, uint8_t* out,
                            size_t capacity, size_t* offsets);

/* ---------------------------------------------------------------- detector ------------ */
#define FM_MAX_HEADS 4
#define FM_MAX_ANCHORS 6   /* yolo_layer.h:11 */
typedef struct fm_det48 {  /* DET_DTYPE, detector.py:18-23 (aligned, 48 B) */
    double tlbr[4];
    int64_t label;
    double conf;
} fm_det48;

typedef struct fm_yolo_cfg {
    int32_t in_w, in_h;                 /* network input (INPUT_SHAPE) */
    int32_t roi_x, roi_y, roi_w, roi_h; /* letterbox ROI inside the input (whole input if !LETTERBOX) */
    int32_t input_tensor;               /* tensor id of the network input */
    int32_t n_heads;
    int32_t head_tensor[FM_MAX_HEADS];  /* fp32 NHWC head tensors, channel = anchor*(5+C) + attr */
    int32_t grid_w[FM_MAX_HEADS], grid_h[FM_MAX_HEADS], n_anchors[FM_MAX_HEADS];
    float anchors[FM_MAX_HEADS][2 * FM_MAX_ANCHORS];
    float scale_xy[FM_MAX_HEADS];
    int32_t num_classes, new_coords;
    uint8_t label_mask[128];            /* class ids to keep (detector.py:262-266) */
    double conf_thresh, nms_thresh, max_area, min_aspect_ratio;
    double size[2], offset[2];          /* upscaled_sz / bbox_offset (detector.py:302-320) */
    int32_t max_candidates;             /* capacity of the candidate list (default 8192) */
} fm_yolo_cfg;

int fm_detect_configure(fm_ctx* ctx, const fm_yolo_cfg* cfg);
/* Anchor-free heads with a DFL box branch (Ultralytics YOLOv8 `Detect`, read from its ONNX export by
 * models/onnx_detector.py): level i ends in 4 * 16 box logits (sides left, top, right, bottom; 16 bins each) and
 * num_classes class logits per cell, in fp32 NHWC tensors.  Decode (csrc/dfl_decode.h): d_side = sum_k k softmax(b[side])_k,
 * anchor point (col + 0.5, row + 0.5), corners (anchor -+ d) * stride, class = first maximum, cls_prob = sigmoid(logit),
 * box_conf = 1, one row per cell, rows numbered level-major. */
typedef struct fm_dfl_heads {
    int32_t n_levels;                   /* == cfg->n_heads */
    int32_t box_tensor[FM_MAX_HEADS], box_coff[FM_MAX_HEADS];   /* tensor id / first channel of the 64 box logits (coff % 4 == 0) */
    int32_t cls_tensor[FM_MAX_HEADS], cls_coff[FM_MAX_HEADS];   /* ... of the class logits (the same tensor or another) */
    float stride[FM_MAX_HEADS];         /* input pixels per cell */
} fm_dfl_heads;
/* fm_detect_configure for such heads: cfg as there (input, ROI, n_heads, grid_w / grid_h, num_classes <= 128, label mask,
 * thresholds, size / offset, max_candidates); its head_tensor, n_anchors, anchors, scale_xy and new_coords are ignored.
 * Everything behind the decode -- fm_detect_async*, fm_detect_sync, fm_detect_raw_candidates, fm_detect_configure_tiles --
 * works as behind fm_detect_configure; a later fm_detect_configure returns to the anchor-based decode. */
int fm_detect_configure_dfl(fm_ctx* ctx, const fm_yolo_cfg* cfg, const fm_dfl_heads* heads);
/* YOLODetector.detect_async (detector.py:270-273): preprocess (bilinear resize in u8, BGR->RGB,
 * /255, detector.py:289-300) -> network -> head decode (plugins/yolo_layer.cu:127-230) ->
 * score/class filter -> per-class DIoU-NMS -> box filter (detector.py:322-365); network and decode on the detector
 * stream, sort / NMS / filter behind them on a stream of their own; only the surviving detections reach the host
 * (written to page-locked memory by the last kernel). */
int fm_detect_async(fm_ctx* ctx);
/* YOLODetector.postprocess (detector.py:275-287): waits for the stream, returns detections sorted
 * by class id.  Returns FM_ERR_STATE if the candidate list overflowed. */
int fm_detect_sync(fm_ctx* ctx, fm_det48* out, int cap, int* n);
/* candidates over conf_thresh / detections after NMS + box filters of the pass fm_detect_sync collected last */
int fm_detect_last_counts(fm_ctx* ctx, int* n_candidates, int* n_detections);
/* test hooks: run only the preprocessing / only the filter+NMS stage on host-provided YOLO
 * candidate rows [n][7] = x, y, w, h, box_conf, class_id, class_prob (yolo_layer.h:34-39) */
int fm_detect_preprocess_only(fm_ctx* ctx);
int fm_filter_dets(fm_ctx* ctx, const float* rows, int n, fm_det48* out, int cap, int* n_out);
int fm_detect_raw_candidates(fm_ctx* ctx, float* rows, int cap, int* n);
/* measurement hook: the decode kernel of the configured detector alone, `iters` launches over the head tensors of the last
 * pass, each between two HIP events -> the mean time in us.  No pass may be in flight. */
int fm_detect_decode_us(fm_ctx* ctx, int iters, float* us);
/* HIP-event duration (ms) of the network launches of the pass fm_detect_sync collected last, recorded on the detector
 * stream (the bench's live roofline measurement); -1 when that pass carried no events (option "net_timing").  A batch
 * pass (fm_detect_async_ahead) reports its duration on the collect of its first frame and -1 on the others.  A pass in
 * two parts (front-ahead) reports the sum of its front's and its back's brackets, not the span between them. */
int fm_detect_net_ms(fm_ctx* ctx, float* ms);
/* Tiled detection (SSDDetector's tiling, fastmot/detector.py:77-139, for the YOLO networks): the frame is resized to a
 * tiling region and cut into n_tiles overlapping tiles of the network's input size, which ONE network pass takes as the
 * samples of a batch.  Call after fm_detect_configure (which returns the detector to untiled); n_tiles = 0 does the same,
 * otherwise 2 <= n_tiles <= FM_MAX_DET_BATCH <= the detector network's max_batch.
 *   origins  [n_tiles][2]  top-left corner of each tile in the region; every tile lies inside it.  Input pixel (x, y) of
 *                          tile t is pixel (x + origin_x, y + origin_y) of the frame resized to region_w x region_h with
 *                          the detector's own arithmetic (detector.py:289-300); the letterbox ROI is not applied.
 *   offsets  [n_tiles][2]  the decode's box offset per tile (subtracted, detector.py:343): -origin * frame size / region
 *                          size; its box scale, one for all tiles, is fm_yolo_cfg.size = tile size * frame size / region size
 * From then on fm_detect_async and fm_detect_async_next run one batch-n_tiles pass over the tiles of the current / next
 * frame -- decode, sort, DIoU-NMS and box filters per tile, in frame coordinates, exactly as for a sample of
 * fm_detect_async_ahead -- and fm_detect_sync returns that frame's detections after the cross-tile merge
 * (fm_detect_merge_tiles with merge_thresh).  A candidate-list overflow in any tile is reported by that frame's
 * fm_detect_sync; fm_detect_last_counts returns the sums over the tiles; fm_detect_net_ms the one pass.
 * fm_detect_async_ahead on a tiled detector is FM_ERR_STATE. */
int fm_detect_configure_tiles(fm_ctx* ctx, int n_tiles, const int32_t* origins, int region_w, int region_h,
                              const double* offsets, double merge_thresh);
/* The per-tile detections of the frame fm_detect_sync collected last, before the merge: tile-major, counts[t] rows of
 * tile t (counts: FM_MAX_DET_BATCH entries).  FM_ERR_ARG when the detector is not tiled or cap is too small. */
int fm_detect_last_tiles(fm_ctx* ctx, fm_det48* out, int cap, int32_t* counts, int* n_tiles);
/* SSDDetector._merge_dets (detector.py:132-139,187-217) on the host, no device call: detections of different tiles
 * (tile_ids[i] in [0, n_tiles)) and the same class whose intersection-over-minimum is >= thresh are linked (running
 * maxima per neighbouring tile, in index order); a connected group collapses into its first member with the enclosing
 * box and the maximum confidence.  Survivors in the iteration order of the reference's (Numba) set, then ordered by class
 * with a stable sort.  out: room for n rows; it may not overlap dets. */
int fm_detect_merge_tiles(const fm_det48* dets, const int32_t* tile_ids, int n, int n_tiles, double thresh,
                          fm_det48* out, int* n_out);

/* ---------------------------------------------------------------- feature extractor --- */
/* FeatureExtractor.extract_async (feature_extractor.py:48-60): for n boxes crop the current
 * device frame (multi_crop, utils/rect.py:93-97: int truncation, clamp >= 0, inclusive br),
 * resize to INPUT_SHAPE with OpenCV's fixed-point INTER_LINEAR (cv2.resize, feature_extractor.py:85),
 * BGR->RGB, /255, ImageNet mean/std (feature_extractor.py:88-98) -> network input, then run the
 * ReID network in batches of max_batch; FM_OP_HEAD leaves the L2-normalised embeddings
 * (feature_extractor.py:73) in the ctx embedding table, where association reads them. */
int fm_extract_configure(fm_ctx* ctx, int input_tensor, int in_w, int in_h);
int fm_extract_async(fm_ctx* ctx, int n, const double* tlbr);
/* FeatureExtractor.postprocess (feature_extractor.py:62-74): sync + copy [n][dim] f32 to host */
int fm_extract_sync(fm_ctx* ctx, int n, float* emb);
/* test hook: the preprocessed crops [n][in_h][in_w][3] as f32 (RGB, normalised) */
int fm_extract_read_input(fm_ctx* ctx, int n, float* out);

/* ---------------------------------------------------------------- optical flow (KLT) --- */
/* Flow.__init__ buffers / parameters (flow.py:17-119).  Image sizes: full frame, optical-flow
 * frame (opt_flow_scale_factor) and background-feature frame (bg_feat_scale_factor). */
typedef struct fm_flow_cfg {
    int32_t small_w, small_h;     /* round(opt_flow_scale_factor * size) */
    int32_t bg_w, bg_h;           /* round(bg_feat_scale_factor * size)  */
    int32_t win_size, max_level, max_count;   /* cv2.calcOpticalFlowPyrLK winSize / maxLevel / criteria */
    double epsilon;
    int32_t fast_thresh;          /* bg_feat_thresh */
    int32_t max_corners, block_size;   /* maxCorners 1 .. 1024 (OpenCV's "<= 0 = no limit" is refused with FM_ERR_ARG, as is
                                        * anything above: the selection keeps a crop's accepted corners in LDS); blockSize 3 or 5.
                                        * A crop with more than 4096 candidates keeps its 4096 strongest: DESIGN.md 7 */
    double quality_level;         /* obj_feat_params */
    int32_t gray_coeff_bits;      /* cv2.cvtColor(BGR2GRAY) fixed point: 14 = B 1868, G 9617, R 4899 (OpenCV <= 4.2-era
                                   * RGB2Gray<uchar>, what the reference's pinned 4.1.1 computes as far as it can be
                                   * established offline), 15 = 3735 / 19235 / 9798 (later 4.x); 0 = 14.  DESIGN.md 7 */
} fm_flow_cfg;
int fm_flow_configure(fm_ctx* ctx, const fm_flow_cfg* cfg);
/* Flow.init (flow.py:121-133): BGR->gray + optical-flow resize (+pyramid) of the current device frame
 * become the "previous" images */
int fm_flow_init(fm_ctx* ctx);
/* first part of Flow.predict (flow.py:153-154): gray / small / pyramid of the current device
 * frame, enqueued on the flow stream (overlaps the detector) */
int fm_flow_begin(fm_ctx* ctx);
/* mask bookkeeping of flow.py:159-181 for nT tracks in closest-first order:
 * area_out[k]  = mask_area(crop(fg_mask, rect_k)) with every earlier rect already zeroed,
 * keep_out[i]  = _rect_filter verdict of propagated keypoint i (kp_off[k]..kp_off[k+1]) */
int fm_flow_targets(fm_ctx* ctx, int nT, const double* inside_tlbr, const float* kps, const int32_t* kp_off,
                    int32_t* area_out, uint8_t* keep_out);
/* cv2.goodFeaturesToTrack on the previous gray crop of each listed track (flow.py:169-178) with
 * the foreground mask of fm_flow_targets, followed by _ellipse_filter (flow.py:297-306).
 * track_idx: indices into the fm_flow_targets arrays; track_tlbr: full (unclipped) boxes;
 * min_dist: minDistance per track.  pts_out: [n][cap][2] f32 frame coordinates, counts_out[n]. */
int fm_flow_detect(fm_ctx* ctx, int n, const int32_t* track_idx, const double* track_tlbr,
                   const int32_t* min_dist, int cap, float* pts_out, int32_t* counts_out);
/* background keypoints (flow.py:187-200): INTER_LINEAR resize of the previous gray frame,
 * INTER_NEAREST resize of the final foreground mask, FAST-9/16 + NMS, mask filter.
 * pts_out: [cap][2] f32 in background-frame coordinates (not yet unscaled). */
int fm_flow_background(fm_ctx* ctx, int cap, float* pts_out, int* n_out);
/* fm_flow_targets + fm_flow_detect (for the tracks that turn out to need new keypoints,
 * flow.py:167-178: len(kept) < feat_density * area, minDistance = max(round(sqrt(area) *
 * feat_dist_factor), 1)) + fm_flow_background in ONE stream round trip.  New keypoints are returned
 * compacted: track k owns new_pts[new_off[k] .. new_off[k] + new_cnt[k]). */
int fm_flow_prepare(fm_ctx* ctx, int nT, const double* inside_tlbr, const double* full_tlbr,
                    const float* kps, const int32_t* kp_off, double feat_density, double feat_dist_factor,
                    int32_t* area_out, uint8_t* keep_out, uint8_t* needy_out, int pts_cap,
                    float* new_pts_out, int32_t* new_off_out, int32_t* new_cnt_out, int* n_new_out,
                    int bg_cap, float* bg_pts_out, int* n_bg_out);
/* cv2.calcOpticalFlowPyrLK(prev_small, cur_small, pts) (flow.py:205-207): Scharr derivatives +
 * pyramidal LK for n points; then the frame buffers are swapped (flow.py:212-213). */
int fm_flow_lk(fm_ctx* ctx, int n, const float* prev_pts, float* next_pts, uint8_t* status, float* err);
/* swap without LK (failure paths of flow.py:191-196) */
int fm_flow_swap(fm_ctx* ctx);
/* second half of Flow.predict on the host side of the library (flow.py:215-263): camera motion by
 * cv2.findHomography(RANSAC) over the background matches, then per track _fg_filter ->
 * cv2.estimateAffinePartial2D(RANSAC) -> _estimate_bbox -> inlier bookkeeping.  Latency-bound
 * serial work (a few microseconds per hypothesis loop): kept in C++ on the host, see DESIGN.md.
 * Inputs: prev/cur points (frame coordinates), status, target ranges [begin,end) per track
 * (closest-first), bg range, boxes.  Outputs: H (3x3), ok flag, per track result code
 * (0 = skipped, 1 = box estimated), est_tlbr, n_matched, inlier flags over all points. */
int fm_flow_estimate(fm_ctx* ctx, int n_pts, const float* prev_pts, const float* cur_pts,
                     const uint8_t* status, int nT, const int32_t* begins, const int32_t* ends,
                     int bg_begin, int bg_end, const double* track_tlbr, int frame_w, int frame_h,
                     int ransac_max_iter, double ransac_conf, int inlier_thresh,
                     double* H_out, int* ok_out, int32_t* result_out, double* est_tlbr_out,
                     int32_t* n_matched_out, uint8_t* inlier_out);
/* Flow.predict (flow.py:135-264) as ONE call = fm_flow_begin + fm_flow_prepare + the keypoint list
 * assembly + fm_flow_lk + fm_flow_estimate, with the NumPy glue arithmetic of the reference (float32
 * scale products) done in the library.  Inputs as fm_flow_prepare (tracks closest-first).
 * Outputs: status (FM_FLOW_OK / NO_BACKGROUND: no background keypoints, buffers swapped, flow.py:191-196 /
 * NO_HOMOGRAPHY: flow.py:227-231); H (3x3); per track result code (0 skipped, 1 box estimated, 2 estimated
 * but rejected), est_tlbr, n_matched; the RANSAC-inlier keypoints compacted in prev_out / cur_out
 * ([pts_cap][2] f32, frame coordinates): track k owns [trk_off[k], trk_off[k+1]) (empty when result 0),
 * the background inliers [bg_range[0], bg_range[1]). */
typedef struct fm_flow_predict_params {
    double feat_density, feat_dist_factor;
    float opt_scale[2], bg_scale[2];      /* opt_flow_scale_factor, bg_feat_scale_factor as float32 */
    double max_error;                     /* compared as float32, like NumPy's err < max_error */
    int32_t ransac_max_iter;
    double ransac_conf;
    int32_t inlier_thresh;
    int32_t frame_w, frame_h;
} fm_flow_predict_params;
enum { FM_FLOW_OK = 0, FM_FLOW_NO_BACKGROUND = 1, FM_FLOW_NO_HOMOGRAPHY = 2 };
int fm_flow_predict(fm_ctx* ctx, int nT, const double* inside_tlbr, const double* full_tlbr, const float* kps,
                    const int32_t* kp_off, const fm_flow_predict_params* prm, int pts_cap, float* prev_out,
                    float* cur_out, int32_t* trk_off_out, int32_t* bg_range_out, double* H_out, int* status_out,
                    int32_t* result_out, double* est_tlbr_out, int32_t* n_matched_out);
/* The KLT + Kalman chain of one step on the library's own worker thread: fm_flow_predict followed by fm_trk_step with
 * the KLT measurements MultiTracker.apply_kalman derives from it (tracker.py:150-183).  nT tracks in prediction order
 * (as fm_flow_predict), nK tracks in table order for the Kalman step: slots, ages and sorted_idx[i] = position of
 * track i among the nT predicted ones or -1; multiplier = max(age_penalty * age, 1) / inlier_ratio.  All pointers
 * must stay valid until fm_track_predict_wait returns; one job at a time PER CONTEXT (every fm_ctx owns its worker).
 * fm_track_predict_wait reports the prediction status (FM_FLOW_*) and whether the Kalman step ran. */
int fm_track_predict_async(fm_ctx* ctx, int nT, const double* inside_tlbr, const double* full_tlbr, const float* kps,
                           const int32_t* kp_off, const fm_flow_predict_params* prm, int pts_cap, float* prev_out,
                           float* cur_out, int32_t* trk_off_out, int32_t* bg_range_out, double* H_out,
                           int32_t* result_out, double* est_tlbr_out, int32_t* n_matched_out, int nK,
                           const int32_t* slots, const int32_t* ages, const int32_t* sorted_idx, double age_penalty,
                           double* tlbr_out, uint8_t* lost_out);
int fm_track_predict_wait(fm_ctx* ctx, int* status_out, int* kalman_done_out);
/* ---------------------------------------------------------------- SSD detector --------- */
/* The stages of the reference's SSDDetector around its TensorRT engine (fastmot/detector.py:94-120,161-185) and the
 * engine's NMS_TRT plugin (reference models/ssd.py:136-150), on the detector stream.  The network (models/ssd.py here:
 * SSDMobileNetV1.build_graph) is FM_NET_DETECTOR at max_batch >= n_tiles; its input is a tensor, so FM_MAX_DET_BATCH does
 * not bind: a pass takes up to FM_MAX_SSD_TILES tiles (the default 4 x 2 grid needs 8).
 *   preprocess   input pixel (x, y) of tile t = pixel (x + tile_x[t], y + tile_y[t]) of the current frame resized to
 *                region_w x region_h with cv2.resize's arithmetic (INTER_LINEAR; an exact 2x decimation: INTER_AREA),
 *                BGR -> RGB, float32(u8 * (2 / 255.) - 1.), fp16
 *   decode       per tile and anchor (cya, cxa, ha, wa): (ty, tx, th, tw) = loc / box_scales, cy = ty ha + cya,
 *                cx = tx wa + cxa, h = exp(th) ha, w = exp(tw) wa, corners clipped to [0, 1]; score = sigmoid(logit)
 *   NMS          per (tile, class != 0): the topk highest scores above 1e-8, greedy NMS among them (IoU without +1; a box is
 *                dropped when its IoU with a kept, higher-scored box is > nms_thresh)
 *   top-K        per tile: the topk highest-scored survivors over all classes, descending, as rows (tile, label, conf,
 *                xmin, ymin, xmax, ymax); unused rows (tile, -1, 0, 0, 0, 0, 0).  Ties in score: (class, anchor) ascending.
 * Head tensor k: fp32 [n_tiles][map_h][map_w][>= n_anchors * (4 + num_classes)], channels [n_anchors * 4 box | n_anchors *
 * num_classes class], anchor-major; the anchor table lists (cy, cx, h, w) in (head, row, column, anchor) order. */
#define FM_MAX_SSD_TILES 16
#define FM_MAX_SSD_HEADS 6
typedef struct fm_ssd_cfg {
    int32_t input_tensor, in_w, in_h;
    int32_t n_heads;
    int32_t head_tensor[FM_MAX_SSD_HEADS], map_w[FM_MAX_SSD_HEADS], map_h[FM_MAX_SSD_HEADS], n_anchors[FM_MAX_SSD_HEADS];
    const float* anchors;        /* host, [n_anchor_rows][4]; copied by fm_ssd_configure */
    int32_t n_anchor_rows;       /* = sum of map_w * map_h * n_anchors, at most 4096 */
    float box_scales[4];         /* (y, x, h, w) */
    int32_t num_classes;         /* including the background class 0; at most 256 */
    int32_t topk;                /* at most 256 */
    float nms_thresh;
    int32_t n_tiles;
    int32_t tile_x[FM_MAX_SSD_TILES], tile_y[FM_MAX_SSD_TILES];
    int32_t region_w, region_h;
} fm_ssd_cfg;
/* (a configuration beyond these limits is refused with FM_ERR_ARG before anything is launched, and the context is then
 * left without an SSD state -- as after a failed allocation -- until a call succeeds) */
int fm_ssd_configure(fm_ctx* ctx, const fm_ssd_cfg* cfg);
/* preprocess -> fm_net_run at batch n_tiles -> decode / NMS / top-K; nothing synchronises */
int fm_ssd_detect_async(fm_ctx* ctx);
/* waits for the pass and copies its n_tiles * topk rows of 7 floats (cap: rows) */
int fm_ssd_detect_sync(fm_ctx* ctx, float* rows, int cap, int* n);
/* test hooks: the preprocess kernel alone (result in the input tensor); decode + NMS + top-K on caller-provided head tensors,
 * heads[k] = dense [n_tiles][map_h * map_w][n_anchors * (4 + num_classes)] f32 (needs no network) */
int fm_ssd_preprocess_only(fm_ctx* ctx);
/* HIP-event times (ms) of the three stages -- preprocess, network, decode / NMS / top-K -- of the last collected pass that ran with
 * option "net_timing" > 0; -1 each otherwise (measurement: scripts/ssd_timing.py) */
int fm_ssd_stage_ms(fm_ctx* ctx, float ms[3]);
int fm_ssd_postprocess_host_heads(fm_ctx* ctx, const float* const* heads, float* rows, int cap, int* n);

/* LDS bytes FM_OP_LITECHAIN needs for c channels on h x w maps (<= 65536 to be launchable): the layer-table
 * builder decides with the same formula whether an OSNet block can use the chain kernel (no device needed) */
size_t fm_litechain_lds_bytes(int c, int w, int h);
/* 1 when FM_OP_RESBLOCK supports c in/out channels with mid hidden channels (no device needed) */
int fm_resblock_supported(int c, int mid);
/* 1 when FM_OP_SEPCONV supports a separable block cin -> cout with a depthwise stride (no device needed) */
int fm_sepconv_supported(int cin, int cout, int stride);
/* 1 when FM_OP_CONVIN runs a pointwise conv K -> cout with instance normalisation over a map of hw pixels (no device needed) */
int fm_convin_supported(int K, int cout, int hw);
/* 1 when FM_OP_NONLOCAL runs a non-local block over c channels and a map of hw pixels (no device needed) */
int fm_nonlocal_supported(int c, int hw);
/* profiling hook: accumulated host wall time (ms) of the stages of fm_flow_predict -- out5 = {begin, prepare,
 * lk, estimate, number of calls}; reset != 0 clears the accumulators */
int fm_flow_timing(double* out5, int reset);
/* test hooks: read the device images (which: 0 prev gray, 1 cur gray, 2.. pyramid levels of prev
 * (2+l) and cur (10+l), 20 bg image) */
int fm_flow_read_image(fm_ctx* ctx, int which, uint8_t* out, int* w, int* h);

/* ------------------------------------------------------------------------------------------------------------------
 * Cross-stream ReID-gallery all-gather (multi-GPU: one process and one fm_ctx per GPU / video stream).  NOT in the
 * reference, which tracks one stream in one process; the exchanged rows extend the history side of _reid_cost
 * (tracker.py:355-366).  RCCL (librccl.so) is loaded on the first call.  fm_gallery_unique_id: rank 0 creates the
 * 128-byte communicator id and the application distributes it; fm_gallery_init (collective) joins it;
 * fm_gallery_allgather_async (collective) enqueues H2D + ncclAllGather + D2H of one fixed-size row per rank on a
 * side stream and returns; fm_gallery_allgather_wait copies out the world * row_bytes gathered rows, rank-major.
 * channel: a context owns two independent communicators, 0 = the gallery, 1 = small control messages of the
 * application (barrier / max-over-ranks of a benchmark); one exchange in flight per channel.
 * In-process constraint: RCCL resolves the HSA runtime by its bare library name; a process that has ALSO loaded
 * another ROCm copy (import torch) must run its collectives through that copy's RCCL (gallery.py: TorchComm). */
int fm_gallery_unique_id(char* out128);
int fm_gallery_init(fm_ctx* ctx, int channel, int world, int rank, const char* id128, size_t row_bytes);
int fm_gallery_allgather_async(fm_ctx* ctx, int channel, const void* send_row);
int fm_gallery_allgather_wait(fm_ctx* ctx, int channel, void* recv_rows, float* stream_ms_out);
int fm_gallery_destroy(fm_ctx* ctx, int channel);

#ifdef __cplusplus
}
#endif
#endif /* FASTMOT_HIP_H */
