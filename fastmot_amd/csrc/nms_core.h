// Candidate sort, per-class DIoU-NMS and the final box filter of the detector on the device (YOLODetector._filter_dets,
// fastmot/detector.py:322-365; diou_nms, fastmot/utils/rect.py:199-244): the shared pieces, then the kernels built from
// them.  Included ONCE by detect.hip, inside its anonymous namespace: the code is part of that translation unit.
//
// Two routes lead through the NMS and must give the same detections, identical to the reference:
//   greedy route    nms_greedy_kernel (the default: up to NG_KMAX candidates, up to NG_MAX_ROUNDS survivors)
//   general route   nms_mask_kernel + nms_scan_kernel (any number of candidates up to the capacity)
// What decides a detection is therefore written once, here: the pair test (diou_pretest in float32, diou_suppresses in
// the reference's float64 for the close calls), the box filter (box_filter), the ordered write of the detections
// (emit_in_order) and the record the host reads (report).
#pragma once

// ------------------------------------------------------------------------------------ small pieces
// a candidate row: x y w h box_conf class cls_prob orig_idx(as float bits), 32 bytes
__device__ __forceinline__ void load_row(const float* __restrict__ rows, int i, float r[8]) {
    const float4 q0 = *reinterpret_cast<const float4*>(rows + (size_t)i * 8);
    const float4 q1 = *reinterpret_cast<const float4*>(rows + (size_t)i * 8 + 4);
    r[0] = q0.x; r[1] = q0.y; r[2] = q0.z; r[3] = q0.w; r[4] = q1.x; r[5] = q1.y; r[6] = q1.z; r[7] = q1.w;
}
__device__ __forceinline__ void store_row(float* __restrict__ rows, int i, const float r[8]) {
    *reinterpret_cast<float4*>(rows + (size_t)i * 8) = make_float4(r[0], r[1], r[2], r[3]);
    *reinterpret_cast<float4*>(rows + (size_t)i * 8 + 4) = make_float4(r[4], r[5], r[6], r[7]);
}

// a 64-bit value of lane `l` / of the first active lane, in scalar registers (wave-uniform bookkeeping)
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
    return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l) |
           ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l) << 32);
}
__device__ __forceinline__ uint64_t readfirstlane64(uint64_t v) {
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) |
           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32);
}

// barrier that waits for this wave's LDS traffic only: __syncthreads() would also drain the global loads in flight
// (its fence waits for vmcnt(0)) and expose their latency in every iteration
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// where the last kernel of a route leaves the detections (by value: the tail of both kernels' argument lists)
struct PostOut {
    double max_area, min_ar;    // box filter (detector.py:358-361)
    fm_det48* dets;             // [cap] device list
    fm_det48* dets_host;        // page-locked copy of its first `prefix` rows, written by the kernel itself
    int prefix;
    int32_t* counters_host;     // page-locked: [0]=n_cand [1]=overflow [2]=n_det [3]=declined
};

// The record of a pass.  declined != 0: the greedy kernel did not take the pass -- more candidates than it was given LDS
// for (1), or more survivors than its round budget (2) -- and collect() runs the general route for it.
__device__ __forceinline__ void report(int32_t* counters, int32_t* counters_host, int n_dets, int declined) {
    counters[2] = n_dets;
    counters[3] = declined;
    counters_host[0] = counters[0]; counters_host[1] = counters[1]; counters_host[2] = n_dets; counters_host[3] = declined;
}

// ------------------------------------------------------------------------------------ sort
// rank sort by (class asc, box_conf desc, original index asc); K is read from the device counter.  Every workgroup
// ranks 256 candidates against all K: the sort keys of 256 candidates at a time are staged in LDS as ONE 64-bit integer
// each -- class (8 bits: emit_candidate admits classes < 128) | descending-order key of box_conf (32 bits) | original
// index (24 bits: fm_detect_configure / fm_filter_dets refuse more rows than that) -- and read by all lanes at the same
// address (broadcast): K^2 integer comparisons from LDS instead of K^2 dependent global reads (K = 1500: 1.24 ms ->
// ~10 us).  The confidence key is the usual order-preserving map of IEEE bits (negative values: all bits flipped,
// others: sign bit set), inverted for the descending order, so a negative or -0.0 confidence (a NEW_COORDS head without
// its logistic activation, rows from the test hook) ranks where the float comparison puts it.
constexpr int FM_SORT_INDEX_BITS = 24;
__device__ __forceinline__ uint64_t sort_key(const float* r) {
    const uint64_t cls = (uint64_t)(uint32_t)(int)r[5] & 0xffull;
    const uint32_t b = __float_as_uint(r[4] + 0.0f);                       // (-0.0 + 0.0 = +0.0: equal to +0.0, as it compares)
    const uint32_t asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    const uint64_t inv_score = (uint32_t)~asc;
    const uint64_t ord = (uint64_t)(uint32_t)__float_as_int(r[7]) & ((1ull << FM_SORT_INDEX_BITS) - 1);
    return (cls << 56) | (inv_score << FM_SORT_INDEX_BITS) | ord;
}

__global__ __launch_bounds__(256) void rank_sort_kernel(const float* __restrict__ cand, float* __restrict__ sorted,
                                                        const int32_t* __restrict__ counters, int cap) {
    const int K = min(counters[0], cap);
    if ((int)blockIdx.x * 256 >= K) return;
    __shared__ uint64_t keys[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < K;
    const float* ri = cand + (size_t)(live ? i : 0) * 8;
    const uint64_t ki = sort_key(ri);
    int rank = 0;
    for (int j0 = 0; j0 < K; j0 += 256) {
        const int j = j0 + threadIdx.x;
        keys[threadIdx.x] = j < K ? sort_key(cand + (size_t)j * 8) : ~0ull;      // (padding keys rank after everything)
        __syncthreads();
#pragma unroll 8
        for (int t = 0; t < 256; ++t) rank += keys[t] < ki ? 1 : 0;
        __syncthreads();
    }
    if (!live) return;
    float r[8];
    load_row(cand, i, r);
    store_row(sorted, rank, r);
}

// The same rank sort with ALL K keys staged in LDS at once (dynamic LDS: 8 bytes per candidate of capacity; used
// whenever that fits, i.e. up to 16384 candidates): the chunked version above pays one dependent global round trip and
// two barriers per 256 keys -- six in a row for the ~1500 candidates of the benchmark, on a GPU whose memory system is
// busy with the detector and ReID networks -- this one pays a single round trip with every load of the workgroup in
// flight, then compares out of LDS two keys per ds_read_b128 (broadcast: every lane reads the same address).
__global__ __launch_bounds__(256) void rank_sort_lds_kernel(const float* __restrict__ cand, float* __restrict__ sorted,
                                                            const int32_t* __restrict__ counters, int cap) {
    __builtin_amdgcn_s_setprio(3);         // (latency-critical side work beside the networks' bulk wavefronts)
    extern __shared__ uint64_t all_keys[];
    const int K = min(counters[0], cap);
    // a workgroup ranks 64 candidates, four lanes each: every lane counts the smaller keys in its quarter of the list
    // (four times the wavefronts of one-lane-per-candidate for the same K^2 comparisons: the chain of a lane -- LDS read,
    // two 64-bit compares, add -- is latency bound, more wavefronts hide it)
    if ((int)blockIdx.x * 64 >= K) return;
    const int Kp = (K + 7) & ~7;                                  // (padding keys rank last)
    const int i = blockIdx.x * 64 + (threadIdx.x >> 2), q = threadIdx.x & 3;
    // this lane's own row is fetched together with the keys (one memory round trip for both, the kernel is a chain of them)
    float r[8];
    load_row(cand, min(i, K - 1), r);
    for (int j = threadIdx.x; j < Kp; j += 256) all_keys[j] = j < K ? sort_key(cand + (size_t)j * 8) : ~0ull;
    __syncthreads();
    const uint64_t ki = all_keys[min(i, Kp - 1)];
    int rank = 0;
    const ulonglong2* k2 = reinterpret_cast<const ulonglong2*>(all_keys) + q * (Kp / 8);
#pragma unroll 8
    for (int t = 0; t < Kp / 8; ++t) {
        const ulonglong2 k = k2[t];
        rank += (k.x < ki ? 1 : 0) + (k.y < ki ? 1 : 0);
    }
    rank += __shfl_xor(rank, 1);
    rank += __shfl_xor(rank, 2);
    if (i >= K || q != 0) return;
    store_row(sorted, rank, r);
}

// ------------------------------------------------------------------------------------ the pair test
// suppression test of utils/rect.py:216-241 for pair (i keeps, j candidate), same class.
__device__ __forceinline__ bool diou_suppresses(const float* a, const float* b, double thresh) {
    const float area_a = a[2] * a[3], area_b = b[2] * b[3];          // float32 products
    const double abr_x = (double)(a[0] + a[2]) - 1, abr_y = (double)(a[1] + a[3]) - 1;
    const double bbr_x = (double)(b[0] + b[2]) - 1, bbr_y = (double)(b[1] + b[3]) - 1;
    const double acx = ((double)a[0] + abr_x) / 2, acy = ((double)a[1] + abr_y) / 2;
    const double bcx = ((double)b[0] + bbr_x) / 2, bcy = ((double)b[1] + bbr_y) / 2;
    const double ixmin = fmaxf(a[0], b[0]), iymin = fmaxf(a[1], b[1]);
    const double ixmax = fmin(abr_x, bbr_x), iymax = fmin(abr_y, bbr_y);
    const double iw = fmax(0., ixmax - ixmin + 1), ih = fmax(0., iymax - iymin + 1);
    const double inter = iw * ih;
    const double uni = (double)(area_a + area_b) - inter;
    const double iou = inter / uni;
    // (d / c)^0.6 >= 0, so DIoU <= IoU: a pair whose IoU does not exceed the threshold is never suppressed -- the
    // float64 pow (hundreds of instructions) is only evaluated for the few pairs that overlap that much.  A NaN IoU
    // (degenerate boxes) fails this test and takes the full path, like the reference's arithmetic.
    if (iou <= thresh) return false;
    const double exmin = fminf(a[0], b[0]), eymin = fminf(a[1], b[1]);
    const double exmax = fmax(abr_x, bbr_x), eymax = fmax(abr_y, bbr_y);
    const double ew = exmax - exmin + 1, eh = eymax - eymin + 1;
    const double c = ew * ew + eh * eh;
    const double d = (acx - bcx) * (acx - bcx) + (acy - bcy) * (acy - bcy);
    const double diou = iou - pow(d / c, 0.6);
    return !(diou <= thresh);
}

// (out of line for the greedy kernel: the float64 pow() inside costs ~100 registers, inlined it set the register count
// of the whole kernel although a handful of pairs per frame reach it)
__device__ __attribute__((noinline)) bool diou_suppresses_call(float a0, float a1, float a2, float a3, float b0, float b1,
                                                               float b2, float b3, double thresh) {
    const float a[4] = {a0, a1, a2, a3}, b[4] = {b0, b1, b2, b3};
    return diou_suppresses(a, b, thresh);
}

// the terms of the pair test that belong to the keeping box alone: computed once per keeper
struct Keeper { float x0, y0, x1, y1, area; };
__device__ __forceinline__ Keeper keeper_of(float x, float y, float w, float h) { return {x, y, x + w, y + h, w * h}; }

// The pair test in float32, two stages; only what neither decides pays for diou_suppresses.
//   1. An estimate of the IoU (the +1 pixel convention of rect.py included): DIoU <= IoU, so a pair whose estimate stays
//      clearly below the threshold (slack 1e-3, far above the float32 error of the estimate) cannot be suppressed.
//   2. The whole DIoU = IoU - (d / c)^0.6 with the hardware log2 / exp2 (centre distance d and enclosing diagonal c as in
//      rect.py:231-240; the -1 / +1 of the pixel convention cancel in both).  Its error is a few 1e-6 absolute; a pair is
//      decided here when the estimate is 1e-4 or more away from the threshold, and only the rest -- a handful per frame --
//      pays for the reference's float64 arithmetic and its pow().  In the dense regime of the benchmark (1500 candidates)
//      nearly every pair that passes the IoU pre-test used to take that path: ~10^6 float64 pow() per frame.
// A NaN anywhere (degenerate boxes) fails every comparison below and ends at PAIR_CLOSE: the exact test decides.
enum PairVerdict { PAIR_KEPT, PAIR_SUPPRESSED, PAIR_CLOSE };
__device__ __forceinline__ PairVerdict diou_pretest(const Keeper& a, float bx, float by, float bw, float bh, float thresh) {
    const float b_x1 = bx + bw, b_y1 = by + bh;
    const float iw = fminf(a.x1, b_x1) - fmaxf(a.x0, bx);
    const float ih = fminf(a.y1, b_y1) - fmaxf(a.y0, by);
    if (iw <= 0.f || ih <= 0.f) return PAIR_KEPT;
    const float inter = iw * ih;
    const float uni = a.area + bw * bh - inter;
    if (inter <= (thresh - 1e-3f) * uni) return PAIR_KEPT;
    const float ew = fmaxf(a.x1, b_x1) - fminf(a.x0, bx), eh = fmaxf(a.y1, b_y1) - fminf(a.y0, by);
    const float dx = 0.5f * ((a.x0 + a.x1) - (bx + b_x1)), dy = 0.5f * ((a.y0 + a.y1) - (by + b_y1));
    const float q = (dx * dx + dy * dy) / (ew * ew + eh * eh);
    const float est = inter / uni - (q > 0.f ? __builtin_amdgcn_exp2f(0.6f * __builtin_amdgcn_logf(q)) : 0.f);
    if (est > thresh + 1e-4f) return PAIR_SUPPRESSED;
    if (est < thresh - 1e-4f) return PAIR_KEPT;
    return PAIR_CLOSE;
}

// ------------------------------------------------------------------------------------ the final filter
// to_tlbr (utils/rect.py:49-57) on float64 copies of the float32 box, then the area and aspect-ratio tests of
// detector.py:356-361
__device__ __forceinline__ bool box_filter(float x, float y, float w, float h, double max_area, double min_ar, double t[4]) {
    const double xmin = x, ymin = y;
    t[0] = rint(xmin); t[1] = rint(ymin);
    t[2] = rint(xmin + (double)w - 1.); t[3] = rint(ymin + (double)h - 1.);
    const double bw = t[2] - t[0] + 1, bh = t[3] - t[1] + 1;
    const double area = (bw <= 0 || bh <= 0) ? 0. : bw * bh;
    const double ar = bw > 0 ? bh / bw : 0.;
    return area > 0 && area <= max_area && ar >= min_ar;
}

// One slice of the sorted list, one row per thread of a workgroup of NW wavefronts: the rows that are `ok` become
// detections behind the *base written so far, in thread order (ballot, per-wave counts), and *base moves on.  `row` is
// read for those rows only.  Called by all threads; base / wave_cnt are LDS (*base set to 0 before the first slice).
template <int NW>
__device__ __forceinline__ void emit_in_order(bool ok, const double t[4], const float* row, int* base, int* wave_cnt,
                                              const PostOut& o) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t bal = __ballot(ok);
    if (lane == 0) wave_cnt[wave] = __builtin_popcountll(bal);
    __syncthreads();
    const int before = *base;
    int off = before + __builtin_popcountll(bal & ((1ull << lane) - 1ull));
    for (int wv = 0; wv < wave; ++wv) off += wave_cnt[wv];
    if (ok) {
        fm_det48 d;
        d.tlbr[0] = t[0]; d.tlbr[1] = t[1]; d.tlbr[2] = t[2]; d.tlbr[3] = t[3];
        d.label = (int64_t)row[5];
        d.conf = (double)(row[4] * row[6]);     // float32 product (detector.py:362)
        o.dets[off] = d;
        if (off < o.prefix) o.dets_host[off] = d;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = before;
        for (int wv = 0; wv < NW; ++wv) n += wave_cnt[wv];
        *base = n;
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------ general route: bit matrix + scan
// mask[w][i] bit b = candidate j = 64*w + b (j > i, same class) is suppressed by i.  A task is one 64 x 64 block of the
// upper triangle (rows rb*64.., column word w >= rb); a workgroup takes tasks blockIdx.x, + gridDim.x, ...  (the grid
// is fixed, K is only known on the device).  Inside a task lane = row, and each of the four wavefronts tests 16 of the 64
// columns (staged in LDS once per task) and writes its quarter of the mask word: the per-lane loop over the columns is a
// dependent chain of ~60 instructions per column with divergent exits -- a quarter of it per wavefront and four times
// the wavefronts (1300 for the benchmark's 1555 candidates, the chip has 1024 SIMDs) took the kernel from 24 to 15 us
// inside the pipeline.
constexpr int NMS_MASK_GRID = 1024;
__global__ __launch_bounds__(256) void nms_mask_kernel(const float* __restrict__ sorted,
                                                       const int32_t* __restrict__ counters, int cap,
                                                       double thresh, uint64_t* __restrict__ mask) {
    __builtin_amdgcn_s_setprio(3);
    const int K = min(counters[0], cap);
    const int kw = (K + 63) / 64;
    const int ntask = kw * (kw + 1) / 2;
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    __shared__ float cols[64][8];
    for (int t = blockIdx.x; t < ntask; t += gridDim.x) {
        // t = w (w + 1) / 2 + rb, 0 <= rb <= w
        int w = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
        while (w * (w + 1) / 2 > t) --w;
        while ((w + 1) * (w + 2) / 2 <= t) ++w;
        const int rb = t - w * (w + 1) / 2;
        const int i = rb * 64 + lane;
        float a[8];
        load_row(sorted, min(i, K - 1), a);
        if (threadIdx.x < 128) {                        // 64 columns x two float4
            const int j = min(w * 64 + (threadIdx.x >> 1), K - 1);
            *reinterpret_cast<float4*>(&cols[threadIdx.x >> 1][(threadIdx.x & 1) * 4]) =
                *reinterpret_cast<const float4*>(sorted + (size_t)j * 8 + (threadIdx.x & 1) * 4);
        }
        __syncthreads();
        uint32_t bits = 0;
        const int b0 = q * 16, nb = min(16, K - w * 64 - b0);
        const Keeper ka = keeper_of(a[0], a[1], a[2], a[3]);
        for (int bb = 0; bb < nb; ++bb) {
            const int b = b0 + bb;
            if (w * 64 + b <= i) continue;
            const float* cb = cols[b];
            if (cb[5] != a[5]) continue;
            const PairVerdict v = diou_pretest(ka, cb[0], cb[1], cb[2], cb[3], (float)thresh);
            if (v == PAIR_SUPPRESSED || (v == PAIR_CLOSE && diou_suppresses(a, cb, thresh))) bits |= (1u << bb);
        }
        // word-major (the scan reads a word of many rows at once); this wavefront's 16 bits of the word
        if (i < K) reinterpret_cast<uint16_t*>(mask)[((size_t)w * cap + i) * 4 + q] = (uint16_t)bits;
        __syncthreads();                                // (cols is reused by the next task)
    }
}

// greedy scan in sorted order + final box filter (detector.py:356-364), one workgroup.  Two chunks of 64 candidates
// (c0 = 2j, c1 = 2j + 1) per iteration j.  The bits "removed by an earlier survivor" of a chunk are the OR of its mask
// word over all SURVIVING rows before the chunk -- a gather over the word-major mask.
//   wavefronts 1..15  do all the memory work, in three groups of five (320 lanes) that own the iterations j = g (mod 3).
//                     The loads of iteration j are issued (unconditionally, row indices clamped) three iterations ahead,
//                     right after the group has published its previous one, and nothing else of that wavefront touches
//                     memory in between: the compiler's own wait (everything outstanding) costs nothing and the round
//                     trip has three iterations' time.  (One group with alternating register sets did not get there:
//                     hipcc's wait counts across the loop's back edge fall to "everything outstanding".)
//                     The group publishes iteration j WHILE wavefront 0 resolves iteration j - 1, so it only knows the
//                     survivors before chunk p0 = 2j - 2:
//                       rem[0], rem[1]   OR of mask word c0 / c1 over the surviving rows before chunk p0,
//                       seven 64 x 64 blocks: (rows p0 | p1) x (word c0 | c1), and (c0, c0), (c0, c1), (c1, c1).
//   wavefront 0       touches LDS only: it folds the rows of the previous iteration's survivors (its own registers) and
//                     of c0's survivors into rem, and resolves each chunk in scalar registers (lane b holds row b's
//                     word of the diagonal block, one step per survivor that removes anything).
// One barrier per 128 candidates, no memory round trip and no gather on the critical path.
// History: 5.1 ms -> 68 us in round 3 (inside the pipeline; every chunk still waited for the loads it had just issued, in
// both roles: profiles/r03_bench_kernel_stats.txt) -> round 4: 107 us at the benchmark's ~1000 survivors of 1555 -> 41 us
// with gather and resolve in turns (two barriers per 128) -> this structure.
// The survivors are then filtered and written in order (prefix counts over the keep bits).
__global__ __launch_bounds__(1024) void nms_scan_kernel(const float* __restrict__ sorted,
                                                       int32_t* __restrict__ counters, int cap,
                                                       const uint64_t* __restrict__ mask, const PostOut out) {
    __builtin_amdgcn_s_setprio(3);
    extern __shared__ uint64_t keep[];       // [cap/64] survivors
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = min(counters[0], cap);
    const int kw = (K + 63) / 64;
    constexpr int GU = 8, GROWS = 320 * GU;  // rows whose loads are pipelined: 2560; beyond that (rare) they are fetched at use
    const int grp = wave > 0 ? (wave - 1) % 3 : 0, gl = wave > 0 ? ((wave - 1) / 3) * 64 + lane : 0;
    const int niter = (kw + 1) / 2;
    // the rows the final filter will want (candidates tid and tid + 1024) are fetched now: one memory round trip less
    // behind the scan
    float pre[2][8];
#pragma unroll
    for (int u = 0; u < 2; ++u) load_row(sorted, min(u * 1024 + tid, max(K - 1, 0)), pre[u]);
    struct Set { uint64_t g0[GU], g1[GU]; uint64_t blk[7]; };
    auto issue = [&](int j, Set& t) {
        const int c0 = 2 * j, c1 = min(2 * j + 1, kw - 1);
        const uint64_t* col0 = mask + (size_t)c0 * cap;
        const uint64_t* col1 = mask + (size_t)c1 * cap;
        const int last = max((c0 - 2) * 64 - 1, 0);
#pragma unroll
        for (int u = 0; u < GU; ++u)
            if (u == 0 || u * 320 <= last) {                                   // (uniform: only the rows that exist)
                const int i = min(u * 320 + gl, last);
                t.g0[u] = col0[i];
                t.g1[u] = col1[i];
            }
        if (wave <= 3) {                                   // the group's first wavefront publishes the blocks
            // (rows beyond K, or before the list for j = 0, are never looked at: their survivor bits are 0)
            const int rp0 = min(max((c0 - 2) * 64 + lane, 0), K - 1), rp1 = min(max((c0 - 1) * 64 + lane, 0), K - 1);
            const int r0 = min(c0 * 64 + lane, K - 1), r1 = min(c1 * 64 + lane, K - 1);
            t.blk[0] = col0[rp0]; t.blk[1] = col1[rp0];
            t.blk[2] = col0[rp1]; t.blk[3] = col1[rp1];
            t.blk[4] = col0[r0]; t.blk[5] = col1[r0]; t.blk[6] = col1[r1];
        }
    };
    auto alive = [&](int i, int lim) -> uint64_t {         // all ones iff row i < lim survived (branch-free)
        return 0ull - (uint64_t)((i < lim ? 1u : 0u) & (uint32_t)((keep[min(i, lim - 1 < 0 ? 0 : lim - 1) >> 6] >> (i & 63)) & 1ull));
    };
    __shared__ unsigned long long rem_word[2][2];          // [iteration parity][c0, c1]: removed bits, double buffered
    __shared__ uint64_t blocks[2][7][64];                  // [iteration parity][block][row]
    if (tid < 4) rem_word[tid >> 1][tid & 1] = 0;
    __syncthreads();
    if (wave > 0) {
        Set mine;
        // reduce the rows whose fate is known (before chunk 2j - 2) and hand iteration j to wavefront 0
        auto publish = [&](int j) {
            const int lim = (2 * j - 2) * 64;
            uint64_t r0 = 0, r1 = 0;                       // (the first use waits for the loads issued three iterations ago)
#pragma unroll
            for (int u = 0; u < GU; ++u) {
                if (u * 320 >= lim) break;                 // (uniform)
                const uint64_t on = alive(u * 320 + gl, lim);
                r0 |= mine.g0[u] & on;
                r1 |= mine.g1[u] & on;
            }
            for (int i0 = GROWS; i0 < lim; i0 += 320) {                        // more than 2560 candidates: not pipelined
                const int i = i0 + gl;
                if (i < lim && ((keep[i >> 6] >> (i & 63)) & 1ull)) {
                    r0 |= mask[(size_t)(2 * j) * cap + i];
                    r1 |= mask[(size_t)min(2 * j + 1, kw - 1) * cap + i];
                }
            }
            if (r0) atomicOr(&rem_word[j & 1][0], (unsigned long long)r0);
            if (r1) atomicOr(&rem_word[j & 1][1], (unsigned long long)r1);
            if (wave <= 3) {
#pragma unroll
                for (int q = 0; q < 7; ++q) blocks[j & 1][q][lane] = mine.blk[q];
            }
        };
        if (grp < niter) issue(grp, mine);
        int turn = grp;
        if (grp == 0 && niter > 0) {
            publish(0);
            if (3 < niter) issue(3, mine);
            turn = 3;
        }
        lds_barrier();
        for (int j = 0; j < niter; ++j) {
            if (j + 1 == turn && turn < niter) {           // (wave-uniform) iteration j + 1 beside wavefront 0's iteration j
                publish(turn);
                if (turn + 3 < niter) issue(turn + 3, mine);
                turn += 3;
            }
            lds_barrier();
        }
    } else {
        // the lowest candidate not removed yet survives and removes its row's bits; repeat until none is left.  Only
        // survivors whose row removes something INSIDE the chunk need a step of the serial loop (two v_readlane and a
        // dependent scalar chain, ~100 cycles): the survivors between two of them are decided in one mask operation --
        // where most candidates survive (the benchmark's scripted heads: ~1000 of 1555) that is 40 -> ~10 steps a chunk
        auto resolve = [&](uint64_t rem, uint64_t dg) -> uint64_t {
            const uint64_t acts = __ballot(dg != 0);                           // rows that remove anything in this chunk
            uint64_t kept = 0;
            uint64_t avail = ~rem;
            for (;;) {
                const uint64_t cand = avail & acts;
                if (!cand) break;
                const int b = __builtin_ctzll(cand);
                const uint64_t row = readlane64(dg, b);
                kept |= avail & ((2ull << b) - 1ull);                          // b and the row-less survivors below it
                avail &= ~row & (~1ull << b);                                  // rows only carry bits above b
            }
            return kept | avail;
        };
        uint64_t kp0 = 0, kp1 = 0;                                             // survivors of the previous iteration's chunks
        lds_barrier();
        for (int j = 0; j < niter; ++j) {
            const int c0 = 2 * j, c1 = 2 * j + 1;
            unsigned long long* rw = rem_word[j & 1];
            const uint64_t (*bk)[64] = blocks[j & 1];
            // rows of the previous iteration's survivors: not known yet when the helpers reduced
            if ((kp0 >> lane) & 1ull) {
                const uint64_t a0 = bk[0][lane], a1 = bk[1][lane];
                if (a0) atomicOr(&rw[0], (unsigned long long)a0);
                if (a1) atomicOr(&rw[1], (unsigned long long)a1);
            }
            if ((kp1 >> lane) & 1ull) {
                const uint64_t b0 = bk[2][lane], b1 = bk[3][lane];
                if (b0) atomicOr(&rw[0], (unsigned long long)b0);
                if (b1) atomicOr(&rw[1], (unsigned long long)b1);
            }
            const uint64_t d0 = bk[4][lane], od = bk[5][lane], d1 = bk[6][lane];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            uint64_t rem0 = readfirstlane64(rw[0]);
            if (c0 == kw - 1 && (K & 63)) rem0 |= ~0ull << (K & 63);           // rows beyond K do not exist
            const uint64_t kept0 = resolve(rem0, d0);
            uint64_t kept1 = 0;
            if (c1 < kw) {
                // chunk c0's survivors remove their rows' bits of word c1
                if (((kept0 >> lane) & 1ull) && od) atomicOr(&rw[1], (unsigned long long)od);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                uint64_t rem1 = readfirstlane64(rw[1]);
                if (c1 == kw - 1 && (K & 63)) rem1 |= ~0ull << (K & 63);
                kept1 = resolve(rem1, d1);
            }
            if (lane == 0) {
                keep[c0] = kept0;
                if (c1 < kw) keep[c1] = kept1;
                rw[0] = 0;
                rw[1] = 0;
            }
            kp0 = kept0;
            kp1 = kept1;
            lds_barrier();
        }
    }
    // final filter of the survivors, in order: slices of 1024 rows
    __shared__ int base;
    __shared__ int wave_cnt[16];
    if (tid == 0) base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < K; i0 += 1024) {
        const int i = i0 + tid;
        float r[8];
        if (i0 < 2048) {
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = i0 == 0 ? pre[0][e] : pre[1][e];
        } else {
            load_row(sorted, min(i, K - 1), r);
        }
        double t[4];
        const bool ok = i < K && ((keep[i >> 6] >> (i & 63)) & 1ull) && box_filter(r[0], r[1], r[2], r[3], out.max_area, out.min_ar, t);
        emit_in_order<16>(ok, t, r, &base, wave_cnt, out);
    }
    if (tid == 0) report(counters, out.counters_host, base, 0);                // (final: never "declined")
}

// ------------------------------------------------------------------------------------ greedy route, survivor by survivor
// Round 4.  The bit matrix + chunked scan above cost 10 + 20 us on an idle GPU and 42 + 88 us inside the pipelined step:
// every dependent trip to memory takes microseconds there (the detector and ReID networks keep the memory system
// saturated), the scan makes one per 64 candidates, and the bit matrix does K^2 / 2 pair tests whatever the outcome.
// This kernel is the reference's greedy loop itself (rect.py:199-244) on the SORTED candidate list, one round per
// SURVIVOR, for up to 4096 candidates in one workgroup of modest footprint (8 wavefronts, <= 128 registers, a few KB .. 64 KB of LDS: it finds room on a
// busy GPU; a 1024-thread / 113 KB first version with the sort inside waited a millisecond for an empty CU):
//   * thread t keeps the sorted candidates t, t + 512, ... in registers (box, class) and their alive bits;
//   * a round: the survivor's box is broadcast from LDS, every thread tests its own alive candidates of that class
//     behind it (diou_pretest; the close calls are collected and get diou_suppresses one at a time), the alive bits go
//     to a 64-word bitmap by ballot, wavefront 0 finds the next alive candidate: two barriers;
//   * the survivors are filtered (box_filter) and written in order at the end.
// Memory is touched three times: sorted rows in, the survivors' confidences in, detections out.  Cost ~ (survivors) x
// ~0.2 us instead of K^2 / 2 pair tests + K / 64 memory round trips: what a real detector produces (tens of objects, a few
// hundred candidates) and the benchmark's dense regime (1500 -> a handful) finish in a few us; all-disjoint boxes degrade
// linearly.  More candidates than the launch provided LDS for (kmax, chosen from the previous pass): the kernel reports
// "declined" and collect() runs the bit matrix + scan for that pass.
constexpr int NG_T = 512, NG_CPT = 8, NG_NW = NG_T / 64, NG_KMAX = NG_T * NG_CPT;
static inline size_t ng_lds_bytes(int kmax) { return (size_t)kmax * 20 + 64 * 8 + 64; }
constexpr int NG_MAX_ROUNDS = 96;      // survivors the greedy kernel resolves before it hands the pass to the bit matrix + scan

__global__ __launch_bounds__(NG_T, 4) void nms_greedy_kernel(const float* __restrict__ sorted, int32_t* __restrict__ counters,
                                                          int cap, int kmax, double thresh, const PostOut out) {
    __builtin_amdgcn_s_setprio(3);
    extern __shared__ __attribute__((aligned(16))) char ng_sm[];
    float4* sbox = reinterpret_cast<float4*>(ng_sm);                              // [kmax] boxes in sorted order
    float* scls = reinterpret_cast<float*>(ng_sm + (size_t)kmax * 16);            // [kmax] their classes
    uint64_t* alive_w = reinterpret_cast<uint64_t*>(ng_sm + (size_t)kmax * 20);   // [64] bitmap of the sorted list
    int32_t* misc = reinterpret_cast<int32_t*>(ng_sm + (size_t)kmax * 20 + 512);  // [0] current survivor, [1] base, [2 .. 2 + NG_NW) wave counts
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = min(counters[0], cap);
    if (K > kmax) {                                      // (uniform) not handled here: the host runs the general route
        if (tid == 0) report(counters, out.counters_host, 0, 1);
        return;
    }
    // ---- the thread's share of the sorted list: candidates tid + NG_T u; wavefront w owns bitmap words w + NG_NW u
    float4 box[NG_CPT];
    float cls[NG_CPT];
    unsigned alive = 0, kept = 0;                        // bit u: candidate tid + NG_T u is alive / is a survivor
#pragma unroll
    for (int u = 0; u < NG_CPT; ++u) {
        const int j = tid + NG_T * u;
        const float* r = sorted + (size_t)min(j, max(K - 1, 0)) * 8;
        box[u] = *reinterpret_cast<const float4*>(r);
        cls[u] = r[5];
    }
#pragma unroll
    for (int u = 0; u < NG_CPT; ++u) {
        const int j = tid + NG_T * u;
        alive |= (j < K ? 1u : 0u) << u;
        if (j < K) { sbox[j] = box[u]; scls[j] = cls[u]; }
        const uint64_t bal = __ballot(j < K);
        if (lane == 0) alive_w[wave + NG_NW * u] = bal;
    }
    if (tid == 0) misc[0] = K > 0 ? 0 : -1;
    __syncthreads();
    // ---- one round per survivor (at most NG_MAX_ROUNDS: a frame whose candidates mostly SURVIVE -- hundreds of rounds --
    // is cheaper through the bit matrix + scan; the pass is then declined like one with too many candidates)
    for (int round = 0;; ++round) {
        const int s = __builtin_amdgcn_readfirstlane(misc[0]);
        if (s < 0) break;
        if (round >= NG_MAX_ROUNDS) {                    // (uniform)
            if (tid == 0) report(counters, out.counters_host, 0, 2);
            return;
        }
        const float4 a4 = sbox[s];
        const Keeper ka = keeper_of(a4.x, a4.y, a4.z, a4.w);
        const float a_cls = scls[s];
        // float32 stages for the thread's candidates (unrolled), the close calls are collected in `need` and get the
        // reference's float64 arithmetic one at a time below: ONE copy of that code (pow() included)
        unsigned need = 0;
#pragma unroll
        for (int u = 0; u < NG_CPT; ++u) {
            const int j = tid + NG_T * u;
            if (j == s) kept |= 1u << u;
            if (((alive >> u) & 1u) && j > s && cls[u] == a_cls) {
                const float4 c = box[u];
                const PairVerdict v = diou_pretest(ka, c.x, c.y, c.z, c.w, (float)thresh);
                if (v == PAIR_SUPPRESSED) alive &= ~(1u << u);
                else if (v == PAIR_CLOSE) need |= 1u << u;
            }
        }
        while (need) {
            const int u = __builtin_ctz(need);
            need &= need - 1;
            const float4 c = sbox[tid + NG_T * u];       // (from LDS: indexing the register copies by a run-time u
                                                         //  would move them to scratch memory)
            if (diou_suppresses_call(a4.x, a4.y, a4.z, a4.w, c.x, c.y, c.z, c.w, thresh)) alive &= ~(1u << u);
        }
#pragma unroll
        for (int u = 0; u < NG_CPT; ++u) {
            const uint64_t bal = __ballot((alive >> u) & 1u);
            if (lane == 0) alive_w[wave + NG_NW * u] = bal;
        }
        __syncthreads();
        if (wave == 0) {
            // next alive candidate behind s: lane l looks at bitmap word l
            uint64_t w = alive_w[lane];
            const int ws = s >> 6;
            if (lane < ws) w = 0;
            else if (lane == ws) w &= (s & 63) == 63 ? 0ull : (~0ull << ((s & 63) + 1));
            const uint64_t nz = __ballot(w != 0);
            int next = -1;
            if (nz) {
                const int fl = __builtin_ctzll(nz);
                next = fl * 64 + __builtin_ctzll(readlane64(w, fl));
            }
            if (lane == 0) misc[0] = next;
        }
        __syncthreads();
    }
    // ---- final filter of the survivors, in sorted order: slices of NG_T rows (their confidences are read from `sorted`
    // for the rows that pass only)
    if (tid == 0) misc[1] = 0;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NG_CPT; ++u) {
        if ((int)NG_T * u >= K) break;                   // (uniform)
        double t[4];
        const bool ok = ((kept >> u) & 1u) && box_filter(box[u].x, box[u].y, box[u].z, box[u].w, out.max_area, out.min_ar, t);
        emit_in_order<NG_NW>(ok, t, sorted + (size_t)(tid + NG_T * u) * 8, &misc[1], misc + 2, out);
    }
    if (tid == 0) report(counters, out.counters_host, misc[1], 0);
}
