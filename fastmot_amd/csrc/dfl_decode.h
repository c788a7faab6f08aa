// Decode of anchor-free heads with a DFL box branch (Ultralytics YOLOv8 `Detect`): device code, included by detect.hip
// inside its anonymous namespace (it uses emit_candidate, FilterArgs, pick_sample and the per-image fields of HeadSet).
//
// A level of stride s with a gh x gw grid ends in two fp32 NHWC tensors (or two channel ranges of one): 4 * 16 box
// logits b[side][k] per cell, sides in the order left, top, right, bottom, and nc class logits.  For cell (row, col):
//     d_side = sum_k k * softmax(b[side])_k                 (the maximum subtracted before the exponential)
//     ax = col + 0.5, ay = row + 0.5
//     x1 = (ax - d_l) s, y1 = (ay - d_t) s, x2 = (ax + d_r) s, y2 = (ay + d_b) s
//     row: x = x1 / in_w, y = y1 / in_h, w = (x2 - x1) / in_w, h = (y2 - y1) / in_h      (top-left corner, as decode_kernel)
//     cls = the FIRST maximum of the class logits, cls_prob = sigmoid(logit), box_conf = 1
//     orig = the anchor's index in level-major order (Ultralytics' make_anchors)
// and the row goes through emit_candidate like every other: class mask, score >= conf_thresh, scale and offset.
//
// dfl_decode_kernel: 16 lanes per cell, four cells per wavefront.  A cell's class logits are read as float4s strided
// over the 16 lanes and reduced to the first maximum with four shuffles; most cells end there, because the score test
// -- emit_candidate's own comparison, on the same value -- fails.  For the others lane j holds one float4 of the box
// bins (side j / 4, bins 4 (j % 4) ..): two shuffles give the side's maximum, two more the sums.  All loads of a cell are
// 16-byte and contiguous over the lanes; no LDS, no scratch.
// dfl_decode_cell_kernel: the same arithmetic in the same order with one thread per cell (each lane walks its cell's
// channels alone): the A/B partner of scripts/yolov8_timing.py, selected by the fm_ctx option "dfl_decode_form" = 1.
// Both forms add in the order: four bins of a quarter side left to right, then quarters (0 + 1) + (2 + 3); they produce
// the same bits.
// Arithmetic: fp32, -ffp-contract=off, __expf as in decode_kernel; the bound is derived in tests/yolov8_ref.py.
#pragma once

#define FM_DFL_BINS 16

struct DflHead {
    const float* box;    // NHWC fp32, channel box_coff + side * 16 + k
    const float* cls;    // NHWC fp32, channel cls_coff + class
    int box_cs, box_coff, cls_cs, cls_coff;
    int gw, gh, base_index;
    float stride;
};

struct DflSet {
    DflHead h[FM_MAX_HEADS];
    int first_block[FM_MAX_HEADS + 1];   // level i owns blocks [first_block[i], first_block[i + 1])
};

// the expectation's two sums over one quarter of a side: bins k0 .. k0 + 3, maximum m of the whole side
__device__ __forceinline__ void dfl_quarter(const float4 v, int k0, float m, float& num, float& den) {
    const float e0 = __expf(v.x - m), e1 = __expf(v.y - m), e2 = __expf(v.z - m), e3 = __expf(v.w - m);
    den = ((e0 + e1) + e2) + e3;
    num = (((float)k0 * e0 + (float)(k0 + 1) * e1) + (float)(k0 + 2) * e2) + (float)(k0 + 3) * e3;
}

__device__ __forceinline__ void dfl_emit(const FilterArgs& fa, const DflHead& h, int cell, float dl, float dt, float dr, float db,
                                         int cls, float cls_prob, int in_w, int in_h) {
    const int row = cell / h.gw, col = cell - row * h.gw;
    const float ax = (float)col + 0.5f, ay = (float)row + 0.5f;
    // (each product on its own: the SLP vectoriser pairs them into v_pk_mul_f32 with a cross-half op_sel, the form
    // tests/test_isa_lint.py keeps out of the library -- DESIGN 5b; the empty asm only ties the value to a register)
    float x1 = (ax - dl) * h.stride, y1 = (ay - dt) * h.stride;
    asm volatile("" : "+v"(x1));
    asm volatile("" : "+v"(y1));
    float x2 = (ax + dr) * h.stride, y2 = (ay + db) * h.stride;
    asm volatile("" : "+v"(x2));
    asm volatile("" : "+v"(y2));
    emit_candidate(fa, x1 / in_w, y1 / in_h, (x2 - x1) / in_w, (y2 - y1) / in_h, 1.0f, cls, cls_prob, h.base_index + cell);
}

// what emit_candidate will decide from (cls, cls_prob) at box_conf = 1: the box branch is read only behind it
__device__ __forceinline__ bool dfl_passes(const FilterArgs& fa, int cls, float cls_prob) {
    if (cls < 0 || cls >= 128 || !fa.label_mask[cls]) return false;
    return 1.0f * cls_prob >= fa.conf_thresh;
}

__device__ __forceinline__ int dfl_level(const DflSet& ds) {
    int hi = 0;
#pragma unroll
    for (int i = 1; i < FM_MAX_HEADS; ++i) hi += (int)blockIdx.x >= ds.first_block[i] ? 1 : 0;
    return hi;
}

__device__ __forceinline__ void dfl_image(const HeadSet& hs, FilterArgs& fa, int img) {
    fa.cand = pick_sample(hs.cand, img);
    fa.counters = pick_sample(hs.counters, img);
    fa.offset[0] = pick_sample(hs.off_x, img);
    fa.offset[1] = pick_sample(hs.off_y, img);
}

// 256 threads = 16 cells; blockIdx.y: the image of a batched pass (hs: only its per-image fields are used)
__global__ void __launch_bounds__(256) dfl_decode_kernel(DflSet ds, HeadSet hs, FilterArgs fa, int in_w, int in_h) {
    const int hi = dfl_level(ds);
    const DflHead& h = ds.h[hi];
    const int j = threadIdx.x & 15;
    const int cell = ((int)blockIdx.x - ds.first_block[hi]) * 16 + ((int)threadIdx.x >> 4);
    const int cells = h.gw * h.gh;
    if (cell >= cells) return;             // (whole 16-lane groups: the shuffles below never leave a group)
    const int img = blockIdx.y;
    dfl_image(hs, fa, img);
    const int nc = fa.num_classes;
    const float* pc = h.cls + ((size_t)img * cells + cell) * h.cls_cs + h.cls_coff;
    int cls = 0;
    float best = -INFINITY;
    // the lane's own logits in ascending order with the strict comparison (the first maximum wins) ...
    for (int i = 4 * j; i < nc; i += 64) {
        if (i + 4 <= nc) {
            const float4 v = *reinterpret_cast<const float4*>(pc + i);
            if (v.x > best) { best = v.x; cls = i; }
            if (v.y > best) { best = v.y; cls = i + 1; }
            if (v.z > best) { best = v.z; cls = i + 2; }
            if (v.w > best) { best = v.w; cls = i + 3; }
        } else {
            for (int k = i; k < nc; ++k) {
                const float l = pc[k];
                if (l > best) { best = l; cls = k; }
            }
        }
    }
    // ... then over the 16 lanes: the larger value, among equals the lower index
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) {
        const float ob = __shfl_xor(best, m, 16);
        const int oc = __shfl_xor(cls, m, 16);
        if (ob > best || (ob == best && oc < cls)) { best = ob; cls = oc; }
    }
    const float cls_prob = sigmoid_fast(best);
    if (!dfl_passes(fa, cls, cls_prob)) return;     // (the same in all 16 lanes of the cell)
    const float* pb = h.box + ((size_t)img * cells + cell) * h.box_cs + h.box_coff;
    const float4 v = *reinterpret_cast<const float4*>(pb + 4 * j);
    float m = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
    m = fmaxf(m, __shfl_xor(m, 1, 16));
    m = fmaxf(m, __shfl_xor(m, 2, 16));
    float num, den;
    dfl_quarter(v, 4 * (j & 3), m, num, den);
    num += __shfl_xor(num, 1, 16); den += __shfl_xor(den, 1, 16);
    num += __shfl_xor(num, 2, 16); den += __shfl_xor(den, 2, 16);
    const float d = num / den;
    const float dl = __shfl(d, 0, 16), dt = __shfl(d, 4, 16), dr = __shfl(d, 8, 16), db = __shfl(d, 12, 16);
    if (j == 0) dfl_emit(fa, h, cell, dl, dt, dr, db, cls, cls_prob, in_w, in_h);
}

// one thread per cell, 256 cells per block
__global__ void __launch_bounds__(256) dfl_decode_cell_kernel(DflSet ds, HeadSet hs, FilterArgs fa, int in_w, int in_h) {
    const int hi = dfl_level(ds);
    const DflHead& h = ds.h[hi];
    const int cell = ((int)blockIdx.x - ds.first_block[hi]) * 256 + (int)threadIdx.x;
    const int cells = h.gw * h.gh;
    if (cell >= cells) return;
    const int img = blockIdx.y;
    dfl_image(hs, fa, img);
    const int nc = fa.num_classes;
    const float* pc = h.cls + ((size_t)img * cells + cell) * h.cls_cs + h.cls_coff;
    int cls = 0;
    float best = -INFINITY;
    int i = 0;
    for (; i + 4 <= nc; i += 4) {
        const float4 v = *reinterpret_cast<const float4*>(pc + i);
        if (v.x > best) { best = v.x; cls = i; }
        if (v.y > best) { best = v.y; cls = i + 1; }
        if (v.z > best) { best = v.z; cls = i + 2; }
        if (v.w > best) { best = v.w; cls = i + 3; }
    }
    for (; i < nc; ++i) {
        const float l = pc[i];
        if (l > best) { best = l; cls = i; }
    }
    const float cls_prob = sigmoid_fast(best);
    if (!dfl_passes(fa, cls, cls_prob)) return;
    const float* pb = h.box + ((size_t)img * cells + cell) * h.box_cs + h.box_coff;
    float d[4];
#pragma unroll
    for (int side = 0; side < 4; ++side) {
        float4 q[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) q[t] = *reinterpret_cast<const float4*>(pb + side * FM_DFL_BINS + 4 * t);
        float qm[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) qm[t] = fmaxf(fmaxf(q[t].x, q[t].y), fmaxf(q[t].z, q[t].w));
        const float m = fmaxf(fmaxf(qm[0], qm[1]), fmaxf(qm[2], qm[3]));
        float num[4], den[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) dfl_quarter(q[t], 4 * t, m, num[t], den[t]);
        d[side] = ((num[0] + num[1]) + (num[2] + num[3])) / ((den[0] + den[1]) + (den[2] + den[3]));
    }
    dfl_emit(fa, h, cell, d[0], d[1], d[2], d[3], cls, cls_prob, in_w, in_h);
}
