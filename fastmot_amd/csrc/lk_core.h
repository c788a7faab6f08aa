// Pyramidal Lucas-Kanade (video/lkpyramid.cpp LKTrackerInvoker) on the device: the per-lane primitives, the window sums,
// the per-level tracking step and the kernels built from them.  Included ONCE by flow.hip, inside its anonymous
// namespace, after MAX_LEVELS and FM_SGPR_CAP: the code is part of that translation unit and is compiled with its flags.
//
// Lane g < win*win owns window pixel (g / win, g % win) -- the samples of a window are taken in parallel, and every
// window sum (A11, A12, A22, b1, b2, the error) is accumulated in the sequential (y, x) order of LKTrackerInvoker's scalar
// loops (seq_step: win*win - 1 dependent float32 adds): bit-identical to oracle/cv_oracle.calc_optical_flow_pyr_lk.  (A
// butterfly reduction agrees with the scalar order to ~1e-4 px only -- enough to flip an inlier decision now and then and
// let the keypoint sets of the two implementations drift apart over a clip, tests/test_e2e_parity_gpu.py.)  Everything
// after the sums is arithmetic that every lane of a window repeats on the same values; the control flow (levels skipped,
// iteration counts) is compiled as branches on "any lane" conditions -- which is why ONE wrong lane changes the result of
// the point.
//
// Why this code is built without the SLP vectoriser (rounds 1-2: "LK results differ from call to call while the ReID
// network runs").  Round 3 captured every iteration of disturbed calls of the one-point-per-wavefront kernel
// of the time (lk_diag_kernel below is that kernel, instrumented; scripts/lk_bisect.py, profiles/r03_lk_bisect.txt):
// samples, running sums and broadcast sums were always right; what was wrong was dx of the position update
//     dx = (A12 * b2 - A22 * b1) * Dt,   dy = (A12 * b1 - A11 * b2) * Dt
// in lanes 48..63 only.  The SLP vectoriser had packed the two expressions into v_pk_mul_f32 / v_pk_add_f32, the cross
// terms through `v_pk_mul_f32 ... op_sel:[0,1] op_sel_hi:[1,0]` (low result from the HIGH register of a source pair);
// on MI355X that instruction form returns a wrong low half in the last 16 lanes of the wavefront now and then while
// wavefronts of the fused LightConv kernels (or of two streamed-conv variants) are resident on the same CU -- never
// when idle, never with unpacked v_mul_f32 / v_sub_f32 (csrc/diag.hip reproduces it stand alone: 0 of 72 M evaluations
// idle, ~25 k wrong lanes beside litechain_kernel, all in lanes 48..63, all in the low half).  A wrong dx in lanes
// 48..63 then ends (or prolongs) the iteration through the any-lane branch: positions off by 1e-4 .. 6 px.
// Consequence: flow.hip is compiled with -fno-slp-vectorize (build.py FILE_FLAGS: no packed fp32 in the KLT kernels; 0
// disagreeing lanes in 5.1 M iterations under the same load), tests/test_isa_lint.py refuses the instruction form in
// every kernel of the library, and the launch needs neither whole CUs nor an ordering against the ReID network.
#pragma once

struct LKArgs {
    const uint8_t* I[MAX_LEVELS];
    const uint8_t* J[MAX_LEVELS];
    const int16_t* D[MAX_LEVELS];
    int w[MAX_LEVELS], h[MAX_LEVELS];
    int levels, win, max_count;
    float eps2, min_eig_thresh;
};

// ---- per-lane primitives
#define LK_DESCALE(x, n) (((x) + (1 << ((n)-1))) >> (n))

__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

__device__ __forceinline__ int lk_px(const uint8_t* __restrict__ row, int c) { return row[c]; }

// the window pixel a lane owns, and the fixed-point bilinear weights of a sub-pixel offset (fa, fb)
struct LKLane { int wx, wy; };
struct LKWeights { int w00, w01, w10, w11; };

__device__ __forceinline__ LKWeights lk_weights(float fa, float fb) {
    LKWeights iw;
    iw.w00 = __float2int_rn((1.f - fa) * (1.f - fb) * (1 << 14));
    iw.w01 = __float2int_rn(fa * (1.f - fb) * (1 << 14));
    iw.w10 = __float2int_rn((1.f - fa) * fb * (1 << 14));
    iw.w11 = (1 << 14) - iw.w00 - iw.w01 - iw.w10;
    return iw;
}

// bilinear sample of image `img` at the lane's pixel of the window whose corner is (bx, by)
__device__ __forceinline__ int lk_sample(const uint8_t* img, int w, int h, int bx, int by, LKLane ln, LKWeights iw) {
    const uint8_t* r0 = img + (size_t)reflect101(by + ln.wy, h) * w;
    const uint8_t* r1 = img + (size_t)reflect101(by + ln.wy + 1, h) * w;
    const int c0 = reflect101(bx + ln.wx, w), c1 = reflect101(bx + ln.wx + 1, w);
    return LK_DESCALE(lk_px(r0, c0) * iw.w00 + lk_px(r0, c1) * iw.w01 + lk_px(r1, c0) * iw.w10 + lk_px(r1, c1) * iw.w11, 14 - 5);
}

// the same interpolation of the Scharr pair of derivative image D, which is zero outside (BORDER_CONSTANT): -> (ixval, iyval)
__device__ __forceinline__ int2 lk_scharr(const int16_t* D, int w, int h, int bx, int by, LKLane ln, LKWeights iw) {
    const int xx0 = bx + ln.wx, xx1 = xx0 + 1, yy0 = by + ln.wy, yy1 = yy0 + 1;
    auto dv = [&](int xx, int yy) -> int2 {
        if (xx < 0 || xx >= w || yy < 0 || yy >= h) return make_int2(0, 0);
        const int v = *reinterpret_cast<const int*>(D + ((size_t)yy * w + xx) * 2);
        return make_int2((int)(short)(v & 0xffff), (int)(short)(v >> 16));
    };
    const int2 d00 = dv(xx0, yy0), d01 = dv(xx1, yy0), d10 = dv(xx0, yy1), d11 = dv(xx1, yy1);
    return make_int2(LK_DESCALE(d00.x * iw.w00 + d01.x * iw.w01 + d10.x * iw.w10 + d11.x * iw.w11, 14),
                     LK_DESCALE(d00.y * iw.w00 + d01.y * iw.w01 + d10.y * iw.w10 + d11.y * iw.w11, 14));
}

// ---- window sums: float32 sum of lanes 0..N-1 in lane order, starting from 0.f like the scalar loops of lkpyramid.cpp.
// Sequential inclusive scan over the lanes: every step adds the left neighbour's running value (DPP wave_shr:1,
// lane 0 reads 0) to the lane's own term, a(s)[i] = a(s-1)[i-1] + v[i].  By induction lane i holds
// ((v0 + v1) + ...) + vi after step i and keeps it, so N-1 steps leave the scalar-order sum in lane N-1: the
// same N-1 dependent float32 adds as the scalar loop, one VALU instruction each (round 2's first version walked
// the lanes with v_readlane: 2 instructions + an SGPR round trip per term).
__device__ __forceinline__ float seq_step(float acc, float v) {
    const int left = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, acc), 0x138 /* wave_shr:1 */, 0xf, 0xf, true);
    return __builtin_bit_cast(float, left) + v;
}
// one / two / three independent sums, their scans interleaved step by step (a DPP read of a VGPR written by the previous
// VALU instruction costs wait states; the neighbouring chain fills them).  a*: the lanes' running sums after the scan,
// lane i = v0 + .. + vi.
template <int N>
__device__ __forceinline__ void seq_scan1(float v0, float& a0) {
    a0 = v0;
#pragma unroll
    for (int k = 1; k < N; ++k) a0 = seq_step(a0, v0);
}
template <int N>
__device__ __forceinline__ void seq_scan2(float v0, float v1, float& a0, float& a1) {
    a0 = v0; a1 = v1;
#pragma unroll
    for (int k = 1; k < N; ++k) { a0 = seq_step(a0, v0); a1 = seq_step(a1, v1); }
}
template <int N>
__device__ __forceinline__ void seq_scan3(float v0, float v1, float v2, float& a0, float& a1, float& a2) {
    a0 = v0; a1 = v1; a2 = v2;
#pragma unroll
    for (int k = 1; k < N; ++k) { a0 = seq_step(a0, v0); a1 = seq_step(a1, v1); a2 = seq_step(a2, v2); }
}

// Two points per wavefront: lanes 0..N-1 carry the window of point 2 w, lanes 32..32+N-1 the window of point 2 w + 1; the
// lanes behind each window LEAVE the kernel at once.  That is what lets the DPP scans of the two windows run in the same
// instructions: a lane whose left neighbour is masked off reads 0 (bound_ctrl), exactly like lane 0 whose neighbour does
// not exist, so the scan restarts at lane 32 by itself.  The broadcast of a sum comes from lane N-1 of the own half
// (ds_bpermute instead of v_readlane).
__device__ __forceinline__ float half_value(float v, int lane_in_half, int half_base) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((half_base + lane_in_half) << 2, __builtin_bit_cast(int, v)));
}
template <int N>
struct LKHalfSums {
    int hb;                                     // first lane of the own half: 0 or 32
    __device__ __forceinline__ float last(float a) const { return half_value(a, N - 1, hb); }
    __device__ __forceinline__ void sum3(float v0, float v1, float v2, float& s0, float& s1, float& s2) const {
        float a0, a1, a2;
        seq_scan3<N>(v0, v1, v2, a0, a1, a2);
        s0 = last(a0); s1 = last(a1); s2 = last(a2);
    }
    __device__ __forceinline__ void sum2(float v0, float v1, float& s0, float& s1) const {
        float a0, a1;
        seq_scan2<N>(v0, v1, a0, a1);
        s0 = last(a0); s1 = last(a1);
    }
    __device__ __forceinline__ float sum1(float v0) const {
        float a0;
        seq_scan1<N>(v0, a0);
        return last(a0);
    }
};

// ---- the J-patch (round 5): the iteration's samples of the NEW frame come from a 16 x 16 byte patch of the level in LDS,
// filled once per (point, level) around the start position (+-5 px of travel inside a level; a window that leaves the
// patch falls back to the global loads).  An iteration then waits for four ds_read_u8 (~100 cycles) instead of four
// global byte loads (~500-700 cycles beside the networks); the values, and with them every result, are the same (sampling
// from global memory alone measured equal within the spread: profiles/r05_lk_patch_and_ring_depth_ab.txt).
// The patch is private to a half-wavefront: a wavefront's LDS operations execute in program order, no barrier is needed
// (and none is possible: lanes leave early and the two halves diverge).
constexpr int LK_PW = 16, LK_PR = 5;

template <int WINC>
struct LKPatch {
    uint8_t* patch;                             // LK_PW x LK_PW bytes of LDS
    int g;                                      // lane in the half-wavefront, < WINC * WINC
    LKLane ln;
    int sx0 = 0, sy0 = 0;                       // top-left corner of the patch in level coordinates
    bool have_patch = false;

    // patch[r][c] = img[reflect101(y0 + r)][reflect101(x0 + c)]: 64 dwords, three per lane.  Inside the image a dword is two
    // ALIGNED loads and a byte alignment; at the borders four byte loads with the reflection lk_sample applies.
    __device__ __forceinline__ void fill(const uint8_t* img, int w, int h, int x0, int y0) {
        sx0 = x0; sy0 = y0;
        const bool inside = x0 >= 0 && x0 + LK_PW + 4 <= w;
        for (int item = g; item < LK_PW * LK_PW / 4; item += WINC * WINC) {
            const int r = item >> 2, c = (item & 3) * 4;
            const uint8_t* row = img + (size_t)reflect101(y0 + r, h) * w;
            uint32_t v;
            if (inside) {
                const uintptr_t ad = reinterpret_cast<uintptr_t>(row) + (uintptr_t)(x0 + c);
                const uint32_t* al = reinterpret_cast<const uint32_t*>(ad & ~uintptr_t(3));
                v = __builtin_amdgcn_alignbyte(al[1], al[0], (uint32_t)(ad & 3));
            } else {
                v = (uint32_t)row[reflect101(x0 + c, w)] | (uint32_t)row[reflect101(x0 + c + 1, w)] << 8 |
                    (uint32_t)row[reflect101(x0 + c + 2, w)] << 16 | (uint32_t)row[reflect101(x0 + c + 3, w)] << 24;
            }
            *reinterpret_cast<uint32_t*>(patch + r * LK_PW + c) = v;
        }
        have_patch = true;
    }
    // lk_sample of the image the patch was filled from: out of the patch when the (win + 1)^2 pixels of the window lie
    // inside it
    __device__ __forceinline__ int sample(const uint8_t* img, int w, int h, int bx, int by, LKWeights iw) const {
        if (have_patch && bx >= sx0 && by >= sy0 && bx + WINC + 1 <= sx0 + LK_PW && by + WINC + 1 <= sy0 + LK_PW) {
            const uint8_t* q = patch + (by - sy0 + ln.wy) * LK_PW + (bx - sx0 + ln.wx);
            return LK_DESCALE((int)q[0] * iw.w00 + (int)q[1] * iw.w01 + (int)q[LK_PW] * iw.w10 + (int)q[LK_PW + 1] * iw.w11, 14 - 5);
        }
        return lk_sample(img, w, h, bx, by, ln, iw);
    }
};

// ---- one level of one point: everything that follows the tracked position (nx, ny), which arrives scaled to `level`.
// The level's template terms -- the lane's sample of the previous frame `ival`, its derivatives `ixval` / `iyval` and the
// raw window sums A11 / A12 / A22 of their products -- are functions of the original point and the level alone; the
// kernels below differ only in where they take them from.  `sums`: the window-sum policy, `pj`: the sampler of the new
// frame J.  -> the point's status; (nx, ny) is written once, with the level's result, and stays as it is when the level
// does not pass the gate (LKTrackerInvoker's `continue`).  (The status goes in and out by value and the iteration moves
// a copy of the position: a bool behind a reference stays a byte in a vector register instead of a lane mask.)
template <int WINC, class Sums, class JSampler>
__device__ __forceinline__ bool lk_level_track(const LKArgs& a, int level, int w, int h, const uint8_t* J, int ival,
                                               int ixval, int iyval, float A11, float A12, float A22, const Sums& sums,
                                               JSampler& pj, float& nx, float& ny, bool st, float& er) {
    constexpr int win = WINC;
    const float half = (win - 1) * 0.5f;
    const float FLT_SCALE = 1.f / (1 << 20);
    pj.have_patch = false;
    A11 *= FLT_SCALE; A12 *= FLT_SCALE; A22 *= FLT_SCALE;
    float Dt = A11 * A22 - A12 * A12;
    const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (2 * win * win);
    if (minEig < a.min_eig_thresh || Dt < 1.1920929e-07f) {
        if (level == 0) st = false;
        return st;
    }
    Dt = 1.f / Dt;
    float x = nx - half, y = ny - half;         // the window's corner
    float pdx = 0.f, pdy = 0.f;
    float outx = x + half, outy = y + half;
    {
        const int fx = (int)floorf(x), fy = (int)floorf(y);
        if (fx >= -win && fx < w && fy >= -win && fy < h) pj.fill(J, w, h, fx - LK_PR, fy - LK_PR);
    }
    for (int j = 0; j < a.max_count; ++j) {
        const int inx = (int)floorf(x), iny = (int)floorf(y);
        if (inx < -win || inx >= w || iny < -win || iny >= h) {
            if (level == 0) st = false;
            break;
        }
        const int diff = pj.sample(J, w, h, inx, iny, lk_weights(x - inx, y - iny)) - ival;
        float b1, b2;
        sums.sum2((float)(diff * ixval), (float)(diff * iyval), b1, b2);
        b1 *= FLT_SCALE; b2 *= FLT_SCALE;
        const float dx = (A12 * b2 - A22 * b1) * Dt, dy = (A12 * b1 - A11 * b2) * Dt;
        x += dx; y += dy;
        outx = x + half; outy = y + half;
        if (dx * dx + dy * dy <= a.eps2) break;
        if (j > 0 && fabsf(dx + pdx) < 0.01f && fabsf(dy + pdy) < 0.01f) {
            outx -= dx * 0.5f; outy -= dy * 0.5f;
            break;
        }
        pdx = dx; pdy = dy;
    }
    nx = outx; ny = outy;
    if (st && level == 0) {
        const float ex = nx - half, ey = ny - half;
        const int inx = (int)floorf(ex), iny = (int)floorf(ey);
        if (inx < -win || inx >= w || iny < -win || iny >= h) return false;
        const int diff = pj.sample(J, w, h, inx, iny, lk_weights(ex - inx, ey - iny)) - ival;
        er = sums.sum1(fabsf((float)diff)) * 1.f / (32 * win * win);
    }
    return st;
}

// the first lane of a window writes the point's result
__device__ __forceinline__ void lk_store(int pt, int g, float nx, float ny, bool st, float er, float* next_pts,
                                         uint8_t* status, float* err) {
    if (g == 0) {
        next_pts[2 * pt] = nx;
        next_pts[2 * pt + 1] = ny;
        status[pt] = st ? 1 : 0;
        err[pt] = er;
    }
}

// ---- two points per wavefront (LKHalfSums, LKPatch), the template terms computed level by level.  The arithmetic is
// per lane, and the control flow -- levels skipped, iteration counts -- is divergent between the halves (the compiler
// masks; nothing is wave-uniform except the level loop).  Half the wavefronts of a one-point-per-wavefront kernel hold
// the registers half as long per point: the kernel's footprint beside the other streams' kernels is what the pipeline
// pays for.  Takes pyramids deeper than LK_PRE levels.
template <int WINC>
__global__ __launch_bounds__(256) FM_SGPR_CAP void lk_pair_kernel(LKArgs a, int n, const float* __restrict__ prev_pts,
                                                                  float* __restrict__ next_pts, uint8_t* __restrict__ status,
                                                                  float* __restrict__ err) {
    __shared__ __attribute__((aligned(16))) uint8_t patch_all[8 * LK_PW * LK_PW];
    const int gidx = blockIdx.x * blockDim.x + threadIdx.x;
    const int l = gidx & 63, g = l & 31, hb = l & 32;
    const int pt = (gidx >> 6) * 2 + (l >> 5);
    constexpr int win = WINC, NW = WINC * WINC;
    if (pt >= n || g >= NW) return;
    const LKLane ln{g % win, g / win};
    const LKHalfSums<NW> sums{hb};
    LKPatch<WINC> pj{patch_all + ((threadIdx.x >> 5) & 7) * (LK_PW * LK_PW), g, ln};
    const float half = (win - 1) * 0.5f;
    const float px0 = prev_pts[2 * pt], py0 = prev_pts[2 * pt + 1];
    float nx = 0.f, ny = 0.f;
    bool st = true;
    float er = 0.f;
    for (int level = a.levels - 1; level >= 0; --level) {
        const int w = a.w[level], h = a.h[level];
        const uint8_t* I = a.I[level];
        const uint8_t* J = a.J[level];
        const int16_t* D = a.D[level];
        const float sc = 1.f / (float)(1 << level);
        float ppx = px0 * sc, ppy = py0 * sc;
        if (level == a.levels - 1) { nx = ppx; ny = ppy; }
        else { nx *= 2.f; ny *= 2.f; }
        ppx -= half; ppy -= half;
        const int ipx = (int)floorf(ppx), ipy = (int)floorf(ppy);
        if (ipx < -win || ipx >= w || ipy < -win || ipy >= h) {
            if (level == 0) { st = false; er = 0.f; }
            continue;
        }
        const LKWeights iw = lk_weights(ppx - ipx, ppy - ipy);
        const int ival = lk_sample(I, w, h, ipx, ipy, ln, iw);
        const int2 dI = lk_scharr(D, w, h, ipx, ipy, ln, iw);
        const int ixval = dI.x, iyval = dI.y;
        float A11, A12, A22;
        sums.sum3((float)(ixval * ixval), (float)(ixval * iyval), (float)(iyval * iyval), A11, A12, A22);
        st = lk_level_track<WINC>(a, level, w, h, J, ival, ixval, iyval, A11, A12, A22, sums, pj, nx, ny, st, er);
    }
    lk_store(pt, g, nx, ny, st, er, next_pts, status, err);
}

// ---- round 6: the same kernel with everything that does NOT depend on the tracked position taken out of the level loop.
// lk_pair_kernel fetches and sums the template terms level by level: per level two dependent trips to memory (~500-700
// cycles each beside the networks) and three 24-step serial scans in front of the first iteration, six times in a row.
// Here all levels' loads are requested at once and the 3 x levels scans run interleaved (18 independent chains: the DPP
// adds issue back to back instead of waiting for each other); the level loop keeps lk_level_track.  Every value is
// computed by the same operations in the same order: bit-identical (tests/test_flow_gpu.py, the e2e parity tests).  Up
// to LK_PRE levels (the reference's maxLevel = 5 gives 6); deeper pyramids take lk_pair_kernel.
constexpr int LK_PRE = 6;

template <int WINC>
__global__ __launch_bounds__(256) FM_SGPR_CAP void lk_pair_pre_kernel(LKArgs a, int n, const float* __restrict__ prev_pts,
                                                                      float* __restrict__ next_pts, uint8_t* __restrict__ status,
                                                                      float* __restrict__ err) {
    __shared__ __attribute__((aligned(16))) uint8_t patch_all[8 * LK_PW * LK_PW];
    const int gidx = blockIdx.x * blockDim.x + threadIdx.x;
    const int l = gidx & 63, g = l & 31, hb = l & 32;
    const int pt = (gidx >> 6) * 2 + (l >> 5);
    constexpr int win = WINC, NW = WINC * WINC;
    if (pt >= n || g >= NW) return;
    const LKLane ln{g % win, g / win};
    const LKHalfSums<NW> sums{hb};
    LKPatch<WINC> pj{patch_all + ((threadIdx.x >> 5) & 7) * (LK_PW * LK_PW), g, ln};
    const float half = (win - 1) * 0.5f;
    const float px0 = prev_pts[2 * pt], py0 = prev_pts[2 * pt + 1];
    float nx = 0.f, ny = 0.f;
    bool st = true;
    float er = 0.f;

    // ---- the template terms of every level
    int ivalL[LK_PRE], ixL[LK_PRE], iyL[LK_PRE];
    bool posok[LK_PRE];
#pragma unroll
    for (int lv = 0; lv < LK_PRE; ++lv) {
        ivalL[lv] = ixL[lv] = iyL[lv] = 0;
        posok[lv] = false;
        if (lv < a.levels) {
            const int w = a.w[lv], h = a.h[lv];
            const float sc = 1.f / (float)(1 << lv);
            const float ppx = px0 * sc - half, ppy = py0 * sc - half;
            const int ipx = (int)floorf(ppx), ipy = (int)floorf(ppy);
            posok[lv] = !(ipx < -win || ipx >= w || ipy < -win || ipy >= h);
            // (a position outside the level is never used: its loads go to a clamped one)
            const int cx = min(max(ipx, -win), w - 1), cy = min(max(ipy, -win), h - 1);
            const LKWeights iw = lk_weights(ppx - ipx, ppy - ipy);
            ivalL[lv] = lk_sample(a.I[lv], w, h, cx, cy, ln, iw);
            const int2 dI = lk_scharr(a.D[lv], w, h, cx, cy, ln, iw);
            ixL[lv] = dI.x; iyL[lv] = dI.y;
        }
    }
    float A11L[LK_PRE], A12L[LK_PRE], A22L[LK_PRE];
    {
        float v0[LK_PRE], v1[LK_PRE], v2[LK_PRE], s0[LK_PRE], s1[LK_PRE], s2[LK_PRE];
#pragma unroll
        for (int lv = 0; lv < LK_PRE; ++lv) {
            s0[lv] = v0[lv] = (float)(ixL[lv] * ixL[lv]);
            s1[lv] = v1[lv] = (float)(ixL[lv] * iyL[lv]);
            s2[lv] = v2[lv] = (float)(iyL[lv] * iyL[lv]);
        }
#pragma unroll
        for (int k = 1; k < NW; ++k)
#pragma unroll
            for (int lv = 0; lv < LK_PRE; ++lv) {
                s0[lv] = seq_step(s0[lv], v0[lv]); s1[lv] = seq_step(s1[lv], v1[lv]); s2[lv] = seq_step(s2[lv], v2[lv]);
            }
#pragma unroll
        for (int lv = 0; lv < LK_PRE; ++lv) {
            A11L[lv] = sums.last(s0[lv]); A12L[lv] = sums.last(s1[lv]); A22L[lv] = sums.last(s2[lv]);
        }
    }

    // ---- coarse to fine: what follows the position
#pragma unroll
    for (int lv = LK_PRE - 1; lv >= 0; --lv) {
        if (lv >= a.levels) continue;
        const float sc = 1.f / (float)(1 << lv);
        if (lv == a.levels - 1) { nx = px0 * sc; ny = py0 * sc; }
        else { nx *= 2.f; ny *= 2.f; }
        if (!posok[lv]) {
            if (lv == 0) { st = false; er = 0.f; }
            continue;
        }
        st = lk_level_track<WINC>(a, lv, a.w[lv], a.h[lv], a.J[lv], ivalL[lv], ixL[lv], iyL[lv], A11L[lv], A12L[lv], A22L[lv],
                                  sums, pj, nx, ny, st, er);
    }
    lk_store(pt, g, nx, ny, st, er, next_pts, status, err);
}

#ifdef FM_DIAG      // diagnostic builds only (FASTMOT_EXTRA_HIPCC_FLAGS=-DFM_DIAG, include/fastmot_hip_diag.h)
// ---- diagnostic variants of the LK kernel (round 3: bisect of the results that differ under load): ONE point
// per wavefront, lanes >= win*win carry zero terms, the sums are broadcast from lane win*win - 1 of the wavefront and the
// control flow is wave-uniform; global loads only.  Its loop is its own: the capture rows and checks sit between all steps.
// MODE 0: window sums as DPP scans (the production arithmetic), 1: through LDS (no cross-lane VALU operation),
// 2: both, compared, re-evaluated on a mismatch (counters say which of the two changed its mind).
// CHK: every image sample is loaded twice (second time through a laundered pointer the compiler cannot merge) and
//      the wave-uniform position update is compared across the lanes.
// CAP: every (level, iteration) appends a record of 8 rows x 64 lanes to `cap`: the lanes' samples, the lanes'
//      running sums after the scan, the broadcast sums, every lane's copy of the position; header = HW_ID / XCC_ID.
// diag[]: 0 sum mismatches (MODE 2), 1 DPP value changed on re-evaluation, 2 LDS value changed, 3 still different
//      after 3 retries, 4 duplicate-load mismatches, 5 lanes disagree on the position, 6 iterations evaluated.
constexpr int LK_CAP_ROWS = 12, LK_CAP_REC = LK_CAP_ROWS * 64, LK_CAP_MAXREC = 80;

__device__ __forceinline__ const uint8_t* launder(const uint8_t* p) {
    asm volatile("" : "+v"(p));
    return p;
}
__device__ __forceinline__ float lane_value(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
__device__ __forceinline__ bool same_bits(float x, float y) { return __builtin_bit_cast(int, x) == __builtin_bit_cast(int, y); }

// The same sums WITHOUT any cross-lane VALU operation: every lane parks its term in the wavefront's LDS slab, then
// every lane reads all N terms back (same address in all lanes: broadcast reads) and adds them in scalar order in its
// own registers -- N - 1 dependent float32 adds per sum again, the result is in every lane by construction.
// LDS operations of one wavefront execute in order; the fences keep the compiler from moving them.
template <int N>
__device__ __forceinline__ float lds_seq(const float* __restrict__ slab) {
    const float4* q = reinterpret_cast<const float4*>(slab);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < N / 4; ++k) {
        const float4 t = q[k];
        acc += t.x; acc += t.y; acc += t.z; acc += t.w;
    }
#pragma unroll
    for (int k = N / 4 * 4; k < N; ++k) acc += slab[k];
    return acc;
}
template <int N, int K>
__device__ __forceinline__ void lds_sums(float* slab, int lane, const float (&v)[K], float (&s)[K]) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (lane < 32) {
#pragma unroll
        for (int k = 0; k < K; ++k) slab[32 * k + lane] = v[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = lds_seq<N>(slab + 32 * k);
    __builtin_amdgcn_wave_barrier();
}

// the whole-wavefront sum policy of the three modes; pfx (capture): the lanes' running sums of the DPP scans
template <int N, int MODE>
struct LKWaveSums {
    float* slab;
    int g;
    int* diag;
    __device__ __forceinline__ void sum2(float v0, float v1, float& s0, float& s1, float* pfx = nullptr) const {
        float d0 = 0.f, d1 = 0.f, a0, a1;
        if (MODE != 1) {
            seq_scan2<N>(v0, v1, a0, a1);
            if (pfx) { pfx[0] = a0; pfx[1] = a1; }
            d0 = lane_value(a0, N - 1); d1 = lane_value(a1, N - 1);
        }
        if (MODE == 0) { s0 = d0; s1 = d1; return; }
        const float v[2] = {v0, v1};
        float l[2];
        lds_sums<N, 2>(slab, g, v, l);
        if (MODE == 2) {
            int tries = 0;
            while ((!same_bits(d0, l[0]) || !same_bits(d1, l[1])) && tries < 3) {
                if (g == 0 && tries == 0) atomicAdd(&diag[0], 1);
                float m[2];
                seq_scan2<N>(v0, v1, a0, a1);
                const float e0 = lane_value(a0, N - 1), e1 = lane_value(a1, N - 1);
                lds_sums<N, 2>(slab, g, v, m);
                if (g == 0) {
                    if (!same_bits(e0, d0) || !same_bits(e1, d1)) atomicAdd(&diag[1], 1);
                    if (!same_bits(m[0], l[0]) || !same_bits(m[1], l[1])) atomicAdd(&diag[2], 1);
                }
                d0 = e0; d1 = e1; l[0] = m[0]; l[1] = m[1];
                ++tries;
            }
            if (tries == 3 && g == 0) atomicAdd(&diag[3], 1);
        }
        s0 = l[0]; s1 = l[1];
    }
    // (three sums = the two-sum helper twice in the LDS / checked modes; the DPP mode keeps the production shape)
    __device__ __forceinline__ void sum3(float v0, float v1, float v2, float& s0, float& s1, float& s2, float* pfx) const {
        if (MODE == 0) {
            seq_scan3<N>(v0, v1, v2, pfx[0], pfx[1], pfx[2]);
            s0 = lane_value(pfx[0], N - 1); s1 = lane_value(pfx[1], N - 1); s2 = lane_value(pfx[2], N - 1);
        } else {
            float s1again;
            sum2(v0, v1, s0, s1, pfx);
            sum2(v2, v1, s2, s1again, pfx + 1);
        }
    }
    __device__ __forceinline__ float sum1(float v0, float* pfx) const {
        if (MODE == 0) {
            seq_scan1<N>(v0, *pfx);
            return lane_value(*pfx, N - 1);
        }
        float s0, s1;
        sum2(v0, 0.f, s0, s1);
        return s0;
    }
};

template <int WINC, int MODE, bool CHK, bool CAP>
__global__ __launch_bounds__(1024) FM_SGPR_CAP void lk_diag_kernel(LKArgs a, int n, const float* __restrict__ prev_pts,
                                                                   float* __restrict__ next_pts, uint8_t* __restrict__ status,
                                                                   float* __restrict__ err, int* __restrict__ diag,
                                                                   int* __restrict__ cap, int* __restrict__ cap_hdr) {
    __shared__ float slab_all[MODE == 0 ? 1 : 16 * 96];
    const int gidx = blockIdx.x * blockDim.x + threadIdx.x;
    const int pt = gidx >> 6, g = gidx & 63;
    if (pt >= n) return;                       // the whole wavefront exits together
    constexpr int win = WINC;
    constexpr int NW = WINC * WINC;
    const bool lane_on = g < NW;
    const LKLane ln{lane_on ? g % win : 0, lane_on ? g / win : 0};
    const LKWaveSums<NW, MODE> sums{slab_all + (MODE == 0 ? 0 : (threadIdx.x >> 6) * 96), g, diag};
    const float half = (win - 1) * 0.5f;
    const float px0 = prev_pts[2 * pt], py0 = prev_pts[2 * pt + 1];
    float nx = 0.f, ny = 0.f;
    bool st = true;
    float er = 0.f;
    const float FLT_SCALE = 1.f / (1 << 20);
    int nrec = 0;
    int* rec0 = CAP ? cap + (size_t)pt * LK_CAP_MAXREC * LK_CAP_REC : nullptr;
    auto put = [&](int row, int v) { if (CAP && nrec < LK_CAP_MAXREC) rec0[(size_t)nrec * LK_CAP_REC + row * 64 + g] = v; };
    auto putf = [&](int row, float v) { put(row, __builtin_bit_cast(int, v)); };
    auto sample = [&](const uint8_t* img, int w, int h, int bx, int by, LKWeights iw) -> int {
        const int v = lk_sample(img, w, h, bx, by, ln, iw);
        if (CHK && lk_sample(launder(img), w, h, bx, by, ln, iw) != v) atomicAdd(&diag[4], 1);
        return v;
    };
    for (int level = a.levels - 1; level >= 0; --level) {
        const int w = a.w[level], h = a.h[level];
        const uint8_t* J = a.J[level];
        const float sc = 1.f / (float)(1 << level);
        float ppx = px0 * sc, ppy = py0 * sc;
        if (level == a.levels - 1) { nx = ppx; ny = ppy; }
        else { nx *= 2.f; ny *= 2.f; }
        ppx -= half; ppy -= half;
        const int ipx = (int)floorf(ppx), ipy = (int)floorf(ppy);
        if (ipx < -win || ipx >= w || ipy < -win || ipy >= h) {
            if (level == 0) { st = false; er = 0.f; }
            continue;
        }
        int ival = 0, ixval = 0, iyval = 0;
        if (lane_on) {
            const LKWeights iw = lk_weights(ppx - ipx, ppy - ipy);
            ival = sample(a.I[level], w, h, ipx, ipy, iw);
            const int2 dI = lk_scharr(a.D[level], w, h, ipx, ipy, ln, iw);
            ixval = dI.x; iyval = dI.y;
        }
        float A11, A12, A22;
        float pfx[3] = {0.f, 0.f, 0.f};
        sums.sum3((float)(ixval * ixval), (float)(ixval * iyval), (float)(iyval * iyval), A11, A12, A22, pfx);
        put(0, ival); put(1, ixval); put(2, iyval); putf(3, pfx[0]); putf(4, pfx[1]); putf(5, pfx[2]);
        putf(6, A11); put(7, (level << 8) | 1);
        ++nrec;
        A11 *= FLT_SCALE; A12 *= FLT_SCALE; A22 *= FLT_SCALE;
        float Dt = A11 * A22 - A12 * A12;
        const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (2 * win * win);
        if (minEig < a.min_eig_thresh || Dt < 1.1920929e-07f) {
            if (level == 0) st = false;
            continue;
        }
        Dt = 1.f / Dt;
        nx -= half; ny -= half;
        float pdx = 0.f, pdy = 0.f;
        float outx = nx + half, outy = ny + half;
        for (int j = 0; j < a.max_count; ++j) {
            const int inx = (int)floorf(nx), iny = (int)floorf(ny);
            if (inx < -win || inx >= w || iny < -win || iny >= h) {
                if (level == 0) st = false;
                break;
            }
            int diff = 0;
            if (lane_on) diff = sample(J, w, h, inx, iny, lk_weights(nx - inx, ny - iny)) - ival;
            float b1, b2;
            float pb[2] = {0.f, 0.f};
            sums.sum2((float)(diff * ixval), (float)(diff * iyval), b1, b2, pb);
            put(0, diff); putf(1, pb[0]); putf(2, pb[1]); putf(5, b1); putf(6, b2); put(7, (level << 8) | (j << 16) | 2);
            b1 *= FLT_SCALE; b2 *= FLT_SCALE;
            const float dx = (A12 * b2 - A22 * b1) * Dt, dy = (A12 * b1 - A11 * b2) * Dt;
            putf(8, nx); putf(9, b1);
            nx += dx; ny += dy;
            putf(3, nx); putf(4, ny); putf(10, dx); putf(11, dy);
            ++nrec;
            if (CHK) {
                if (g == 0) atomicAdd(&diag[6], 1);
                const int fx = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, nx));
                const int fy = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, ny));
                if (__builtin_bit_cast(int, nx) != fx || __builtin_bit_cast(int, ny) != fy) {
                    atomicAdd(&diag[5], 1);
                    atomicAdd(&diag[8 + (g >> 4)], 1);          // which quarter of the wavefront
                }
            }
            outx = nx + half; outy = ny + half;
            if (dx * dx + dy * dy <= a.eps2) break;
            if (j > 0 && fabsf(dx + pdx) < 0.01f && fabsf(dy + pdy) < 0.01f) {
                outx -= dx * 0.5f; outy -= dy * 0.5f;
                break;
            }
            pdx = dx; pdy = dy;
        }
        nx = outx; ny = outy;
        if (st && level == 0) {
            const float ex = nx - half, ey = ny - half;
            const int inx = (int)floorf(ex), iny = (int)floorf(ey);
            if (inx < -win || inx >= w || iny < -win || iny >= h) { st = false; continue; }
            int diff = 0;
            if (lane_on) diff = sample(J, w, h, inx, iny, lk_weights(ex - inx, ey - iny)) - ival;
            float pe = 0.f;
            er = sums.sum1(fabsf((float)diff), &pe) * 1.f / (32 * win * win);
            put(0, diff); putf(1, pe); putf(5, er); put(7, 3);
            ++nrec;
        }
    }
    lk_store(pt, g, nx, ny, st, er, next_pts, status, err);
    if (CAP && g == 0) {
        cap_hdr[4 * pt] = (int)__builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));       // HW_REG_HW_ID
        cap_hdr[4 * pt + 1] = (int)__builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11));  // HW_REG_XCC_ID
        cap_hdr[4 * pt + 2] = nrec;
        cap_hdr[4 * pt + 3] = (int)blockIdx.x;
    }
}
#endif  // FM_DIAG
