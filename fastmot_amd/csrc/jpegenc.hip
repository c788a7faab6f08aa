// Packed BGR u8 -> baseline JPEG (8-bit, YCbCr 4:2:0, Annex-K Huffman tables, JFIF): the device half of the output path,
// behind fm_frame_encode_jpeg (the frame the context holds on the device) and fm_jpeg_encode_bgr (host pixels through a
// staging buffer).  jpegenc_host.hip writes the marker segments and gathers what the kernels here leave in page-locked
// memory; DESIGN 11f describes the whole path.
//
// The file has a restart interval of one MCU row, so every MCU row is a segment of its own: its DC predictors start at
// zero and it ends on a byte boundary, padded with 1-bits.  That makes the entropy coder -- serial by construction in a
// file without restarts -- parallel over rows, and inside a row the only dependence between blocks is where a block's
// bits start, which a prefix sum over the blocks' bit lengths gives.
//
// The arithmetic is libjpeg's, integer and exact (tests/jpegenc_ref.py states it in numpy; the tests compare files and
// coefficients with Pillow's): 16-bit fixed-point colour conversion, edge replication to the MCU grid (below the image the
// chroma repeats its last averaged row, not the last pixel row), 2 x 2 chroma averaging with the alternating bias, the "islow" forward DCT on samples - 128 (rows first, 13-bit constants, two extra
// bits kept between the passes, output scaled by 8), division by 8 x the quantisation value rounded half away from zero;
// a luma block that lies wholly outside the image's own block grid is a dummy: AC zero, DC that of the block before it.
//
// Five launches on the encoder's own stream:
//   jpegenc_fdct_kernel    one wavefront per MCU (four per workgroup): 16 x 16 pixels -> Y / Cb / Cr in LDS, chroma
//                          averaged, 48 row passes and 48 column passes of the DCT on 48 lanes, quantisation; writes the
//                          six blocks in coded order (Y00 Y01 Y10 Y11 Cb Cr), each in zig-zag order, 64 lanes x 2 bytes.
//   jpegenc_scan_kernel    one workgroup per MCU row: bit length of every block (a thread walks a run of blocks), a
//                          workgroup prefix sum, the blocks' bit offsets and the row's total; it also zeroes the words
//                          of the row buffer that two blocks share.
//   jpegenc_pack_kernel    one thread per block: codes the block again, this time into a 64-bit accumulator, and stores
//                          whole 32-bit words (byte-swapped: the stream is MSB first); the first and last word of a
//                          block, which it may share with its neighbours, are merged with atomicOr on the zeroed word.
//                          The row's last block appends the 1-bits that pad the segment.
//   jpegenc_stuff_kernel   one workgroup per MCU row: counts the 0xFF bytes of a run of bytes per thread, prefix sum,
//                          copies the run with a 0x00 behind every 0xFF; leaves the segment's length.
//   jpegenc_gather_kernel  one workgroup per MCU row: copies the segment, 16 bytes per lane, into page-locked memory
//                          behind the segments before it (each starts on a multiple of 16).
// Only compressed bytes cross to the host.  No address depends on a pixel's or a coefficient's value except through the
// bit lengths, and those are bounded per block by construction (FM_JPEGENC_BLOCK_BITS: the quantiser clamps AC values to
// 10 bits and DC values to 11, which 8-bit samples never exceed), so every row stays inside its part of the buffers.
#include "common.h"
#include "jpegenc.h"

namespace {

constexpr int BLK_STRIDE = 72;                // words of LDS per block (64 used): column reads of the six blocks spread over the banks
constexpr int MCU_WORDS = 6 * BLK_STRIDE;
constexpr int WG = 256;

__constant__ uint8_t ZIGZAG_DEV[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct EncGeo {
    int W, H;
    long long pitch;          // bytes between rows of the source
    int mx, my;               // MCU grid
    int real_bw, real_bh;     // luma blocks that hold image pixels: ceil(W / 8), ceil(H / 8)
    unsigned row_bytes;       // spacing of the rows in the unstuffed buffer (twice that in the stuffed one)
};

struct EncQt {
    uint16_t q[128];          // luminance, chrominance; row-major
};

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// One 1-D pass of the "islow" forward DCT, in place.  FIRST: the row pass (results keep two extra bits).
template <bool FIRST>
__device__ __forceinline__ void fdct_1d(int (&d)[8]) {
    const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int N = FIRST ? 11 : 15;
    d[0] = FIRST ? (tmp10 + tmp11) * 4 : descale(tmp10 + tmp11, 2);
    d[4] = FIRST ? (tmp10 - tmp11) * 4 : descale(tmp10 - tmp11, 2);
    int z1 = (tmp12 + tmp13) * 4433;
    d[2] = descale(z1 + tmp13 * 6270, N);
    d[6] = descale(z1 - tmp12 * 15137, N);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
    z1 *= -7373, z2 *= -20995;
    z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    d[7] = descale(t4 + z1 + z3, N);
    d[5] = descale(t5 + z2 + z4, N);
    d[3] = descale(t6 + z2 + z3, N);
    d[1] = descale(t7 + z1 + z4, N);
}

// sign(c) * ((|c| + div / 2) / div), div = 8 q; clamped to `lim` bits of magnitude (see the file header)
__device__ __forceinline__ int quantise(int c, int q, int lim) {
    const int div = q * 8;
    const int m = min((abs(c) + (div >> 1)) / div, lim);
    return c < 0 ? -m : m;
}

__global__ __launch_bounds__(WG) void jpegenc_fdct_kernel(const uint8_t* __restrict__ bgr, int16_t* __restrict__ coef, EncGeo g, EncQt qt) {
    __shared__ int ws[(WG / 64) * MCU_WORDS];
    __shared__ int chroma[(WG / 64) * 2 * 256];
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int mcu = blockIdx.x * (WG / 64) + wave;
    const bool active = mcu < g.mx * g.my;
    const int my = active ? mcu / g.mx : 0, mx = active ? mcu - my * g.mx : 0;
    int* const w = ws + wave * MCU_WORDS;
    int* const cbf = chroma + wave * 512;
    int* const crf = cbf + 256;

    if (active) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = i * 64 + l, py = p >> 4, px = p & 15;
            const int gx = min(mx * 16 + px, g.W - 1), gy = min(my * 16 + py, g.H - 1);      // edge replication
            const uint8_t* const s = bgr + (size_t)gy * g.pitch + (size_t)gx * 3;
            int B = s[0], G = s[1], R = s[2];
            const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
            w[((py >> 3) * 2 + (px >> 3)) * BLK_STRIDE + (py & 7) * 8 + (px & 7)] = Y - 128;
            // chroma rows below the image repeat the last AVERAGED row, i.e. the last PAIR of rows (libjpeg pads the
            // chroma plane after the averaging); with an even height that is not the last row twice
            const int gyc = min(min(my * 16 + py, ((g.H + 1) / 2 - 1) * 2 + (py & 1)), g.H - 1);
            if (gyc != gy) {
                const uint8_t* const sc = bgr + (size_t)gyc * g.pitch + (size_t)gx * 3;
                B = sc[0], G = sc[1], R = sc[2];
            }
            cbf[p] = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
            crf[p] = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
        }
    }
    __syncthreads();
    if (active) {                                       // chroma sample l of the MCU's 8 x 8
        const int at = (l >> 3) * 32 + (l & 7) * 2, bias = 1 + (l & 1);
        w[4 * BLK_STRIDE + l] = ((cbf[at] + cbf[at + 1] + cbf[at + 16] + cbf[at + 17] + bias) >> 2) - 128;
        w[5 * BLK_STRIDE + l] = ((crf[at] + crf[at + 1] + crf[at + 16] + crf[at + 17] + bias) >> 2) - 128;
    }
    __syncthreads();
    int* const blk = w + (l >> 3) * BLK_STRIDE;         // lanes 0..47: block l / 8, row / column l % 8
    const int j = l & 7;
    if (active && l < 48) {
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = blk[j * 8 + k];
        fdct_1d<true>(v);
#pragma unroll
        for (int k = 0; k < 8; ++k) blk[j * 8 + k] = v[k];
    }
    __syncthreads();
    if (active && l < 48) {
        int v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = blk[r * 8 + j];
        fdct_1d<false>(v);
#pragma unroll
        for (int r = 0; r < 8; ++r) blk[r * 8 + j] = v[r];
    }
    __syncthreads();
    if (!active) return;
    // dummy luma blocks take the quantised DC of the block before them
    int dc[4];
    bool dummy[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        dummy[b] = mx * 2 + (b & 1) >= g.real_bw || my * 2 + (b >> 1) >= g.real_bh;
        dc[b] = dummy[b] ? dc[b > 0 ? b - 1 : 0] : quantise(w[b * BLK_STRIDE], qt.q[0], 1024);
    }
    const int n = ZIGZAG_DEV[l];
    int16_t* const out = coef + (size_t)mcu * 384 + l;
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        int v = quantise(w[b * BLK_STRIDE + n], qt.q[(b < 4 ? 0 : 64) + n], l ? 1023 : 1024);
        if (b < 4 && dummy[b]) v = l ? 0 : dc[b];
        out[b * 64] = (int16_t)v;
    }
}

// Bits of one block through `sink.put(bits, count)`, count <= 27.  blk: 64 coefficients in zig-zag order; pred: the DC
// of the component's previous block in the row; dc / ac: the code look-ups of the block's table set (in LDS).
template <class Sink>
__device__ __forceinline__ void code_block(const int16_t* __restrict__ blk, int pred, const uint32_t* dc, const uint32_t* ac, Sink& sink) {
    uint32_t wv[32];                                     // the block in registers: every index below is a constant
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 q = reinterpret_cast<const uint4*>(blk)[i];
        wv[4 * i] = q.x, wv[4 * i + 1] = q.y, wv[4 * i + 2] = q.z, wv[4 * i + 3] = q.w;
    }
#define FM_COEF(k) ((int)(int16_t)(wv[(k) >> 1] >> (((k) & 1) * 16)))
    {
        const int diff = FM_COEF(0) - pred;
        const int mag = abs(diff), nbits = 32 - __clz(mag);             // (__clz(0) == 32)
        const uint32_t e = dc[min(nbits, 15)];
        sink.put(((e >> 5) << nbits) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nbits) - 1)), (int)(e & 31) + nbits);
    }
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int v = FM_COEF(k);
        if (v == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            sink.put(ac[0xF0] >> 5, (int)(ac[0xF0] & 31));
            run -= 16;
        }
        const int mag = abs(v), nbits = min(32 - __clz(mag), 10);
        const uint32_t e = ac[(run << 4) | nbits];
        sink.put(((e >> 5) << nbits) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nbits) - 1)), (int)(e & 31) + nbits);
        run = 0;
    }
    if (run) sink.put(ac[0] >> 5, (int)(ac[0] & 31));
#undef FM_COEF
}

// DC predictor of block b (coded order, six per MCU) of a row whose coefficients start at `row`
__device__ __forceinline__ int dc_pred(const int16_t* __restrict__ row, int b) {
    const int mcu = b / 6, j = b - mcu * 6;
    if (j >= 1 && j <= 3) return row[(size_t)(b - 1) * 64];
    if (mcu == 0) return 0;
    return row[(size_t)((mcu - 1) * 6 + (j ? j : 3)) * 64];
}

__device__ __forceinline__ void load_tables(const uint32_t* __restrict__ tables, uint32_t* tab) {
    for (int i = threadIdx.x; i < 2 * FM_JPEGENC_TABLE_WORDS; i += WG) tab[i] = tables[i];
    __syncthreads();
}

struct CountSink {
    unsigned bits = 0;
    __device__ __forceinline__ void put(uint32_t, int n) { bits += n; }
};

// Inclusive prefix sum of one value per thread over the workgroup; `buf`: WG words of LDS.
__device__ __forceinline__ unsigned wg_inclusive_scan(unsigned v, unsigned* buf) {
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < WG; d <<= 1) {
        const unsigned add = threadIdx.x >= (unsigned)d ? buf[threadIdx.x - d] : 0;
        __syncthreads();
        buf[threadIdx.x] += add;
        __syncthreads();
    }
    return buf[threadIdx.x];
}

__global__ __launch_bounds__(WG) void jpegenc_scan_kernel(const int16_t* __restrict__ coef, const uint32_t* __restrict__ tables,
                                                          uint32_t* __restrict__ bitoff, uint32_t* __restrict__ rowbits,
                                                          uint8_t* __restrict__ raw, EncGeo g) {
    __shared__ uint32_t tab[2 * FM_JPEGENC_TABLE_WORDS];
    __shared__ unsigned sums[WG];
    load_tables(tables, tab);
    const int row = blockIdx.x, nblk = 6 * g.mx, per = (nblk + WG - 1) / WG;
    const int b0 = min((int)threadIdx.x * per, nblk), b1 = min(b0 + per, nblk);
    const int16_t* const crow = coef + (size_t)row * nblk * 64;
    uint32_t* const off = bitoff + (size_t)row * nblk;
    uint32_t* const words = reinterpret_cast<uint32_t*>(raw + (size_t)row * g.row_bytes);
    unsigned sum = 0;
    for (int b = b0; b < b1; ++b) {
        const uint32_t* const t = tab + (b % 6 >= 4 ? FM_JPEGENC_TABLE_WORDS : 0);
        CountSink s;
        code_block(crow + (size_t)b * 64, dc_pred(crow, b), t, t + 16, s);
        off[b] = s.bits;
        sum += s.bits;
    }
    const unsigned incl = wg_inclusive_scan(sum, sums);
    unsigned at = incl - sum;
    for (int b = b0; b < b1; ++b) {
        const unsigned len = off[b];
        off[b] = at;
        words[at >> 5] = 0;             // the word a block starts in may hold the end of the block before it
        at += len;
    }
    if (threadIdx.x == WG - 1) {
        rowbits[row] = incl;
        words[incl >> 5] = 0;           // ... and the word the row's last block ends in
    }
}

// Appends bits at a bit offset of the row buffer: whole words are stored, the first and the last word of a block --
// which the neighbouring blocks also write -- are merged into the zeroed word.
struct PackSink {
    uint32_t* words;
    uint64_t acc = 0;
    int nacc;
    bool shared_first;
    __device__ __forceinline__ PackSink(uint32_t* row_words, unsigned bit) : words(row_words + (bit >> 5)), nacc(bit & 31), shared_first(bit & 31) {}
    __device__ __forceinline__ void put(uint32_t v, int n) {
        acc = (acc << n) | v;
        nacc += n;
        if (nacc >= 32) {
            const uint32_t wv = __builtin_bswap32((uint32_t)(acc >> (nacc - 32)));
            if (shared_first)
                atomicOr(words, wv);
            else
                *words = wv;
            shared_first = false;
            ++words;
            nacc -= 32;
        }
    }
    __device__ __forceinline__ void finish() {
        if (nacc) atomicOr(words, __builtin_bswap32((uint32_t)(acc << (32 - nacc))));
    }
};

__global__ __launch_bounds__(WG) void jpegenc_pack_kernel(const int16_t* __restrict__ coef, const uint32_t* __restrict__ tables,
                                                          const uint32_t* __restrict__ bitoff, const uint32_t* __restrict__ rowbits,
                                                          uint8_t* __restrict__ raw, EncGeo g) {
    __shared__ uint32_t tab[2 * FM_JPEGENC_TABLE_WORDS];
    load_tables(tables, tab);
    const int nblk = 6 * g.mx;
    const long long id = (long long)blockIdx.x * WG + threadIdx.x;
    if (id >= (long long)nblk * g.my) return;
    const int row = (int)(id / nblk), b = (int)(id - (long long)row * nblk);
    const int16_t* const crow = coef + (size_t)row * nblk * 64;
    const uint32_t* const t = tab + (b % 6 >= 4 ? FM_JPEGENC_TABLE_WORDS : 0);
    PackSink s(reinterpret_cast<uint32_t*>(raw + (size_t)row * g.row_bytes), bitoff[id]);
    code_block(crow + (size_t)b * 64, dc_pred(crow, b), t, t + 16, s);
    if (b == nblk - 1) {
        const int pad = (int)(-rowbits[row] & 7u);
        s.put((1u << pad) - 1, pad);
    }
    s.finish();
}

__global__ __launch_bounds__(WG) void jpegenc_stuff_kernel(const uint8_t* __restrict__ raw, const uint32_t* __restrict__ rowbits,
                                                           uint8_t* __restrict__ stuffed, uint32_t* __restrict__ seg_len,
                                                           uint32_t* __restrict__ seg_len_host, EncGeo g) {
    __shared__ unsigned sums[WG];
    const int row = blockIdx.x;
    const unsigned nbytes = (rowbits[row] + 7) >> 3, per = (nbytes + WG - 1) / WG;
    const unsigned i0 = min(threadIdx.x * per, nbytes), i1 = min(i0 + per, nbytes);
    const uint8_t* const src = raw + (size_t)row * g.row_bytes;
    uint8_t* const dst = stuffed + (size_t)row * g.row_bytes * 2;
    unsigned ff = 0;
    for (unsigned i = i0; i < i1; ++i) ff += src[i] == 0xFF;
    const unsigned incl = wg_inclusive_scan(ff, sums);
    unsigned o = i0 + incl - ff;
    for (unsigned i = i0; i < i1; ++i) {
        const uint8_t v = src[i];
        dst[o++] = v;
        if (v == 0xFF) dst[o++] = 0;
    }
    if (threadIdx.x == WG - 1) seg_len[row] = seg_len_host[row] = nbytes + incl;
}

__global__ __launch_bounds__(WG) void jpegenc_gather_kernel(const uint8_t* __restrict__ stuffed, const uint32_t* __restrict__ seg_len,
                                                            uint8_t* __restrict__ segs_host, EncGeo g) {
    __shared__ unsigned long long part[WG];
    const int row = blockIdx.x;
    unsigned long long before = 0;
    for (int r = threadIdx.x; r < row; r += WG) before += (seg_len[r] + 15u) & ~15u;
    part[threadIdx.x] = before;
    __syncthreads();
    for (int d = WG / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
        __syncthreads();
    }
    const uint4* const src = reinterpret_cast<const uint4*>(stuffed + (size_t)row * g.row_bytes * 2);
    uint4* const dst = reinterpret_cast<uint4*>(segs_host + part[0]);
    const unsigned n16 = (seg_len[row] + 15u) >> 4;
    for (unsigned i = threadIdx.x; i < n16; i += WG) dst[i] = src[i];
}

}  // namespace

struct EncState {
    hipStream_t s = nullptr;
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;
    bool timed = false;
    uint32_t* tables = nullptr;
    int cap_mx = 0, cap_my = 0;           // what the buffers below were sized for
    int16_t* coef = nullptr;
    uint32_t *bitoff = nullptr, *rowbits = nullptr, *seg_len = nullptr;
    uint8_t *raw = nullptr, *stuffed = nullptr;
    uint32_t* seg_len_host = nullptr;     // page-locked
    uint8_t* segs_host = nullptr;         // page-locked
    size_t segs_bytes = 0;
    uint8_t* stage = nullptr;             // fm_jpeg_encode_bgr: the pixels on the device ...
    uint8_t* stage_host = nullptr;        // ... and page-locked on the host
    size_t stage_cap = 0;
};

namespace {

void free_buffers(EncState* e) {
    for (void* p : {(void*)e->coef, (void*)e->bitoff, (void*)e->rowbits, (void*)e->seg_len, (void*)e->raw, (void*)e->stuffed})
        if (p) (void)hipFree(p);
    for (void* p : {(void*)e->seg_len_host, (void*)e->segs_host})
        if (p) (void)hipHostFree(p);
    e->coef = nullptr, e->bitoff = e->rowbits = e->seg_len = e->seg_len_host = nullptr, e->raw = e->stuffed = e->segs_host = nullptr;
    e->cap_mx = e->cap_my = 0;
    e->segs_bytes = 0;
}

int ensure(fm_ctx* ctx, int mx, int my) {
    if (!ctx->enc) {                    // published only once everything in it exists
        EncState* e = new EncState;
        uint32_t host[2 * FM_JPEGENC_TABLE_WORDS];
        fm_jpegenc_code_tables(host);
        hipError_t err = hipStreamCreateWithFlags(&e->s, hipStreamNonBlocking);
        if (err == hipSuccess) err = hipEventCreate(&e->ev_t0);
        if (err == hipSuccess) err = hipEventCreate(&e->ev_t1);
        if (err == hipSuccess) err = hipMalloc(&e->tables, sizeof host);
        if (err == hipSuccess) err = hipMemcpy(e->tables, host, sizeof host, hipMemcpyHostToDevice);
        if (err != hipSuccess) {
            if (e->tables) (void)hipFree(e->tables);
            if (e->ev_t0) (void)hipEventDestroy(e->ev_t0);
            if (e->ev_t1) (void)hipEventDestroy(e->ev_t1);
            if (e->s) (void)hipStreamDestroy(e->s);
            delete e;
            fm_set_error("JPEG encode: setting up the encoder failed -> %s", hipGetErrorString(err));
            return FM_ERR_HIP;
        }
        ctx->enc = e;
    }
    EncState* e = ctx->enc;
    if (mx <= e->cap_mx && my <= e->cap_my) return 0;
    FM_HIP(hipStreamSynchronize(e->s));
    const int cx = mx > e->cap_mx ? mx : e->cap_mx, cy = my > e->cap_my ? my : e->cap_my;
    free_buffers(e);
    const size_t nblk = (size_t)6 * cx * cy, row_bytes = fm_jpegenc_row_bytes(cx);
    FM_HIP(hipMalloc(&e->coef, nblk * 64 * sizeof(int16_t)));
    FM_HIP(hipMalloc(&e->bitoff, nblk * sizeof(uint32_t)));
    FM_HIP(hipMalloc(&e->rowbits, (size_t)cy * sizeof(uint32_t)));
    FM_HIP(hipMalloc(&e->seg_len, (size_t)cy * sizeof(uint32_t)));
    FM_HIP(hipMalloc(&e->raw, row_bytes * cy));
    FM_HIP(hipMalloc(&e->stuffed, 2 * row_bytes * cy));
    FM_HIP(hipHostMalloc(&e->seg_len_host, (size_t)cy * sizeof(uint32_t), hipHostMallocDefault));
    FM_HIP(hipHostMalloc(&e->segs_host, 2 * row_bytes * cy, hipHostMallocDefault));
    e->segs_bytes = 2 * row_bytes * cy;
    e->cap_mx = cx, e->cap_my = cy;
    return 0;
}

// Encodes the width x height BGR frame at `src` (device memory, `pitch` bytes between rows), which work already enqueued
// on the encoder's stream completes, and returns once the file is in `out`.
int encode(fm_ctx* ctx, const uint8_t* src, int width, int height, long long pitch, int quality, uint8_t* out, size_t capacity, size_t* length) {
    EncState* e = ctx->enc;
    EncGeo g;
    g.W = width, g.H = height, g.pitch = pitch;
    g.mx = (width + 15) / 16, g.my = (height + 15) / 16;
    g.real_bw = (width + 7) / 8, g.real_bh = (height + 7) / 8;
    g.row_bytes = (unsigned)fm_jpegenc_row_bytes(e->cap_mx);       // (rows as wide as the buffers were sized for)
    EncQt qt;
    if (int rc = fm_jpeg_encode_tables(quality, qt.q)) return rc;
    const long long n_mcu = (long long)g.mx * g.my, nblk = 6 * n_mcu;
    hipStream_t s = e->s;
    FM_HIP(hipEventRecord(e->ev_t0, s));
    hipLaunchKernelGGL(jpegenc_fdct_kernel, dim3((unsigned)((n_mcu + WG / 64 - 1) / (WG / 64))), dim3(WG), 0, s, src, e->coef, g, qt);
    FM_HIP(hipGetLastError());
    hipLaunchKernelGGL(jpegenc_scan_kernel, dim3(g.my), dim3(WG), 0, s, e->coef, e->tables, e->bitoff, e->rowbits, e->raw, g);
    FM_HIP(hipGetLastError());
    hipLaunchKernelGGL(jpegenc_pack_kernel, dim3((unsigned)((nblk + WG - 1) / WG)), dim3(WG), 0, s, e->coef, e->tables, e->bitoff, e->rowbits,
                       e->raw, g);
    FM_HIP(hipGetLastError());
    hipLaunchKernelGGL(jpegenc_stuff_kernel, dim3(g.my), dim3(WG), 0, s, e->raw, e->rowbits, e->stuffed, e->seg_len, e->seg_len_host, g);
    FM_HIP(hipGetLastError());
    hipLaunchKernelGGL(jpegenc_gather_kernel, dim3(g.my), dim3(WG), 0, s, e->stuffed, e->seg_len, e->segs_host, g);
    FM_HIP(hipGetLastError());
    FM_HIP(hipEventRecord(e->ev_t1, s));
    FM_HIP(hipStreamSynchronize(s));
    e->timed = true;
    return fm_jpeg_encode_assemble(width, height, quality, e->seg_len_host, e->segs_host, e->segs_bytes, out, capacity, length);
}

bool args_ok(int width, int height, int quality) {
    return quality >= 1 && quality <= 100 && width >= 1 && height >= 1 && width <= FM_SRC_MAX_DIM && height <= FM_SRC_MAX_DIM;
}

}  // namespace

void fm_jpegenc_free(fm_ctx* ctx) {
    EncState* e = ctx->enc;
    if (!e) return;
    if (e->s) (void)hipStreamSynchronize(e->s);
    free_buffers(e);
    if (e->tables) (void)hipFree(e->tables);
    if (e->stage) (void)hipFree(e->stage);
    if (e->stage_host) (void)hipHostFree(e->stage_host);
    if (e->ev_t0) (void)hipEventDestroy(e->ev_t0);
    if (e->ev_t1) (void)hipEventDestroy(e->ev_t1);
    if (e->s) (void)hipStreamDestroy(e->s);
    delete e;
    ctx->enc = nullptr;
}

// For overlay.hip, which renders on the encoder's stream and encodes its own buffer
int fm_jpegenc_ensure(fm_ctx* ctx, int mcus_x, int mcus_y) { return ensure(ctx, mcus_x, mcus_y); }
hipStream_t fm_jpegenc_stream(fm_ctx* ctx) { return ctx->enc ? ctx->enc->s : nullptr; }
int fm_jpegenc_encode_device(fm_ctx* ctx, const uint8_t* src, int width, int height, int quality, uint8_t* out, size_t capacity, size_t* length) {
    FM_CHECK_ARG(args_ok(width, height, quality));
    if (int rc = ensure(ctx, (width + 15) / 16, (height + 15) / 16)) return rc;
    return encode(ctx, src, width, height, (long long)width * 3, quality, out, capacity, length);
}

extern "C" int fm_frame_encode_jpeg(fm_ctx* ctx, int quality, uint8_t* out, size_t capacity, size_t* length) {
    FM_CHECK_ARG(ctx && out && length && ctx->frame_cur && args_ok(ctx->frame_w, ctx->frame_h, quality));
    if (int rc = ensure(ctx, (ctx->frame_w + 15) / 16, (ctx->frame_h + 15) / 16)) return rc;
    // No event of the pipeline is waited for: the current frame is complete on the device, as the host sees it, when
    // the call that made it current returned.  fm_frame_upload and its _nv12 / _jpeg / _src forms synchronise the stream
    // of their copy, conversion and resize; a ring frame was stored synchronously; fm_frame_promote_next synchronises
    // the stream that carries every look-ahead upload before it makes the slot's frame current.  The encoder's stream
    // is joined to the caller by the synchronise in encode(), before which no next frame can be uploaded over this one.
    return encode(ctx, ctx->frame_cur, ctx->frame_w, ctx->frame_h, (long long)ctx->frame_w * 3, quality, out, capacity, length);
}

extern "C" int fm_jpeg_encode_bgr(fm_ctx* ctx, const uint8_t* pixels, int width, int height, size_t pitch, int quality, uint8_t* out,
                                  size_t capacity, size_t* length) {
    FM_CHECK_ARG(ctx && pixels && out && length && args_ok(width, height, quality) && pitch >= (size_t)width * 3);
    if (int rc = ensure(ctx, (width + 15) / 16, (height + 15) / 16)) return rc;
    EncState* e = ctx->enc;
    const size_t row = (size_t)width * 3, bytes = row * height;
    if (bytes > e->stage_cap) {
        if (e->stage) (void)hipFree(e->stage);
        if (e->stage_host) (void)hipHostFree(e->stage_host);
        e->stage = e->stage_host = nullptr;
        e->stage_cap = 0;
        FM_HIP(hipMalloc(&e->stage, bytes));
        FM_HIP(hipHostMalloc(&e->stage_host, bytes, hipHostMallocDefault));
        e->stage_cap = bytes;
    }
    const uint8_t* from = pixels;
    if (pitch != row || !fm_host_is_pinned(pixels, bytes)) {      // (the previous call's copy out of stage_host is complete: it returned)
        if (pitch == row)
            memcpy(e->stage_host, pixels, bytes);
        else
            for (int r = 0; r < height; ++r) memcpy(e->stage_host + (size_t)r * row, pixels + (size_t)r * pitch, row);
        from = e->stage_host;
    }
    FM_HIP(hipMemcpyAsync(e->stage, from, bytes, hipMemcpyHostToDevice, e->s));
    return encode(ctx, e->stage, width, height, (long long)row, quality, out, capacity, length);
}

extern "C" int fm_jpeg_encode_stream_ms(fm_ctx* ctx, float* ms) {
    FM_CHECK_ARG(ctx && ms);
    *ms = -1.f;
    if (ctx->enc && ctx->enc->timed) FM_HIP(hipEventElapsedTime(ms, ctx->enc->ev_t0, ctx->enc->ev_t1));
    return 0;
}
