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
// ONE set of kernels serves the whole frame and the object crops of fm_frame_encode_regions (many images of different
// sizes in one pass).  Each kernel is a template over a MAP that says where an index of its launch lies: FrameMap, one
// image found by index arithmetic (no table, no upload: the code the whole-frame path always had), and TableMap, the
// concatenation of all images' MCUs, blocks and MCU rows behind a per-row and a per-image table that
// fm_jpeg_encode_regions_plan lays out on the host.  Everything per MCU, per block and per byte is the same text.
//
// Five launches on the encoder's own stream (TableMap: a sixth, tiny one, jpegenc_segoff_kernel, in front of the gather):
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

const uint8_t* fm_overlay_buffer(fm_ctx* ctx);            // overlay.hip: the overlay picture of the current frame size, or null

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
    unsigned row_bytes;       // spacing of the rows in the unstuffed buffer (twice that in the stuffed one)
};

// Per-image and per-MCU-row tables of a call with many images (TableMap).  Rows are the unit everything but the DCT works
// on, so a row carries what those kernels need and they never touch the image table.
struct EncImg {
    int32_t x0, y0;           // the crop's corner in the source picture
    int32_t cw, ch;           // the crop's size in source pixels
    int32_t W, H;             // the file's size: ceil(cw / shrink), ceil(ch / shrink)
    int32_t mx;               // MCUs across
    int32_t row0;             // its first row in the call
};
struct EncRow {
    int32_t first_mcu;        // of the row in the call's MCU index space (strictly increasing: every row has an MCU)
    int32_t img;
    int32_t mx;               // MCUs of the row = of its image
    uint32_t raw_off;         // of the row in the unstuffed buffer, bytes, a multiple of 16 (twice that in the stuffed one)
};

struct McuAt {                // what the DCT kernel needs to know about one MCU
    const uint8_t* org;       // the image's first pixel in the source
    int W, H;                 // the image's size (after `shrink`): edge replication, the chroma rule and the dummy blocks
    int cw, ch;               // are all per IMAGE -- nothing here is the frame's
    int mx, my;               // the MCU's place in its image
};
struct RowAt {                // ... and the other kernels about one MCU row
    int nblk;                 // blocks of the row, 6 per MCU
    size_t blk0;              // its first block in the call's block index space (coefficients, bit offsets)
    size_t raw_off;
};

struct FrameMap {
    static constexpr bool TABLE = false;
    const uint8_t* src;
    EncGeo g;
    __device__ __forceinline__ long long pitch() const { return g.pitch; }
    __device__ __forceinline__ int shrink() const { return 1; }
    __device__ __forceinline__ int n_mcu() const { return g.mx * g.my; }
    __device__ __forceinline__ long long n_blk() const { return (long long)6 * g.mx * g.my; }
    __device__ __forceinline__ McuAt mcu_at(int mcu) const {
        const int my = mcu / g.mx;
        return {src, g.W, g.H, g.W, g.H, mcu - my * g.mx, my};
    }
    __device__ __forceinline__ RowAt row_at(int row) const { return {6 * g.mx, (size_t)row * (6 * g.mx), (size_t)row * g.row_bytes}; }
    __device__ __forceinline__ int row_of_block(long long id) const { return (int)(id / (6 * g.mx)); }
};

struct TableMap {
    static constexpr bool TABLE = true;
    const uint8_t* src;
    long long src_pitch;
    const EncImg* imgs;
    const EncRow* rows;
    int n_rows, n_mcus, s;
    __device__ __forceinline__ long long pitch() const { return src_pitch; }
    __device__ __forceinline__ int shrink() const { return s; }
    __device__ __forceinline__ int n_mcu() const { return n_mcus; }
    __device__ __forceinline__ long long n_blk() const { return (long long)6 * n_mcus; }
    // the last row that starts at or before `mcu` (mcu < n_mcus): the table is sorted, a dozen steps for thousands of rows
    __device__ __forceinline__ int row_of_mcu(int mcu) const {
        int lo = 0, hi = n_rows - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (rows[mid].first_mcu <= mcu)
                lo = mid;
            else
                hi = mid - 1;
        }
        return lo;
    }
    __device__ __forceinline__ McuAt mcu_at(int mcu) const {
        const int row = row_of_mcu(mcu);
        const EncRow r = rows[row];
        const EncImg im = imgs[r.img];
        // x0 * 3 is an arbitrary byte offset: the pixels are fetched byte by byte, nothing assumes an alignment
        return {src + (size_t)im.y0 * src_pitch + (size_t)im.x0 * 3, im.W, im.H, im.cw, im.ch, mcu - r.first_mcu, row - im.row0};
    }
    __device__ __forceinline__ RowAt row_at(int row) const {
        const EncRow r = rows[row];
        return {6 * r.mx, (size_t)6 * r.first_mcu, (size_t)r.raw_off};
    }
    __device__ __forceinline__ int row_of_block(long long id) const { return row_of_mcu((int)(id / 6)); }
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

// Pixel (X, Y) of an image as the DCT sees it.  shrink 1: the source pixel.  shrink s: the rounded mean (sum + n / 2) / n
// per channel over the crop pixels [sX, sX + s) x [sY, sY + s) that lie inside the CROP (cw x ch) -- blocks at its right
// and lower edge average fewer pixels, never the frame's beyond it.  No reduced picture is stored.
template <class Map>
__device__ __forceinline__ void fetch_bgr(const Map& m, const McuAt& a, int X, int Y, int& B, int& G, int& R) {
    const int s = m.shrink();
    if (!Map::TABLE || s == 1) {
        const uint8_t* const p = a.org + (size_t)Y * m.pitch() + (size_t)X * 3;
        B = p[0], G = p[1], R = p[2];
        return;
    }
    const int x0 = X * s, x1 = min(x0 + s, a.cw), y0 = Y * s, y1 = min(y0 + s, a.ch);
    int sb = 0, sg = 0, sr = 0;
    for (int y = y0; y < y1; ++y) {
        const uint8_t* p = a.org + (size_t)y * m.pitch() + (size_t)x0 * 3;
        for (int x = x0; x < x1; ++x, p += 3) sb += p[0], sg += p[1], sr += p[2];
    }
    const int n = (x1 - x0) * (y1 - y0);
    B = (sb + n / 2) / n, G = (sg + n / 2) / n, R = (sr + n / 2) / n;
}

template <class Map>
__global__ __launch_bounds__(WG) void jpegenc_fdct_kernel(Map m, int16_t* __restrict__ coef, EncQt qt) {
    __shared__ int ws[(WG / 64) * MCU_WORDS];
    __shared__ int chroma[(WG / 64) * 2 * 256];
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int mcu = blockIdx.x * (WG / 64) + wave;
    const bool active = mcu < m.n_mcu();
    const McuAt a = m.mcu_at(active ? mcu : 0);
    const int my = a.my, mx = a.mx;
    int* const w = ws + wave * MCU_WORDS;
    int* const cbf = chroma + wave * 512;
    int* const crf = cbf + 256;

    if (active) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = i * 64 + l, py = p >> 4, px = p & 15;
            // edge replication to the MCU grid: the IMAGE's last column / row (a crop's, not its neighbours in the frame)
            const int gx = min(mx * 16 + px, a.W - 1), gy = min(my * 16 + py, a.H - 1);
            int B, G, R;
            fetch_bgr(m, a, gx, gy, B, G, R);
            const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
            w[((py >> 3) * 2 + (px >> 3)) * BLK_STRIDE + (py & 7) * 8 + (px & 7)] = Y - 128;
            // chroma rows below the image repeat the last AVERAGED row, i.e. the last PAIR of rows (libjpeg pads the
            // chroma plane after the averaging); with an even height that is not the last row twice.  The image's own H.
            const int gyc = min(min(my * 16 + py, ((a.H + 1) / 2 - 1) * 2 + (py & 1)), a.H - 1);
            if (gyc != gy) fetch_bgr(m, a, gx, gyc, B, G, R);
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
    // dummy luma blocks take the quantised DC of the block before them; which blocks hold pixels is the image's matter
    const int real_bw = (a.W + 7) / 8, real_bh = (a.H + 7) / 8;
    int dc[4];
    bool dummy[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        dummy[b] = mx * 2 + (b & 1) >= real_bw || my * 2 + (b >> 1) >= real_bh;
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

template <class Map>
__global__ __launch_bounds__(WG) void jpegenc_scan_kernel(const int16_t* __restrict__ coef, const uint32_t* __restrict__ tables,
                                                          uint32_t* __restrict__ bitoff, uint32_t* __restrict__ rowbits,
                                                          uint8_t* __restrict__ raw, Map m) {
    __shared__ uint32_t tab[2 * FM_JPEGENC_TABLE_WORDS];
    __shared__ unsigned sums[WG];
    load_tables(tables, tab);
    // A row is an MCU row of ONE image, so the DC predictors (dc_pred: zero at the row's first MCU) restart at every row
    // of every image.  A row wider than 42 MCUs has more blocks than threads (per > 1), a 1-MCU image six blocks: the
    // other threads carry a sum of zero through the scan.
    const RowAt ra = m.row_at(blockIdx.x);
    const int row = blockIdx.x, nblk = ra.nblk, per = (nblk + WG - 1) / WG;
    const int b0 = min((int)threadIdx.x * per, nblk), b1 = min(b0 + per, nblk);
    const int16_t* const crow = coef + ra.blk0 * 64;
    uint32_t* const off = bitoff + ra.blk0;
    uint32_t* const words = reinterpret_cast<uint32_t*>(raw + ra.raw_off);
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

template <class Map>
__global__ __launch_bounds__(WG) void jpegenc_pack_kernel(const int16_t* __restrict__ coef, const uint32_t* __restrict__ tables,
                                                          const uint32_t* __restrict__ bitoff, const uint32_t* __restrict__ rowbits,
                                                          uint8_t* __restrict__ raw, Map m) {
    __shared__ uint32_t tab[2 * FM_JPEGENC_TABLE_WORDS];
    load_tables(tables, tab);
    const long long id = (long long)blockIdx.x * WG + threadIdx.x;
    if (id >= m.n_blk()) return;
    // The atomicOr merges below stay inside the row's own buffer: rows never share a word, each starts on a 16-byte
    // boundary of its own and is sized for its own width (fm_jpeg_encode_regions_plan), whichever image a neighbour
    // thread's block belongs to.
    const int row = m.row_of_block(id);
    const RowAt ra = m.row_at(row);
    const int nblk = ra.nblk, b = (int)(id - (long long)ra.blk0);
    const int16_t* const crow = coef + ra.blk0 * 64;
    const uint32_t* const t = tab + (b % 6 >= 4 ? FM_JPEGENC_TABLE_WORDS : 0);
    PackSink s(reinterpret_cast<uint32_t*>(raw + ra.raw_off), bitoff[id]);
    code_block(crow + (size_t)b * 64, dc_pred(crow, b), t, t + 16, s);
    if (b == nblk - 1) {
        const int pad = (int)(-rowbits[row] & 7u);
        s.put((1u << pad) - 1, pad);
    }
    s.finish();
}

template <class Map>
__global__ __launch_bounds__(WG) void jpegenc_stuff_kernel(const uint8_t* __restrict__ raw, const uint32_t* __restrict__ rowbits,
                                                           uint8_t* __restrict__ stuffed, uint32_t* __restrict__ seg_len,
                                                           uint32_t* __restrict__ seg_len_host, Map m) {
    __shared__ unsigned sums[WG];
    const int row = blockIdx.x;
    const unsigned nbytes = (rowbits[row] + 7) >> 3, per = (nbytes + WG - 1) / WG;
    const unsigned i0 = min(threadIdx.x * per, nbytes), i1 = min(i0 + per, nbytes);
    const size_t raw_off = m.row_at(row).raw_off;
    const uint8_t* const src = raw + raw_off;
    uint8_t* const dst = stuffed + raw_off * 2;
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

// Where every segment starts in page-locked memory: the exclusive prefix sum of the lengths, each rounded up to 16.  One
// workgroup, once per call with many images, so that the thousands of rows of such a call need not each sum the
// lengths of all rows before them as the rows of one frame do in jpegenc_gather_kernel.
__global__ __launch_bounds__(WG) void jpegenc_segoff_kernel(const uint32_t* __restrict__ seg_len, uint32_t* __restrict__ seg_off, int n_rows) {
    __shared__ unsigned sums[WG];
    const int per = (n_rows + WG - 1) / WG;
    const int r0 = min((int)threadIdx.x * per, n_rows), r1 = min(r0 + per, n_rows);
    unsigned sum = 0;
    for (int r = r0; r < r1; ++r) sum += (seg_len[r] + 15u) & ~15u;
    unsigned at = wg_inclusive_scan(sum, sums) - sum;
    for (int r = r0; r < r1; ++r) {
        seg_off[r] = at;
        at += (seg_len[r] + 15u) & ~15u;
    }
}

template <class Map>
__global__ __launch_bounds__(WG) void jpegenc_gather_kernel(const uint8_t* __restrict__ stuffed, const uint32_t* __restrict__ seg_len,
                                                            const uint32_t* __restrict__ seg_off, uint8_t* __restrict__ segs_host, Map m) {
    __shared__ unsigned long long part[WG];
    const int row = blockIdx.x;
    if (Map::TABLE) {
        if (threadIdx.x == 0) part[0] = seg_off[row];
        __syncthreads();
    } else {
        unsigned long long before = 0;
        for (int r = threadIdx.x; r < row; r += WG) before += (seg_len[r] + 15u) & ~15u;
        part[threadIdx.x] = before;
        __syncthreads();
        for (int d = WG / 2; d > 0; d >>= 1) {
            if ((int)threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
            __syncthreads();
        }
    }
    const uint4* const src = reinterpret_cast<const uint4*>(stuffed + m.row_at(row).raw_off * 2);
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
    // what the buffers below were sized for: MCUs (coefficients, bit offsets), MCU rows (lengths), bytes of unstuffed rows
    size_t cap_mcus = 0, cap_rows = 0, cap_raw = 0;
    int16_t* coef = nullptr;
    uint32_t *bitoff = nullptr, *rowbits = nullptr, *seg_len = nullptr, *seg_off = nullptr;
    uint8_t *raw = nullptr, *stuffed = nullptr;
    uint32_t* seg_len_host = nullptr;     // page-locked
    uint8_t* segs_host = nullptr;         // page-locked
    size_t segs_bytes = 0;
    uint8_t* stage = nullptr;             // fm_jpeg_encode_bgr: the pixels on the device ...
    uint8_t* stage_host = nullptr;        // ... and page-locked on the host
    size_t stage_cap = 0;
    DevBuf tab;                           // fm_frame_encode_regions: the image and row tables, staged page-locked
    std::vector<fm_crop_plan> plans;
};

namespace {

void free_buffers(EncState* e) {
    for (void* p : {(void*)e->coef, (void*)e->bitoff, (void*)e->rowbits, (void*)e->seg_len, (void*)e->seg_off, (void*)e->raw, (void*)e->stuffed})
        if (p) (void)hipFree(p);
    for (void* p : {(void*)e->seg_len_host, (void*)e->segs_host})
        if (p) (void)hipHostFree(p);
    e->coef = nullptr, e->bitoff = e->rowbits = e->seg_len = e->seg_off = e->seg_len_host = nullptr, e->raw = e->stuffed = e->segs_host = nullptr;
    e->cap_mcus = e->cap_rows = e->cap_raw = 0;
    e->segs_bytes = 0;
}

// The encoder's stream and tables (first use), and working buffers for a call of `mcus` MCUs in `rows` MCU rows whose
// unstuffed row buffers take `raw_bytes` together (0, 0, 0: the stream alone).  Each of the three only ever grows.
int ensure(fm_ctx* ctx, size_t mcus, size_t rows, size_t raw_bytes) {
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
    if (mcus <= e->cap_mcus && rows <= e->cap_rows && raw_bytes <= e->cap_raw) return 0;
    FM_HIP(hipStreamSynchronize(e->s));
    const size_t cm = mcus > e->cap_mcus ? mcus : e->cap_mcus, cr = rows > e->cap_rows ? rows : e->cap_rows;
    const size_t cb = raw_bytes > e->cap_raw ? raw_bytes : e->cap_raw;
    free_buffers(e);
    const size_t nblk = 6 * cm;
    FM_HIP(hipMalloc(&e->coef, nblk * 64 * sizeof(int16_t)));
    FM_HIP(hipMalloc(&e->bitoff, nblk * sizeof(uint32_t)));
    FM_HIP(hipMalloc(&e->rowbits, cr * sizeof(uint32_t)));
    FM_HIP(hipMalloc(&e->seg_len, cr * sizeof(uint32_t)));
    FM_HIP(hipMalloc(&e->seg_off, cr * sizeof(uint32_t)));
    FM_HIP(hipMalloc(&e->raw, cb));
    FM_HIP(hipMalloc(&e->stuffed, 2 * cb));
    FM_HIP(hipHostMalloc(&e->seg_len_host, cr * sizeof(uint32_t), hipHostMallocDefault));
    FM_HIP(hipHostMalloc(&e->segs_host, 2 * cb, hipHostMallocDefault));
    e->segs_bytes = 2 * cb;
    e->cap_mcus = cm, e->cap_rows = cr, e->cap_raw = cb;
    return 0;
}

int ensure_frame(fm_ctx* ctx, int mx, int my) { return ensure(ctx, (size_t)mx * my, (size_t)my, fm_jpegenc_row_bytes(mx) * my); }

// The launches of one call over `m`, between the two timing events; `rows` MCU rows in all.
template <class Map>
int launch_all(EncState* e, const Map& m, long long n_mcu, int rows, const EncQt& qt) {
    const long long nblk = 6 * n_mcu;
    hipStream_t s = e->s;
    FM_HIP(hipEventRecord(e->ev_t0, s));
    hipLaunchKernelGGL(jpegenc_fdct_kernel<Map>, dim3((unsigned)((n_mcu + WG / 64 - 1) / (WG / 64))), dim3(WG), 0, s, m, e->coef, qt);
    FM_HIP(hipGetLastError());
    hipLaunchKernelGGL(jpegenc_scan_kernel<Map>, dim3(rows), dim3(WG), 0, s, e->coef, e->tables, e->bitoff, e->rowbits, e->raw, m);
    FM_HIP(hipGetLastError());
    hipLaunchKernelGGL(jpegenc_pack_kernel<Map>, dim3((unsigned)((nblk + WG - 1) / WG)), dim3(WG), 0, s, e->coef, e->tables, e->bitoff,
                       e->rowbits, e->raw, m);
    FM_HIP(hipGetLastError());
    hipLaunchKernelGGL(jpegenc_stuff_kernel<Map>, dim3(rows), dim3(WG), 0, s, e->raw, e->rowbits, e->stuffed, e->seg_len, e->seg_len_host, m);
    FM_HIP(hipGetLastError());
    if (Map::TABLE) {
        hipLaunchKernelGGL(jpegenc_segoff_kernel, dim3(1), dim3(WG), 0, s, e->seg_len, e->seg_off, rows);
        FM_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(jpegenc_gather_kernel<Map>, dim3(rows), dim3(WG), 0, s, e->stuffed, e->seg_len, e->seg_off, e->segs_host, m);
    FM_HIP(hipGetLastError());
    FM_HIP(hipEventRecord(e->ev_t1, s));
    FM_HIP(hipStreamSynchronize(s));
    e->timed = true;
    return 0;
}

// Encodes the width x height BGR frame at `src` (device memory, `pitch` bytes between rows), which work already enqueued
// on the encoder's stream completes, and returns once the file is in `out`.
int encode(fm_ctx* ctx, const uint8_t* src, int width, int height, long long pitch, int quality, uint8_t* out, size_t capacity, size_t* length) {
    EncState* e = ctx->enc;
    FrameMap m;
    m.src = src;
    EncGeo& g = m.g;
    g.W = width, g.H = height, g.pitch = pitch;
    g.mx = (width + 15) / 16, g.my = (height + 15) / 16;
    g.row_bytes = (unsigned)fm_jpegenc_row_bytes(g.mx);
    EncQt qt;
    if (int rc = fm_jpeg_encode_tables(quality, qt.q)) return rc;
    if (int rc = launch_all(e, m, (long long)g.mx * g.my, g.my, qt)) return rc;
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
    e->tab.release();
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
int fm_jpegenc_ensure(fm_ctx* ctx, int mcus_x, int mcus_y) { return ensure_frame(ctx, mcus_x, mcus_y); }
hipStream_t fm_jpegenc_stream(fm_ctx* ctx) { return ctx->enc ? ctx->enc->s : nullptr; }
int fm_jpegenc_encode_device(fm_ctx* ctx, const uint8_t* src, int width, int height, int quality, uint8_t* out, size_t capacity, size_t* length) {
    FM_CHECK_ARG(args_ok(width, height, quality));
    if (int rc = ensure_frame(ctx, (width + 15) / 16, (height + 15) / 16)) return rc;
    return encode(ctx, src, width, height, (long long)width * 3, quality, out, capacity, length);
}

extern "C" int fm_frame_encode_jpeg(fm_ctx* ctx, int quality, uint8_t* out, size_t capacity, size_t* length) {
    FM_CHECK_ARG(ctx && out && length && ctx->frame_cur && args_ok(ctx->frame_w, ctx->frame_h, quality));
    if (int rc = ensure_frame(ctx, (ctx->frame_w + 15) / 16, (ctx->frame_h + 15) / 16)) return rc;
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
    if (int rc = ensure_frame(ctx, (width + 15) / 16, (height + 15) / 16)) return rc;
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

extern "C" int fm_frame_encode_regions(fm_ctx* ctx, int which, const fm_crop_rect* rects, int n, int shrink, int quality, uint8_t* out,
                                       size_t capacity, size_t* offsets) {
    FM_CHECK_ARG(ctx && offsets && (which == FM_EXPORT_FRAME || which == FM_EXPORT_OVERLAY) && ctx->frame_cur &&
                 args_ok(ctx->frame_w, ctx->frame_h, 1));
    if (quality < 1 || quality > 100) {
        fm_set_error("object encode: quality %d outside 1..100", quality);
        return FM_ERR_ARG;
    }
    // Everything is refused here, before anything is enqueued: the list's own limits by the plan, then the frame's.
    fm_crop_totals tot;
    if (int rc = fm_jpeg_encode_regions_plan(rects, n, shrink, nullptr, &tot)) return rc;
    for (int i = 0; i < n; ++i)
        if (rects[i].x1 >= ctx->frame_w || rects[i].y1 >= ctx->frame_h) {
            fm_set_error("object encode: rectangle %d (%d, %d, %d, %d) reaches outside the %dx%d frame", i, rects[i].x0, rects[i].y0,
                         rects[i].x1, rects[i].y1, ctx->frame_w, ctx->frame_h);
            return FM_ERR_ARG;
        }
    const uint8_t* const src = which == FM_EXPORT_FRAME ? ctx->frame_cur : fm_overlay_buffer(ctx);
    if (!src) {
        fm_set_error("object encode: no overlay picture of the current frame size (fm_frame_render_overlay comes first)");
        return FM_ERR_ARG;
    }
    if (n == 0) {
        offsets[0] = 0;
        return 0;
    }
    FM_CHECK_ARG(out);
    if (capacity < tot.bound) {
        fm_set_error("object encode: capacity %zu is below the bound of the %d files, %llu bytes (fm_jpeg_encode_regions_bound)", capacity, n,
                     (unsigned long long)tot.bound);
        return FM_ERR_ARG;
    }
    if (int rc = ensure(ctx, (size_t)tot.mcus, (size_t)tot.rows, (size_t)tot.raw_bytes)) return rc;
    EncState* e = ctx->enc;
    e->plans.resize(n);
    if (int rc = fm_jpeg_encode_regions_plan(rects, n, shrink, e->plans.data(), &tot)) return rc;
    // The tables: n images, then the rows.  The staging is free to rewrite: the call that used it last returned behind
    // its synchronise (one that failed half way is waited for here).
    FM_HIP(hipStreamSynchronize(e->s));
    const size_t img_bytes = (((size_t)n * sizeof(EncImg)) + 15) & ~(size_t)15, all = img_bytes + (size_t)tot.rows * sizeof(EncRow);
    if (int rc = e->tab.reserve(all)) return rc;
    EncImg* const imgs = e->tab.host<EncImg>();
    EncRow* const rows = reinterpret_cast<EncRow*>(e->tab.host<char>() + img_bytes);
    for (int i = 0; i < n; ++i) {
        const fm_crop_plan& p = e->plans[i];
        imgs[i] = {rects[i].x0, rects[i].y0, rects[i].x1 - rects[i].x0 + 1, rects[i].y1 - rects[i].y0 + 1, p.width, p.height, p.mcus_x, p.first_row};
        const uint32_t row_bytes = (uint32_t)fm_jpegenc_row_bytes(p.mcus_x);
        for (int r = 0; r < p.mcus_y; ++r)
            rows[p.first_row + r] = {p.first_mcu + r * p.mcus_x, i, p.mcus_x, (uint32_t)p.raw_offset + (uint32_t)r * row_bytes};
    }
    FM_HIP(hipMemcpyAsync(e->tab.d, e->tab.h, all, hipMemcpyHostToDevice, e->s));
    TableMap m;
    m.src = src, m.src_pitch = (long long)ctx->frame_w * 3;
    m.imgs = e->tab.dev<EncImg>(), m.rows = reinterpret_cast<const EncRow*>(e->tab.dev<char>() + img_bytes);
    m.n_rows = tot.rows, m.n_mcus = tot.mcus, m.s = shrink;
    EncQt qt;
    if (int rc = fm_jpeg_encode_tables(quality, qt.q)) return rc;
    // fm_frame_encode_jpeg's argument for why the current frame is complete holds unchanged (no pipeline stream is waited
    // for, frames prefetched for later steps lie in other slots); the overlay buffer was rendered on this very stream.
    if (int rc = launch_all(e, m, tot.mcus, tot.rows, qt)) return rc;
    return fm_jpeg_encode_regions_assemble(e->plans.data(), n, quality, e->seg_len_host, e->segs_host, e->segs_bytes, out, capacity, offsets);
}

extern "C" int fm_jpeg_encode_stream_ms(fm_ctx* ctx, float* ms) {
    FM_CHECK_ARG(ctx && ms);
    *ms = -1.f;
    if (ctx->enc && ctx->enc->timed) FM_HIP(hipEventElapsedTime(ms, ctx->enc->ev_t0, ctx->enc->ev_t1));
    return 0;
}
