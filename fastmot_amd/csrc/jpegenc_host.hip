// Host half of the JPEG output path: everything of a baseline JPEG file that is not per-pixel or per-coefficient work
// -- the quality -> quantisation-table rule, the Annex-K Huffman tables (as DHT segments for the file and as code / size
// look-ups for the device), the marker segments in front of the scan, and the gathering of the scan's restart segments
// into the finished file.  The device half (jpegenc.hip) makes the segments: one byte-aligned, byte-stuffed piece of
// entropy-coded data per MCU row.
//
// No fm_ctx, no GPU, no state: every function here may be called from any number of threads at once
// (tests/test_jpegenc_host.py calls them without a device).
//
// Every write goes through `Writer`, which counts what it is asked to put and stores only what fits: a capacity that is
// too small gives FM_ERR_ARG after the fact, never a store past `out + capacity`.
#include "common.h"
#include "jpegenc.h"

namespace {

// Annex K.1 (luminance, chrominance), row-major
const uint8_t BASE_QT[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K.3: code counts per length 1..16, then the symbols in code order
const uint8_t DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr size_t HEADER_BYTES = 2 + 18 + 2 * 69 + 19 + 2 * 33 + 2 * 183 + 6 + 14;     // SOI .. SOS, as written below

struct Writer {
    uint8_t* out;
    size_t cap, n = 0;          // n: bytes asked for so far (the file's length once everything was put)
    void put(const void* p, size_t k) {
        if (n <= cap && k <= cap - n) memcpy(out + n, p, k);
        n += k;
    }
    void u8(unsigned v) {
        const uint8_t b = (uint8_t)v;
        put(&b, 1);
    }
    void u16(unsigned v) { u8(v >> 8), u8(v); }
    void marker(unsigned m) { u8(0xFF), u8(m); }
};

void tables(int quality, uint16_t* qt) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const long v = ((long)BASE_QT[t][i] * s + 50) / 100;
            qt[64 * t + i] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
}

void write_header(Writer& w, int width, int height, int quality) {
    uint16_t qt[128];
    tables(quality, qt);
    w.marker(0xD8);
    w.marker(0xE0), w.u16(16), w.put("JFIF", 5), w.u8(1), w.u8(1), w.u8(0), w.u16(1), w.u16(1), w.u8(0), w.u8(0);
    for (int t = 0; t < 2; ++t) {
        w.marker(0xDB), w.u16(67), w.u8(t);
        for (int k = 0; k < 64; ++k) w.u8(qt[64 * t + ZIGZAG[k]]);
    }
    w.marker(0xC0), w.u16(17), w.u8(8), w.u16(height), w.u16(width), w.u8(3);
    w.u8(1), w.u8(0x22), w.u8(0);
    w.u8(2), w.u8(0x11), w.u8(1);
    w.u8(3), w.u8(0x11), w.u8(1);
    for (int t = 0; t < 2; ++t) {           // DC then AC of table 0, DC then AC of table 1
        w.marker(0xC4), w.u16(2 + 1 + 16 + 12), w.u8(t), w.put(DC_BITS[t], 16), w.put(DC_VALS, 12);
        w.marker(0xC4), w.u16(2 + 1 + 16 + 162), w.u8(0x10 | t), w.put(AC_BITS[t], 16), w.put(AC_VALS[t], 162);
    }
    w.marker(0xDD), w.u16(4), w.u16((width + 15) / 16);
    w.marker(0xDA), w.u16(12), w.u8(3), w.u8(1), w.u8(0x00), w.u8(2), w.u8(0x11), w.u8(3), w.u8(0x11), w.u8(0), w.u8(63), w.u8(0);
}

bool size_ok(int width, int height) { return width >= 1 && height >= 1 && width <= FM_SRC_MAX_DIM && height <= FM_SRC_MAX_DIM; }

// (code << 5) | size for every symbol of a table; 0 where the table has no code
void code_table(const uint8_t* bits, const uint8_t* vals, uint32_t* out, int entries) {
    for (int i = 0; i < entries; ++i) out[i] = 0;
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) out[vals[k]] = (code << 5) | (uint32_t)l;
        code <<= 1;
    }
}

}  // namespace

void fm_jpegenc_code_tables(uint32_t* out) {
    for (int t = 0; t < 2; ++t) {
        code_table(DC_BITS[t], DC_VALS, out + t * FM_JPEGENC_TABLE_WORDS, 16);
        code_table(AC_BITS[t], AC_VALS[t], out + t * FM_JPEGENC_TABLE_WORDS + 16, 256);
    }
}

size_t fm_jpegenc_row_bytes(int mcus_x) { return (((size_t)mcus_x * FM_JPEGENC_MCU_BYTES + 1 + 15) & ~(size_t)15) + 16; }

extern "C" size_t fm_jpeg_encode_bound(int width, int height) {
    if (!size_ok(width, height)) return 0;
    const size_t mx = (width + 15) / 16, my = (height + 15) / 16;
    // per MCU row: the worst-case entropy-coded bytes, every one of them stuffed, and the RSTn marker / EOI behind it
    return HEADER_BYTES + my * (2 * (mx * FM_JPEGENC_MCU_BYTES + 1) + 2);
}

extern "C" int fm_jpeg_encode_tables(int quality, uint16_t* qt) {
    FM_CHECK_ARG(qt && quality >= 1 && quality <= 100);
    tables(quality, qt);
    return 0;
}

extern "C" int fm_jpeg_encode_header(int width, int height, int quality, uint8_t* out, size_t capacity, size_t* length) {
    FM_CHECK_ARG(out && length && quality >= 1 && quality <= 100 && size_ok(width, height));
    Writer w{out, capacity};
    write_header(w, width, height, quality);
    *length = w.n;
    if (w.n > capacity) {
        fm_set_error("JPEG encode: the header needs %zu bytes, the output holds %zu", w.n, capacity);
        return FM_ERR_ARG;
    }
    return 0;
}

extern "C" int fm_jpeg_encode_assemble(int width, int height, int quality, const uint32_t* seg_len, const uint8_t* segs, size_t segs_bytes,
                                       uint8_t* out, size_t capacity, size_t* length) {
    FM_CHECK_ARG(seg_len && segs && out && length && quality >= 1 && quality <= 100 && size_ok(width, height));
    const int rows = (height + 15) / 16;
    size_t at = 0;                          // the segments lie one behind the other, each at the next multiple of 16
    for (int r = 0; r < rows; ++r) {
        FM_CHECK_ARG(at <= segs_bytes && seg_len[r] <= segs_bytes - at);
        at += ((size_t)seg_len[r] + 15) & ~(size_t)15;
    }
    Writer w{out, capacity};
    write_header(w, width, height, quality);
    at = 0;
    for (int r = 0; r < rows; ++r) {
        if (r) w.marker(0xD0 + ((r - 1) & 7));
        w.put(segs + at, seg_len[r]);
        at += ((size_t)seg_len[r] + 15) & ~(size_t)15;
    }
    w.marker(0xD9);
    *length = w.n;
    if (w.n > capacity) {
        fm_set_error("JPEG encode: the file needs %zu bytes, the output holds %zu", w.n, capacity);
        return FM_ERR_ARG;
    }
    return 0;
}

// ---- object crops: many images in one pass of the encoder (fm_frame_encode_regions, jpegenc.hip)
extern "C" int fm_jpeg_encode_regions_plan(const fm_crop_rect* rects, int n, int shrink, fm_crop_plan* plans, fm_crop_totals* totals) {
    if (n < 0 || (n > 0 && !rects) || !totals) {
        fm_set_error("object encode: a null pointer or a negative count (n = %d)", n);
        return FM_ERR_ARG;
    }
    if (shrink != 1 && shrink != 2 && shrink != 4) {
        fm_set_error("object encode: shrink %d is not 1, 2 or 4", shrink);
        return FM_ERR_ARG;
    }
    if (n > FM_OBJENC_MAX_REGIONS) {
        fm_set_error("object encode: %d rectangles in one call, FM_OBJENC_MAX_REGIONS is %d", n, FM_OBJENC_MAX_REGIONS);
        return FM_ERR_ARG;
    }
    long long mcus = 0, rows = 0;
    uint64_t raw = 0, bound = 0;
    for (int i = 0; i < n; ++i) {
        const fm_crop_rect& r = rects[i];
        if (r.x0 < 0 || r.y0 < 0 || r.x1 < r.x0 || r.y1 < r.y0 || (long long)r.x1 - r.x0 >= FM_SRC_MAX_DIM ||
            (long long)r.y1 - r.y0 >= FM_SRC_MAX_DIM) {
            fm_set_error("object encode: rectangle %d (%d, %d, %d, %d) is empty, negative or wider / higher than %d", i, r.x0, r.y0, r.x1,
                         r.y1, FM_SRC_MAX_DIM);
            return FM_ERR_ARG;
        }
        const int w = (r.x1 - r.x0 + shrink) / shrink, h = (r.y1 - r.y0 + shrink) / shrink;      // ceil((x1 - x0 + 1) / shrink)
        const int mx = (w + 15) / 16, my = (h + 15) / 16;
        if (plans) {
            fm_crop_plan& p = plans[i];
            p.width = w, p.height = h, p.mcus_x = mx, p.mcus_y = my;
            p.first_mcu = (int32_t)mcus, p.first_block = (int32_t)(6 * mcus), p.first_row = (int32_t)rows, p.reserved = 0;
            p.raw_offset = raw, p.bound = fm_jpeg_encode_bound(w, h);
        }
        mcus += (long long)mx * my, rows += my;
        // every MCU row a buffer of its own, sized for ITS width and starting on a 16-byte boundary (fm_jpegenc_row_bytes
        // is a multiple of 16): the pack kernel's atomicOr on a row's first and last word never meets another image's
        raw += (uint64_t)fm_jpegenc_row_bytes(mx) * my;
        bound += fm_jpeg_encode_bound(w, h);
        if (mcus > FM_OBJENC_MAX_MCUS) {         // (checked inside the loop: the sums above stay far below 32 bits)
            fm_set_error("object encode: the rectangles up to number %d take %lld MCUs, FM_OBJENC_MAX_MCUS is %d", i, mcus,
                         FM_OBJENC_MAX_MCUS);
            return FM_ERR_ARG;
        }
    }
    totals->mcus = (int32_t)mcus, totals->blocks = (int32_t)(6 * mcus), totals->rows = (int32_t)rows, totals->reserved = 0;
    totals->raw_bytes = raw, totals->bound = bound;
    return 0;
}

extern "C" size_t fm_jpeg_encode_regions_bound(const fm_crop_rect* rects, int n, int shrink) {
    fm_crop_totals t;
    return fm_jpeg_encode_regions_plan(rects, n, shrink, nullptr, &t) ? 0 : (size_t)t.bound;
}

extern "C" int fm_jpeg_encode_regions_assemble(const fm_crop_plan* plans, int n, int quality, const uint32_t* seg_len, const uint8_t* segs,
                                               size_t segs_bytes, uint8_t* out, size_t capacity, size_t* offsets) {
    FM_CHECK_ARG(n >= 0 && offsets && (n == 0 || (plans && seg_len && segs && out)) && quality >= 1 && quality <= 100);
    // The lengths came from device memory: fm_jpeg_encode_assemble's check, over all rows of all images, before anything
    // is read.  The plans are checked with them -- rows numbered without gaps, sizes the header can state.
    size_t at = 0;
    int row = 0;
    for (int i = 0; i < n; ++i) {
        const fm_crop_plan& p = plans[i];
        FM_CHECK_ARG(size_ok(p.width, p.height) && p.first_row == row && p.mcus_y == (p.height + 15) / 16);
        for (int r = 0; r < p.mcus_y; ++r, ++row) {
            if (!(at <= segs_bytes && seg_len[row] <= segs_bytes - at)) {
                fm_set_error("object encode: the segment lengths do not fit the segment buffer (row %d of image %d: %u bytes at %zu of %zu)",
                             r, i, seg_len[row], at, segs_bytes);
                return FM_ERR_ARG;
            }
            at += ((size_t)seg_len[row] + 15) & ~(size_t)15;
        }
    }
    Writer w{out, capacity};
    at = 0, row = 0;
    for (int i = 0; i < n; ++i) {
        const fm_crop_plan& p = plans[i];
        offsets[i] = w.n;
        write_header(w, p.width, p.height, quality);
        for (int r = 0; r < p.mcus_y; ++r, ++row) {
            if (r) w.marker(0xD0 + ((r - 1) & 7));          // r counts inside the image: every file starts at RST0
            w.put(segs + at, seg_len[row]);
            at += ((size_t)seg_len[row] + 15) & ~(size_t)15;
        }
        w.marker(0xD9);
    }
    offsets[n] = w.n;
    if (w.n > capacity) {
        fm_set_error("object encode: the files need %zu bytes, the output holds %zu", w.n, capacity);
        return FM_ERR_ARG;
    }
    return 0;
}
