// Host half of the JPEG ingest path: marker parsing and Huffman decoding of a baseline JPEG file, the part of the
// format that is serial by construction.  What comes out -- the quantised coefficients, de-zigzagged, per component as
// [block_row][block_col][64] over the MCU-padded grid, and one quantisation table per component -- is what
// fm_frame_upload_jpeg (frames.hip) copies to the device, where jpeg.hip does everything that is parallel:
// dequantisation, inverse DCT, chroma upsampling, colour conversion.  fastmot_amd/utils/jpeg.py states the same decode in
// numpy; tests/test_jpeg_host.py compares the two entry for entry.
//
// No fm_ctx, no GPU, no state: both functions may be called from any number of threads at once.
//
// Every read of the input goes through a bounds check (`BitReader::fill`, the `need` checks of the marker loop), every
// write lands in coef[0, coef_count) by construction: the block address comes from the MCU counters, the position in
// the block from k <= 63, which is checked after every run.  Malformed data returns FM_ERR_ARG.
#include "common.h"

namespace {

constexpr int LOOK = 9;                       // bits of the Huffman look-ahead table

const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffTable {
    bool present = false;
    // look[prefix of LOOK bits]: (code length << 8) | symbol for codes of at most LOOK bits, 0 for longer (or no) codes
    uint16_t look[1 << LOOK];
    // canonical decoding of the longer codes: a code of length l is valid iff code <= maxcode[l], and its symbol is
    // symbols[code + delta[l]]
    // AC tables only -- fast[prefix of LOOK bits]: when a code AND the value behind it fit into LOOK bits,
    // (value << 8) | (run << 4) | (bits of both), else 0 (a value is never 0, so an entry in use is never 0)
    int16_t fast[1 << LOOK];
    int32_t maxcode[18];
    int32_t delta[17];
    uint8_t symbols[256];
};

struct Parsed {
    struct fm_jpeg_info info;
    uint16_t qt[4][64];                       // row-major
    bool qt_present[4] = {};
    HuffTable dc[4], ac[4];
    int tq[3], td[3], ta[3];
    size_t scan_offset = 0;
};

int fail(const char* what) {
    fm_set_error("JPEG: %s", what);
    return FM_ERR_ARG;
}

int unsupported(struct fm_jpeg_info* info, int code, const char* what) {
    info->unsupported = code;
    fm_set_error("JPEG: unsupported: %s", what);
    return FM_ERR_UNSUPPORTED;
}

int build_table(HuffTable& t, const uint8_t* counts, const uint8_t* symbols, int total) {
    memset(t.look, 0, sizeof t.look);
    memcpy(t.symbols, symbols, total);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        t.delta[l] = k - code;
        for (int i = 0; i < counts[l - 1]; ++i, ++code, ++k)
            if (l <= LOOK) {
                const int lo = code << (LOOK - l);
                if (lo + (1 << (LOOK - l)) > (1 << LOOK)) return fail("Huffman table with more codes than its lengths allow");
                for (int j = 0; j < (1 << (LOOK - l)); ++j) t.look[lo + j] = (uint16_t)((l << 8) | symbols[k]);
            }
        if (code > (1 << l)) return fail("Huffman table with more codes than its lengths allow");
        t.maxcode[l] = counts[l - 1] ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    for (int i = 0; i < (1 << LOOK); ++i) {
        t.fast[i] = 0;
        const int l = t.look[i] >> 8, rs = t.look[i] & 255, sz = rs & 15;
        if (!l || !sz || l + sz > LOOK) continue;
        int v = (i >> (LOOK - l - sz)) & ((1 << sz) - 1);
        if (v < (1 << (sz - 1))) v -= (1 << sz) - 1;
        if (v >= -128 && v <= 127) t.fast[i] = (int16_t)(v * 256 + (rs >> 4) * 16 + l + sz);
    }
    t.present = true;
    return 0;
}

// Fills in everything that follows from width, height, ncomp and the luma sampling factors.
void geometry(struct fm_jpeg_info* g) {
    const int h0 = g->ncomp == 3 ? g->hsamp[0] : 1, v0 = g->ncomp == 3 ? g->vsamp[0] : 1;
    g->mcu_w = 8 * h0, g->mcu_h = 8 * v0;
    g->mcus_x = (g->width + g->mcu_w - 1) / g->mcu_w;
    g->mcus_y = (g->height + g->mcu_h - 1) / g->mcu_h;
    long long off = 0;
    for (int c = 0; c < 3; ++c) {
        g->blocks_w[c] = g->blocks_h[c] = 0;
        g->coef_offset[c] = 0;
        if (c >= g->ncomp) continue;
        g->blocks_w[c] = g->mcus_x * (c ? 1 : h0);
        g->blocks_h[c] = g->mcus_y * (c ? 1 : v0);
        g->coef_offset[c] = off;
        off += (long long)g->blocks_w[c] * g->blocks_h[c] * 64;
    }
    g->coef_count = off;
}

int parse(const uint8_t* d, size_t n, Parsed& p) {
    struct fm_jpeg_info& g = p.info;
    memset(&g, 0, sizeof g);
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail("not a JPEG file (no SOI marker)");
    bool have_frame = false;
    int adobe = -1, comp_id[3] = {};
    size_t pos = 2;
    for (;;) {
        if (n - pos < 4) return fail("truncated before the scan");
        if (d[pos] != 0xFF) return fail("marker expected");
        const int m = d[pos + 1];
        if (m == 0xFF) { pos += 1; continue; }
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) { pos += 2; continue; }
        const size_t ln = ((size_t)d[pos + 2] << 8) | d[pos + 3];
        if (ln < 2 || n - pos - 2 < ln) return fail("truncated marker segment");
        const uint8_t* s = d + pos + 4;
        const size_t sl = ln - 2;
        if (m == 0xDB) {
            for (size_t q = 0; q < sl;) {
                const int prec = s[q] >> 4, id = s[q] & 15;
                if (prec > 1 || id > 3) return fail("bad quantisation table");
                const size_t size = 64 * (prec + 1);
                if (sl - q - 1 < size) return fail("truncated quantisation table");
                for (int k = 0; k < 64; ++k)
                    p.qt[id][ZIGZAG[k]] = prec ? (uint16_t)((s[q + 1 + 2 * k] << 8) | s[q + 2 + 2 * k]) : s[q + 1 + k];
                p.qt_present[id] = true;
                q += 1 + size;
            }
        } else if (m == 0xC4) {
            for (size_t q = 0; q < sl;) {
                if (sl - q < 17) return fail("truncated Huffman table");
                const int cls = s[q] >> 4, id = s[q] & 15;
                int total = 0;
                for (int i = 0; i < 16; ++i) total += s[q + 1 + i];
                if (cls > 1 || id > 3 || total > 256 || sl - q - 17 < (size_t)total) return fail("bad Huffman table");
                if (int rc = build_table(cls ? p.ac[id] : p.dc[id], s + q + 1, s + q + 17, total)) return rc;
                q += 17 + total;
            }
        } else if (m == 0xDD) {
            if (ln != 4) return fail("bad DRI segment");
            g.restart_interval = (s[0] << 8) | s[1];
        } else if (m == 0xEE) {
            if (sl >= 12 && !memcmp(s, "Adobe", 5)) adobe = s[11];
        } else if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            if (m == 0xC2) return unsupported(&g, FM_JPEG_UNSUPPORTED_PROGRESSIVE, "progressive (SOF2)");
            if (m >= 0xC9) return unsupported(&g, FM_JPEG_UNSUPPORTED_ARITHMETIC, "arithmetic coding");
            if (m > 0xC1) return unsupported(&g, FM_JPEG_UNSUPPORTED_PROCESS, "lossless or hierarchical process");
            if (have_frame) return fail("two frame headers");
            if (sl < 6) return fail("truncated frame header");
            g.height = (s[1] << 8) | s[2], g.width = (s[3] << 8) | s[4], g.ncomp = s[5];
            if (sl != 6 + 3 * (size_t)g.ncomp) return fail("bad frame header");
            if (s[0] != 8) return unsupported(&g, FM_JPEG_UNSUPPORTED_PRECISION, "samples that are not 8-bit");
            if (!g.width || !g.height) return fail("empty frame");
            if (g.ncomp != 1 && g.ncomp != 3) return unsupported(&g, FM_JPEG_UNSUPPORTED_COMPONENTS, "not 1 or 3 components");
            for (int c = 0; c < g.ncomp; ++c) {
                comp_id[c] = s[6 + 3 * c];
                g.hsamp[c] = s[7 + 3 * c] >> 4, g.vsamp[c] = s[7 + 3 * c] & 15;
                p.tq[c] = s[8 + 3 * c];
                if (g.hsamp[c] < 1 || g.hsamp[c] > 4 || g.vsamp[c] < 1 || g.vsamp[c] > 4 || p.tq[c] > 3) return fail("bad frame header");
            }
            have_frame = true;
        } else if (m == 0xDA) {
            if (!have_frame) return fail("scan before the frame header");
            if (sl < 1 || sl != 4 + 2 * (size_t)s[0]) return fail("bad scan header");
            if (s[0] != g.ncomp) return unsupported(&g, FM_JPEG_UNSUPPORTED_SCANS, "more than one scan");
            for (int c = 0; c < g.ncomp; ++c) {
                if (s[1 + 2 * c] != comp_id[c]) return fail("scan components do not match the frame");
                p.td[c] = s[2 + 2 * c] >> 4, p.ta[c] = s[2 + 2 * c] & 15;
                if (p.td[c] > 3 || p.ta[c] > 3) return fail("bad scan header");
            }
            if (s[sl - 3] != 0 || s[sl - 2] != 63 || s[sl - 1] != 0) return fail("bad scan header");
            p.scan_offset = pos + 2 + ln;
            break;
        } else if (m == 0xD9) {
            return fail("no scan");
        }
        pos += 2 + ln;
    }
    if (g.ncomp == 3) {
        if (adobe == 0 || (adobe < 0 && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B'))
            return unsupported(&g, FM_JPEG_UNSUPPORTED_COLORSPACE, "RGB-coded components");
        const int h0 = g.hsamp[0], v0 = g.vsamp[0];
        const bool luma_ok = (h0 == 1 && v0 == 1) || (h0 == 2 && v0 == 1) || (h0 == 2 && v0 == 2);
        if (!luma_ok || g.hsamp[1] != 1 || g.vsamp[1] != 1 || g.hsamp[2] != 1 || g.vsamp[2] != 1)
            return unsupported(&g, FM_JPEG_UNSUPPORTED_SAMPLING, "sampling factors other than 4:4:4, 4:2:2, 4:2:0");
    }
    for (int c = 0; c < g.ncomp; ++c)
        if (!p.qt_present[p.tq[c]] || !p.dc[p.td[c]].present || !p.ac[p.ta[c]].present) return fail("a table the scan names is missing");
    geometry(&g);
    return 0;
}

// MSB-first bit reader over the scan's bytes.  It removes 0xFF00 stuffing and never moves past a marker or the end of
// the data: from there on it supplies zero bits and counts them (`fake`), and `overrun()` tells whether any of those
// were consumed -- a valid stream consumes none.
struct BitReader {
    const uint8_t* d;
    size_t n, pos;
    uint64_t acc = 0;       // the next `bits` bits of the stream, right-aligned
    int bits = 0, fake = 0;

    inline void fill() {    // at least 33 bits afterwards: a Huffman code (<= 16) and the value behind it (<= 15)
        if (bits > 32) return;
        if (fake == 0 && n - pos >= 4) {        // four bytes at once when none of them is 0xFF
            const uint32_t w = ((uint32_t)d[pos] << 24) | ((uint32_t)d[pos + 1] << 16) | ((uint32_t)d[pos + 2] << 8) | d[pos + 3];
            const uint32_t x = ~w;
            if (!((x - 0x01010101u) & ~x & 0x80808080u)) {
                acc = (acc << 32) | w;
                bits += 32;
                pos += 4;
                return;
            }
        }
        while (bits <= 56) {
            unsigned b = 0;
            if (pos < n && fake == 0) {
                b = d[pos];
                if (b != 0xFF) {
                    ++pos;
                } else if (pos + 1 < n && d[pos + 1] == 0) {
                    pos += 2;
                } else {    // a marker, or a 0xFF that ends the data
                    b = 0;
                    fake += 8;
                }
            } else {
                fake += 8;
            }
            acc = (acc << 8) | b;
            bits += 8;
        }
    }
    inline unsigned peek(int k) const { return (unsigned)(acc >> (bits - k)) & ((1u << k) - 1); }
    inline void skip(int k) { bits -= k; }
    inline bool overrun() const { return bits < fake; }
    void restart() { acc = 0, bits = 0, fake = 0; }
};

// One Huffman symbol; at least 16 bits are in the reader.  -1: no such code.
inline int decode_symbol(BitReader& br, const HuffTable& t) {
    const unsigned e = t.look[br.peek(LOOK)];
    if (e) {
        br.skip(e >> 8);
        return e & 255;
    }
    const int v = (int)br.peek(16);
    for (int l = LOOK + 1; l <= 16; ++l) {
        const int code = v >> (16 - l);
        if (code <= t.maxcode[l]) {
            br.skip(l);
            return t.symbols[code + t.delta[l]];
        }
    }
    return -1;
}

// The s-bit value that follows a symbol of size s (1 <= s <= 15), sign-extended the JPEG way.
inline int receive_extend(BitReader& br, int s) {
    const int v = (int)br.peek(s);
    br.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

}  // namespace

int fm_jpeg_layout(int width, int height, int ncomp, int hsamp0, int vsamp0, struct fm_jpeg_info* out) {
    FM_CHECK_ARG(out && width > 0 && height > 0 && width <= 65535 && height <= 65535 && (ncomp == 1 || ncomp == 3));
    FM_CHECK_ARG(ncomp == 1 || (hsamp0 == 1 && vsamp0 == 1) || (hsamp0 == 2 && vsamp0 == 1) || (hsamp0 == 2 && vsamp0 == 2));
    memset(out, 0, sizeof *out);
    out->width = width, out->height = height, out->ncomp = ncomp;
    for (int c = 0; c < ncomp; ++c) out->hsamp[c] = out->vsamp[c] = 1;
    if (ncomp == 3) out->hsamp[0] = hsamp0, out->vsamp[0] = vsamp0;
    geometry(out);
    return 0;
}

extern "C" int fm_jpeg_info(const uint8_t* data, size_t n, struct fm_jpeg_info* out) {
    FM_CHECK_ARG(data && out);
    Parsed* p = new Parsed;
    const int rc = parse(data, n, *p);
    *out = p->info;
    delete p;
    return rc;
}

extern "C" int fm_jpeg_entropy_decode(const uint8_t* data, size_t n, const struct fm_jpeg_info* info, int16_t* coef, uint16_t* qt) {
    FM_CHECK_ARG(data && info && coef && qt);
    Parsed* pp = new Parsed;
    struct Free { Parsed* p; ~Free() { delete p; } } guard{pp};
    Parsed& p = *pp;
    if (int rc = parse(data, n, p)) return rc;
    const struct fm_jpeg_info& g = p.info;
    // the caller sized `coef` from `info`: it must be this file's
    FM_CHECK_ARG(info->width == g.width && info->height == g.height && info->ncomp == g.ncomp && info->coef_count == g.coef_count &&
                 info->hsamp[0] == g.hsamp[0] && info->vsamp[0] == g.vsamp[0]);
    memset(qt, 0, 3 * 64 * sizeof(uint16_t));
    for (int c = 0; c < g.ncomp; ++c) memcpy(qt + 64 * c, p.qt[p.tq[c]], 64 * sizeof(uint16_t));
    memset(coef, 0, (size_t)g.coef_count * sizeof(int16_t));

    BitReader br{data, n, p.scan_offset};
    const long long n_mcu = (long long)g.mcus_x * g.mcus_y;
    const int interval = g.restart_interval;
    int pred[3] = {0, 0, 0};
    int next_rst = 0;
    long long until_restart = interval ? interval : n_mcu;
    const int hs0 = g.mcu_w / 8, vs0 = g.mcu_h / 8;
    for (int my = 0; my < g.mcus_y; ++my)
        for (int mx = 0; mx < g.mcus_x; ++mx) {
            if (until_restart == 0) {
                // the interval's bits are used up: what is left in the reader is padding; the marker is where it stopped
                if (br.overrun()) return fail("truncated or corrupt scan");
                size_t q = br.pos;
                while (q + 1 < n && data[q] == 0xFF && data[q + 1] == 0xFF) ++q;
                if (q + 1 >= n || data[q] != 0xFF || data[q + 1] != 0xD0 + next_rst) return fail("restart marker missing");
                br.pos = q + 2;
                br.restart();
                next_rst = (next_rst + 1) & 7;
                pred[0] = pred[1] = pred[2] = 0;
                until_restart = interval;
            }
            --until_restart;
            for (int c = 0; c < g.ncomp; ++c) {
                const int hs = c ? 1 : hs0, vs = c ? 1 : vs0;
                const HuffTable& dct = p.dc[p.td[c]];
                const HuffTable& act = p.ac[p.ta[c]];
                for (int by = 0; by < vs; ++by)
                    for (int bx = 0; bx < hs; ++bx) {
                        int16_t* blk = coef + g.coef_offset[c] + ((long long)(my * vs + by) * g.blocks_w[c] + (mx * hs + bx)) * 64;
                        br.fill();
                        int s = decode_symbol(br, dct);
                        if (s < 0) return fail("Huffman code that does not exist");
                        if (s > 15) return fail("bad DC size");
                        if (s) pred[c] += receive_extend(br, s);
                        pred[c] = (int16_t)pred[c];
                        blk[0] = (int16_t)pred[c];
                        for (int k = 1; k < 64;) {
                            br.fill();
                            if (const int e = act.fast[br.peek(LOOK)]) {     // code and value in one look-up
                                k += (e >> 4) & 15;
                                if (k > 63) return fail("run past coefficient 63");
                                br.skip(e & 15);
                                blk[ZIGZAG[k++]] = (int16_t)(e >> 8);
                                continue;
                            }
                            const int rs = decode_symbol(br, act);
                            if (rs < 0) return fail("Huffman code that does not exist");
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (!s) {
                                if (r != 15) break;      // EOB
                                k += 16;                 // ZRL
                                continue;
                            }
                            k += r;
                            if (k > 63) return fail("run past coefficient 63");
                            blk[ZIGZAG[k++]] = (int16_t)receive_extend(br, s);
                        }
                        if (br.overrun()) return fail("truncated or corrupt scan");
                    }
            }
        }
    return 0;
}
