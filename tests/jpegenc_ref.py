"""Numpy restatement of the arithmetic of the GPU JPEG encoder (csrc/jpegenc.hip): a test helper, not product
code.  BGR frame -> quantised coefficients of a baseline 4:2:0 file, in the layout `utils.jpeg.entropy_decode` returns
(per component [block_row][block_col][64] over the MCU-padded grid, row-major inside a block), so the two compare entry
for entry.

The steps are libjpeg's, restated from its documented behaviour: integer colour conversion, edge replication of the
full-resolution planes to the MCU grid (chroma rows below the image: the last AVERAGED row repeated), 2 x 2 chroma
averaging with the alternating bias, the `islow` forward DCT on
samples - 128, rounding division by 8 x the quality-scaled Annex-K table, and the dummy-block rule for luma blocks that
lie wholly outside the image's block grid."""
import numpy as np

BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)


def quality_tables(quality):
    """(luma, chroma) quantisation tables, 64 values each, row-major."""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255).astype(np.uint16) for base in (BASE_LUMA, BASE_CHROMA))


def bgr_to_ycc(bgr):
    b, g, r = (bgr[..., c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def pad_edge(plane, h, w):
    return np.pad(plane, ((0, h - plane.shape[0]), (0, w - plane.shape[1])), mode='edge')


def downsample(plane):
    """2 x 2 averaging, bias 1, 2, 1, 2 ... along the output columns."""
    s = plane[0::2, 0::2] + plane[0::2, 1::2] + plane[1::2, 0::2] + plane[1::2, 1::2]
    bias = 1 + (np.arange(s.shape[1]) & 1)
    return (s + bias[None, :]) >> 2


def fdct_islow(blocks):
    """[..., 8, 8] samples - 128 (int64) -> coefficients scaled by 8, [..., 8, 8]."""
    def descale(x, n):
        return (x + (1 << (n - 1))) >> n

    def pass_(d, first):
        """1-D transform along the last axis."""
        d = [d[..., k] for k in range(8)]
        tmp0, tmp7 = d[0] + d[7], d[0] - d[7]
        tmp1, tmp6 = d[1] + d[6], d[1] - d[6]
        tmp2, tmp5 = d[2] + d[5], d[2] - d[5]
        tmp3, tmp4 = d[3] + d[4], d[3] - d[4]
        tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
        n = 11 if first else 15
        o = [None] * 8
        o[0] = (tmp10 + tmp11) << 2 if first else descale(tmp10 + tmp11, 2)
        o[4] = (tmp10 - tmp11) << 2 if first else descale(tmp10 - tmp11, 2)
        z1 = (tmp12 + tmp13) * 4433
        o[2] = descale(z1 + tmp13 * 6270, n)
        o[6] = descale(z1 - tmp12 * 15137, n)
        z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
        z5 = (z3 + z4) * 9633
        tmp4, tmp5, tmp6, tmp7 = tmp4 * 2446, tmp5 * 16819, tmp6 * 25172, tmp7 * 12299
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        o[7] = descale(tmp4 + z1 + z3, n)
        o[5] = descale(tmp5 + z2 + z4, n)
        o[3] = descale(tmp6 + z2 + z3, n)
        o[1] = descale(tmp7 + z1 + z4, n)
        return np.stack(o, axis=-1)

    rows = pass_(blocks, True)
    return np.swapaxes(pass_(np.swapaxes(rows, -1, -2), False), -1, -2)


def quantise(coef, table):
    """coef [..., 64] scaled by 8, table 64 values -> sign(c) * ((|c| + div / 2) // div), div = 8 * table."""
    div = table.astype(np.int64) * 8
    return np.sign(coef) * ((np.abs(coef) + (div >> 1)) // div)


def plane_blocks(plane, table):
    """Sample plane [8 bh, 8 bw] -> quantised coefficients [bh, bw, 64]."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    blk = (plane - 128).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
    return quantise(fdct_islow(blk).reshape(bh, bw, 64), table)


def encode_coefficients(bgr, quality):
    """BGR [H, W, 3] uint8 -> (coef int16 [coef_count], qt uint16 [192]) of the 4:2:0 file, as entropy_decode lays them out."""
    h, w = bgr.shape[:2]
    my, mx = -(-h // 16), -(-w // 16)
    luma, chroma = quality_tables(quality)
    y, cb, cr = bgr_to_ycc(bgr)
    yb = plane_blocks(pad_edge(y, 16 * my, 16 * mx), luma)

    def chroma_plane(p):
        """Columns padded at full resolution, rows to an even count; averaged; THEN the last averaged row repeated."""
        return pad_edge(downsample(pad_edge(p, h + (h & 1), 16 * mx)), 8 * my, 8 * mx)

    # dummy blocks: block columns / rows past the last one that holds image pixels; coded order inside an MCU is
    # (0,0) (0,1) (1,0) (1,1), each dummy takes the DC of the block before it
    real_w, real_h = -(-w // 8), -(-h // 8)
    for r in range(2 * my):
        for c in range(2 * mx):
            if c < real_w and r < real_h:
                continue
            k = (r & 1) * 2 + (c & 1)               # >= 1: block 0 of an MCU always holds pixels
            pr, pc = (r & ~1) + ((k - 1) >> 1), (c & ~1) + ((k - 1) & 1)
            yb[r, c, :] = 0
            yb[r, c, 0] = yb[pr, pc, 0]
    parts = [yb, plane_blocks(chroma_plane(cb), chroma), plane_blocks(chroma_plane(cr), chroma)]
    coef = np.concatenate([p.reshape(-1) for p in parts]).astype(np.int16)
    return coef, np.concatenate([luma, chroma, chroma]).astype(np.uint16)


def interior_mask(width, height):
    """Per coefficient (same layout): True for the blocks that are compared with Pillow's -- every sample of the block
    exists in its component's plane, width x height for luma, ceil(width / 2) x ceil(height / 2) for chroma.  For luma
    that is "all source pixels inside the image"; the chroma set is larger than that by the blocks whose last column /
    row averages the image's last odd column / row with its replica, which libjpeg computes the same way."""
    my, mx = -(-height // 16), -(-width // 16)
    yr, yc = np.arange(2 * my)[:, None], np.arange(2 * mx)[None, :]
    ym = (8 * yr + 8 <= height) & (8 * yc + 8 <= width)
    cr, cc = np.arange(my)[:, None], np.arange(mx)[None, :]
    cm = (8 * cr + 8 <= -(-height // 2)) & (8 * cc + 8 <= -(-width // 2))
    return np.concatenate([np.repeat(m.reshape(-1), 64) for m in (ym, cm, cm)])


def _codes(counts, symbols):
    """Huffman table as DHT states it -> {symbol: (code, length)}."""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            out[symbols[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def entropy_segments(coef, hd):
    """Coefficients (entropy_decode's layout) -> one byte-stuffed entropy-coded segment per MCU row, coded with the tables
    of the parsed header `hd` (utils.jpeg.parse of the encoder's header): the DC predictors start at zero in every row and
    the row is padded to a byte with 1-bits."""
    from fastmot_amd.utils.jpeg import ZIGZAG
    zz = [int(z) for z in ZIGZAG]
    dc = [_codes(*hd.dc[hd.td[c]]) for c in range(3)]
    ac = [_codes(*hd.ac[hd.ta[c]]) for c in range(3)]
    coef = np.asarray(coef).astype(np.int64)
    segs = []
    for my in range(hd.mcus_y):
        acc, nbits, pred = 0, 0, [0, 0, 0]

        def put(code, n):
            nonlocal acc, nbits
            acc = (acc << n) | code
            nbits += n

        def value(v):
            n = int(abs(v)).bit_length()
            return (v if v >= 0 else v - 1) & ((1 << n) - 1), n

        for mx in range(hd.mcus_x):
            for c, by, bx in [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (2, 0, 0)]:
                hs = 2 if c == 0 else 1
                base = hd.coef_offset[c] + ((my * hs + by) * hd.blocks_w[c] + mx * hs + bx) * 64
                blk = [int(coef[base + zz[k]]) for k in range(64)]
                bits, n = value(blk[0] - pred[c])
                pred[c] = blk[0]
                put(*dc[c][n])
                put(bits, n)
                run = 0
                for k in range(1, 64):
                    if blk[k] == 0:
                        run += 1
                        continue
                    while run > 15:
                        put(*ac[c][0xF0])
                        run -= 16
                    bits, n = value(blk[k])
                    put(*ac[c][(run << 4) | n])
                    put(bits, n)
                    run = 0
                if run:
                    put(*ac[c][0])
        pad = -nbits & 7
        put((1 << pad) - 1, pad)
        segs.append(acc.to_bytes(nbits // 8, 'big').replace(b'\xff', b'\xff\x00'))
    return segs
