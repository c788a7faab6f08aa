"""Baseline JPEG frames: the host-side handle that MOT.step accepts (JPEGFrame), and the numpy statement of the decode
that csrc/jpeg_host.hip (markers, Huffman) and csrc/jpeg.hip (dequantisation, inverse DCT, chroma upsampling, colour
conversion) compute.  The arithmetic is libjpeg-turbo's default decode path, which is what Pillow runs, restated here
from its documented behaviour; it is integer and exact, so `decode_bgr` equals Pillow's decode bit for bit and the GPU
equals both (tests/test_jpeg_host.py, tests/test_jpeg_gpu.py).

Supported: baseline sequential DCT (SOF0), 8 bits, one interleaved scan, any restart interval, with one component
(greyscale) or three YCbCr components whose luma is sampled 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0) and whose chroma
is 1x1.  Everything else raises UnsupportedJPEG (a ValueError) naming what the file uses.

Inverse DCT ("ISLOW"; dequantise, column pass with a descale by 11 bits, row pass with a descale by 18, + 128, clamp):
    even:  z1 = (in2 + in6) * 4433, tmp2 = z1 - in6 * 15137, tmp3 = z1 + in2 * 6270,
           tmp0 = (in0 + in4) << 13, tmp1 = (in0 - in4) << 13,
           tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2
    odd:   t0, t1, t2, t3 = in7, in5, in3, in1; z1 = t0 + t3, z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3,
           z5 = (z3 + z4) * 9633, t0 *= 2446, t1 *= 16819, t2 *= 25172, t3 *= 12299, z1 *= -7373, z2 *= -20995,
           z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5, t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4
    out0/7 = tmp10 +- t3, out1/6 = tmp11 +- t2, out2/5 = tmp12 +- t1, out3/4 = tmp13 +- t0, each (x + (1 << (n-1))) >> n
Chroma upsampling ("fancy", triangle filter) over the chroma plane's REAL samples, CW = ceil(W / 2) (CH likewise), every
neighbour index clamped to the plane -- which gives the library's edge formulas:
    2x1:  out[2c] = (3 s[c] + s[c-1] + 1) >> 2,  out[2c+1] = (3 s[c] + s[c+1] + 2) >> 2
    2x2:  v[c] = 3 cur[c] + near[c] (near: the row above for the upper output row, below for the lower one),
          out[2c] = (3 v[c] + v[c-1] + 8) >> 4,  out[2c+1] = (3 v[c] + v[c+1] + 7) >> 4
    a chroma plane at most 2 samples wide is replicated instead (the library switches the filter off there)
Colour (cb = Cb - 128, cr = Cr - 128, arithmetic shifts, results clamped):
    R = Y + ((91881 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16)
"""
import ctypes as C

import numpy as np


class UnsupportedJPEG(ValueError):
    """A well-formed JPEG that uses something outside the supported subset (the message names it)."""


def _zigzag():
    order = sorted(((r, c) for r in range(8) for c in range(8)),
                   key=lambda p: (p[0] + p[1], p[0] if (p[0] + p[1]) % 2 else p[1]))
    return np.array([r * 8 + c for r, c in order], np.int32)


ZIGZAG = _zigzag()          # ZIGZAG[k]: row-major position in the block of the k-th coefficient of the stream
QT_ENTRIES = 3 * 64         # quantisation tables handed to the device: one per component slot


class WrongSizeJPEG(ValueError):
    """A JPEG whose frame size is not the one the caller asked for."""


class Header:
    """What `parse` returns: the frame geometry (the fields of fm_jpeg_info under the same names) plus the tables."""


def geometry(hd):
    """Fills in the MCU grid, block grids and coefficient offsets from width, height, ncomp, hsamp[0], vsamp[0]."""
    h0, v0 = (hd.hsamp[0], hd.vsamp[0]) if hd.ncomp == 3 else (1, 1)
    hd.mcu_w, hd.mcu_h = 8 * h0, 8 * v0
    hd.mcus_x, hd.mcus_y = -(-hd.width // hd.mcu_w), -(-hd.height // hd.mcu_h)
    hd.blocks_w, hd.blocks_h, hd.coef_offset = [0] * 3, [0] * 3, [0] * 3
    off = 0
    for c in range(hd.ncomp):
        hs, vs = (h0, v0) if c == 0 else (1, 1)
        hd.blocks_w[c], hd.blocks_h[c], hd.coef_offset[c] = hd.mcus_x * hs, hd.mcus_y * vs, off
        off += hd.blocks_w[c] * hd.blocks_h[c] * 64
    hd.coef_count = off
    return hd


def parse(data):
    """Marker segments of a JPEG file up to the start of its scan -> Header.  ValueError for malformed data,
    UnsupportedJPEG for files outside the supported subset."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise ValueError('not a JPEG file (no SOI marker)')
    hd = Header()
    hd.qt = {}                      # table id -> 64 values, row-major
    hd.dc, hd.ac = {}, {}           # table id -> (counts[16], symbols)
    hd.restart_interval = 0
    hd.adobe_transform = None
    hd.width = None
    pos = 2
    while True:
        if pos + 4 > n:
            raise ValueError('truncated before the scan')
        if data[pos] != 0xFF:
            raise ValueError('marker expected')
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            pos += 2
            continue
        ln = (data[pos + 2] << 8) | data[pos + 3]
        if ln < 2 or pos + 2 + ln > n:
            raise ValueError('truncated marker segment')
        seg = data[pos + 4:pos + 2 + ln]
        if m == 0xDB:
            q = 0
            while q < len(seg):
                prec, tid = seg[q] >> 4, seg[q] & 15
                if prec > 1 or tid > 3:
                    raise ValueError('bad quantisation table')
                size = 64 * (prec + 1)
                if q + 1 + size > len(seg):
                    raise ValueError('truncated quantisation table')
                raw = np.frombuffer(seg, np.uint8, size, q + 1).astype(np.uint16)
                vals = (raw[0::2] << 8 | raw[1::2]) if prec else raw
                t = np.zeros(64, np.uint16)
                t[ZIGZAG] = vals
                hd.qt[tid] = t
                q += 1 + size
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                if q + 17 > len(seg):
                    raise ValueError('truncated Huffman table')
                cls, tid = seg[q] >> 4, seg[q] & 15
                counts = list(seg[q + 1:q + 17])
                total = sum(counts)
                if cls > 1 or tid > 3 or total > 256 or q + 17 + total > len(seg):
                    raise ValueError('bad Huffman table')
                code = 0
                for c in counts:
                    code = (code + c) << 1
                    if code > 1 << 17:
                        raise ValueError('bad Huffman table')
                (hd.ac if cls else hd.dc)[tid] = (counts, list(seg[q + 17:q + 17 + total]))
                q += 17 + total
        elif m == 0xDD:
            if ln != 4:
                raise ValueError('bad DRI segment')
            hd.restart_interval = (seg[0] << 8) | seg[1]
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b'Adobe':
                hd.adobe_transform = seg[11]
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if m == 0xC2:
                raise UnsupportedJPEG('progressive JPEG (SOF2)')
            if m != 0xC0 and m != 0xC1:
                raise UnsupportedJPEG(f'JPEG process SOF{m - 0xC0} ({"arithmetic coding" if m >= 0xC9 else "lossless / hierarchical"})')
            if hd.width is not None:
                raise ValueError('two frame headers')
            if len(seg) < 6:
                raise ValueError('truncated frame header')
            prec = seg[0]
            hd.height, hd.width, hd.ncomp = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if len(seg) != 6 + 3 * hd.ncomp:
                raise ValueError('bad frame header')
            if prec != 8:
                raise UnsupportedJPEG(f'{prec}-bit samples')
            if hd.width == 0 or hd.height == 0:
                raise ValueError('empty frame')
            if hd.ncomp not in (1, 3):
                raise UnsupportedJPEG(f'{hd.ncomp} colour components (CMYK / YCCK)' if hd.ncomp == 4 else f'{hd.ncomp} colour components')
            hd.comp_id = [seg[6 + 3 * c] for c in range(hd.ncomp)]
            hd.hsamp = [seg[7 + 3 * c] >> 4 for c in range(hd.ncomp)] + [0] * (3 - hd.ncomp)
            hd.vsamp = [seg[7 + 3 * c] & 15 for c in range(hd.ncomp)] + [0] * (3 - hd.ncomp)
            hd.tq = [seg[8 + 3 * c] for c in range(hd.ncomp)]
            if any(not 1 <= s <= 4 for s in hd.hsamp[:hd.ncomp] + hd.vsamp[:hd.ncomp]) or any(t > 3 for t in hd.tq):
                raise ValueError('bad frame header')
        elif m == 0xDA:
            if hd.width is None:
                raise ValueError('scan before the frame header')
            if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
                raise ValueError('bad scan header')
            if seg[0] != hd.ncomp:
                raise UnsupportedJPEG('more than one scan')
            hd.td, hd.ta = [], []
            for c in range(hd.ncomp):
                if seg[1 + 2 * c] != hd.comp_id[c]:
                    raise ValueError('scan components do not match the frame')
                hd.td.append(seg[2 + 2 * c] >> 4)
                hd.ta.append(seg[2 + 2 * c] & 15)
            if seg[-3] != 0 or seg[-2] != 63 or seg[-1] != 0:
                raise ValueError('bad scan header')
            hd.scan_offset = pos + 2 + ln
            break
        elif m == 0xD9:
            raise ValueError('no scan')
        pos += 2 + ln
    if hd.ncomp == 3:
        if hd.adobe_transform == 0 or (hd.adobe_transform is None and hd.comp_id == [82, 71, 66]):
            raise UnsupportedJPEG('RGB-coded components (no YCbCr transform)')
        samp = (hd.hsamp[0], hd.vsamp[0])
        if samp not in ((1, 1), (2, 1), (2, 2)) or (hd.hsamp[1], hd.vsamp[1], hd.hsamp[2], hd.vsamp[2]) != (1, 1, 1, 1):
            raise UnsupportedJPEG('sampling factors ' + ', '.join(f'{hd.hsamp[c]}x{hd.vsamp[c]}' for c in range(3)))
    for c in range(hd.ncomp):
        if hd.tq[c] not in hd.qt or hd.td[c] not in hd.dc or hd.ta[c] not in hd.ac:
            raise ValueError('a table the scan names is missing')
    return geometry(hd)


def _lookup(counts, symbols):
    """16-bit look-up of a Huffman table: code length (0: no such code) and symbol for every 16-bit prefix."""
    length = np.zeros(1 << 16, np.uint8)
    symbol = np.zeros(1 << 16, np.uint8)
    code, k = 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            lo = code << (16 - ln)
            length[lo:lo + (1 << (16 - ln))] = ln
            symbol[lo:lo + (1 << (16 - ln))] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return length, symbol


def _segments(data, pos):
    """The scan's entropy-coded data split at its RSTn markers, byte stuffing removed."""
    segs, cur, n = [], bytearray(), len(data)
    expect = 0
    while pos < n:
        b = data[pos]
        if b != 0xFF:
            cur.append(b)
            pos += 1
            continue
        if pos + 1 >= n:
            break
        nx = data[pos + 1]
        if nx == 0:
            cur.append(0xFF)
            pos += 2
        elif nx == 0xFF:
            pos += 1
        elif nx == 0xD0 + expect:
            segs.append(bytes(cur))
            cur = bytearray()
            expect = (expect + 1) & 7
            pos += 2
        else:
            break
    segs.append(bytes(cur))
    return segs


def entropy_decode(data, hd=None):
    """Huffman-decodes the scan -> (coef, qt): coef int16 [coef_count], per component [block_row][block_col][64] over the
    MCU-padded grid, row-major inside a block (de-zigzagged), quantised; qt uint16 [3 * 64], one row-major table per
    component."""
    data = bytes(data)
    hd = parse(data) if hd is None else hd
    coef = np.zeros(hd.coef_count, np.int16)
    qt = np.zeros(QT_ENTRIES, np.uint16)
    for c in range(hd.ncomp):
        qt[64 * c:64 * c + 64] = hd.qt[hd.tq[c]]
    dct = [_lookup(*hd.dc[hd.td[c]]) for c in range(hd.ncomp)]
    act = [_lookup(*hd.ac[hd.ta[c]]) for c in range(hd.ncomp)]
    segs = _segments(data, hd.scan_offset)
    n_mcu = hd.mcus_x * hd.mcus_y
    per_seg = hd.restart_interval or n_mcu
    if len(segs) < -(-n_mcu // per_seg):
        raise ValueError('truncated scan')
    zz = [int(z) for z in ZIGZAG]
    blocks = []                                   # per MCU: (component, block row offset, block column offset)
    for c in range(hd.ncomp):
        hs, vs = (hd.mcu_w // 8, hd.mcu_h // 8) if c == 0 else (1, 1)
        blocks += [(c, by, bx) for by in range(vs) for bx in range(hs)]
    out = coef                                    # (int16 stores wrap like the C decoder's)
    mcu = 0
    for seg in segs:
        if mcu >= n_mcu:
            break
        acc = int.from_bytes(seg, 'big') << 64    # the segment as one integer, 64 zero bits behind it
        total = 8 * len(seg) + 64
        p = 0                                     # bits consumed
        pred = [0] * hd.ncomp

        def peek16():
            return (acc >> (total - p - 16)) & 0xFFFF

        for _ in range(min(per_seg, n_mcu - mcu)):
            my, mx = divmod(mcu, hd.mcus_x)
            for c, by, bx in blocks:
                hs, vs = (hd.mcu_w // 8, hd.mcu_h // 8) if c == 0 else (1, 1)
                base = hd.coef_offset[c] + ((my * vs + by) * hd.blocks_w[c] + mx * hs + bx) * 64
                if p + 16 > total:
                    raise ValueError('truncated scan')
                w = peek16()
                ln = int(dct[c][0][w])
                if not ln:
                    raise ValueError('bad Huffman code')
                s = int(dct[c][1][w])
                p += ln
                if s > 15:
                    raise ValueError('bad DC size')
                if s:
                    if p + 16 > total:
                        raise ValueError('truncated scan')
                    v = peek16() >> (16 - s)
                    p += s
                    if v < 1 << (s - 1):
                        v -= (1 << s) - 1
                    pred[c] += v
                pred[c] = ((pred[c] + 32768) & 0xFFFF) - 32768
                out[base] = pred[c]
                k = 1
                while k < 64:
                    if p + 16 > total:
                        raise ValueError('truncated scan')
                    w = peek16()
                    ln = int(act[c][0][w])
                    if not ln:
                        raise ValueError('bad Huffman code')
                    rs = int(act[c][1][w])
                    p += ln
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        k += 16
                        continue
                    k += r
                    if k > 63:
                        raise ValueError('run past coefficient 63')
                    if p + 16 > total:
                        raise ValueError('truncated scan')
                    v = peek16() >> (16 - s)
                    p += s
                    if v < 1 << (s - 1):
                        v -= (1 << s) - 1
                    out[base + zz[k]] = v
                    k += 1
            mcu += 1
        if p > 8 * len(seg):
            raise ValueError('truncated scan')
    if mcu < n_mcu:
        raise ValueError('truncated scan')
    return coef, qt


def idct_islow(blocks, qt):
    """blocks: int array [..., 64] of quantised coefficients (row-major), qt: 64 values -> uint8 samples [..., 8, 8]."""
    x = (np.asarray(blocks).astype(np.int64) * np.asarray(qt).astype(np.int64)).reshape(blocks.shape[:-1] + (8, 8))

    def pass_(a, shift):
        """1-D transform along the second-to-last axis."""
        i = [a[..., k, :] for k in range(8)]
        z1 = (i[2] + i[6]) * 4433
        tmp2 = z1 - i[6] * 15137
        tmp3 = z1 + i[2] * 6270
        tmp0 = (i[0] + i[4]) << 13
        tmp1 = (i[0] - i[4]) << 13
        tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
        t0, t1, t2, t3 = i[7], i[5], i[3], i[1]
        z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
        z5 = (z3 + z4) * 9633
        t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
        z1, z2 = z1 * -7373, z2 * -20995
        z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
        t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
        outs = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
        return np.stack([(o + (1 << (shift - 1))) >> shift for o in outs], axis=-2)

    ws = pass_(x, 11)                                               # columns: along the row index
    out = np.swapaxes(pass_(np.swapaxes(ws, -1, -2), 18), -1, -2)   # rows
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def component_planes(coef, qt, hd):
    """Sample planes [blocks_h * 8, blocks_w * 8] uint8 of every component (MCU padding included)."""
    planes = []
    for c in range(hd.ncomp):
        bh, bw = hd.blocks_h[c], hd.blocks_w[c]
        blk = np.asarray(coef[hd.coef_offset[c]:hd.coef_offset[c] + bh * bw * 64]).reshape(bh, bw, 64)
        s = idct_islow(blk, qt[64 * c:64 * c + 64])
        planes.append(np.ascontiguousarray(s.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)))
    return planes


def upsample(plane, hs, vs, width, height):
    """Chroma plane (MCU padding included) -> uint8 [height, width] at the luma's resolution.  hs, vs: the luma's sampling
    factors, (1, 1), (2, 1) or (2, 2)."""
    cw, ch = -(-width // hs), -(-height // vs)
    s = plane[:ch, :cw].astype(np.int32)
    if hs == 1:
        return s[:height, :width].astype(np.uint8)
    if cw <= 2:                                   # too narrow for the triangle filter: replication
        return np.repeat(np.repeat(s, vs, axis=0), 2, axis=1)[:height, :width].astype(np.uint8)
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    if vs == 1:
        out = np.empty((ch, 2 * cw), np.int32)
        out[:, 0::2] = (3 * s + left + 1) >> 2
        out[:, 1::2] = (3 * s + right + 2) >> 2
        return out[:height, :width].astype(np.uint8)
    above = np.concatenate([s[:1], s[:-1]], axis=0)
    below = np.concatenate([s[1:], s[-1:]], axis=0)
    out = np.empty((2 * ch, 2 * cw), np.int32)
    for r, near in ((0, above), (1, below)):
        v = 3 * s + near
        vl = np.concatenate([v[:, :1], v[:, :-1]], axis=1)
        vr = np.concatenate([v[:, 1:], v[:, -1:]], axis=1)
        out[r::2, 0::2] = (3 * v + vl + 8) >> 4
        out[r::2, 1::2] = (3 * v + vr + 7) >> 4
    return out[:height, :width].astype(np.uint8)


def ycc_to_bgr(y, cb, cr):
    """Equally shaped uint8 arrays Y, Cb, Cr -> uint8 [..., 3] in B, G, R order."""
    yy = np.asarray(y, np.int32)
    b = np.asarray(cb, np.int32) - 128
    r = np.asarray(cr, np.int32) - 128
    out = np.empty(yy.shape + (3,), np.uint8)
    out[..., 2] = np.clip(yy + ((91881 * r + 32768) >> 16), 0, 255)
    out[..., 1] = np.clip(yy + ((-22554 * b - 46802 * r + 32768) >> 16), 0, 255)
    out[..., 0] = np.clip(yy + ((116130 * b + 32768) >> 16), 0, 255)
    return out


def coefficients_to_bgr(coef, qt, hd):
    """The device's half of the decode in numpy: coefficients + tables -> BGR frame [height, width, 3] uint8."""
    planes = component_planes(coef, qt, hd)
    y = planes[0][:hd.height, :hd.width]
    if hd.ncomp == 1:
        return np.ascontiguousarray(np.repeat(y[:, :, None], 3, axis=2))
    hs, vs = hd.hsamp[0], hd.vsamp[0]
    return ycc_to_bgr(y, upsample(planes[1], hs, vs, hd.width, hd.height), upsample(planes[2], hs, vs, hd.width, hd.height))


def decode_bgr(data):
    """A supported JPEG file's bytes -> BGR frame [height, width, 3] uint8, equal to Pillow's decode of it."""
    hd = parse(data)
    coef, qt = entropy_decode(data, hd)
    return coefficients_to_bgr(coef, qt, hd)


# ---------------------------------------------------------------------------------------------- the native decoder
FM_ERR_ARG = -2
FM_ERR_UNSUPPORTED = -4


class JpegInfo(C.Structure):
    """fm_jpeg_info of include/fastmot_hip.h."""
    _fields_ = [('width', C.c_int), ('height', C.c_int), ('ncomp', C.c_int),
                ('hsamp', C.c_int * 3), ('vsamp', C.c_int * 3),
                ('mcu_w', C.c_int), ('mcu_h', C.c_int), ('mcus_x', C.c_int), ('mcus_y', C.c_int),
                ('restart_interval', C.c_int),
                ('blocks_w', C.c_int * 3), ('blocks_h', C.c_int * 3),
                ('unsupported', C.c_int),
                ('coef_offset', C.c_longlong * 3), ('coef_count', C.c_longlong)]


# fm_jpeg_info.unsupported (FM_JPEG_UNSUPPORTED_* of the header) -> what the file uses
UNSUPPORTED = {1: 'progressive JPEG (SOF2)', 2: 'arithmetic coding', 3: 'a lossless or hierarchical JPEG process',
               4: 'samples that are not 8-bit', 5: 'a number of colour components other than 1 or 3 (CMYK / YCCK)',
               6: 'RGB-coded components (no YCbCr transform)', 7: 'sampling factors other than 4:4:4, 4:2:2 and 4:2:0',
               8: 'more than one scan'}


def max_coefficients(width, height):
    """Coefficient count of the largest supported layout of a width x height frame (4:4:4 on a 16-pixel MCU grid)."""
    return 3 * (-(-width // 16) * 16) * (-(-height // 16) * 16)


class JPEGFrame:
    """Host frame that is a baseline JPEG file, entropy-decoded; MOT.step, the detectors and the ctx frame calls accept it
    wherever they accept a BGR ndarray.  The constructor parses the markers and Huffman-decodes the scan on the calling
    thread (csrc/jpeg_host.hip, the GIL released); dequantisation, inverse DCT, chroma upsampling and colour conversion
    run on the GPU while the frame is uploaded (csrc/jpeg.hip), and give the BGR frame Pillow decodes from the file.

    data: the file's bytes.  buffer (optional): an int16 array to decode into, e.g. one of ctx.pinned_jpeg_buffers(n)
    -- at least coef_count + 192 elements; it must stay unmodified until the step that uses the frame has returned.
    size (optional): the (width, height) the caller wants -- a file of another size raises WrongSizeJPEG (a ValueError)
    right after its header was parsed, before anything is allocated or decoded.
    ValueError (UnsupportedJPEG) for a JPEG outside the supported subset, naming what it uses; ValueError for data that is
    not a well-formed JPEG."""

    def __init__(self, data, buffer=None, size=None):
        from .. import _lib
        lib = _lib.load()
        data = bytes(data)
        info = JpegInfo()
        rc = lib.fm_jpeg_info(data, C.c_size_t(len(data)), C.byref(info))
        if rc == FM_ERR_UNSUPPORTED:
            raise UnsupportedJPEG('unsupported JPEG: the file uses ' + UNSUPPORTED.get(info.unsupported, 'an unknown feature'))
        if rc:
            raise ValueError(f'not a decodable JPEG: {lib.fm_last_error().decode()}')
        if size is not None and (info.width, info.height) != tuple(size):
            raise WrongSizeJPEG(f'JPEG is {info.width}x{info.height}, not {size[0]}x{size[1]}')
        need = info.coef_count + QT_ENTRIES
        if buffer is None:
            buffer = np.empty(need, np.int16)
        elif (not isinstance(buffer, np.ndarray) or buffer.dtype != np.int16 or buffer.ndim != 1 or not buffer.flags.c_contiguous
              or buffer.size < need):
            raise ValueError(f'buffer must be a contiguous int16 array of at least {need} elements')
        self.info = info
        self.buffer = buffer
        self.coef = buffer[:info.coef_count]
        self.qt = buffer[info.coef_count:need].view(np.uint16)
        rc = lib.fm_jpeg_entropy_decode(data, C.c_size_t(len(data)), C.byref(info), _lib._ptr(self.coef), _lib._ptr(self.qt))
        if rc:
            raise ValueError(f'not a decodable JPEG: {lib.fm_last_error().decode()}')
        self.size = (info.width, info.height)
        self.shape = (info.height, info.width, 3)          # of the BGR frame it becomes on the device

    def to_bgr(self):
        """The BGR frame [H, W, 3] uint8, decoded on the host (numpy: for callers that need the pixels, not for speed)."""
        hd = Header()
        for name in ('width', 'height', 'ncomp'):
            setattr(hd, name, getattr(self.info, name))
        hd.hsamp, hd.vsamp = list(self.info.hsamp), list(self.info.vsamp)
        return coefficients_to_bgr(self.coef, self.qt, geometry(hd))


# ---------------------------------------------------------------------------------------------- the native encoder
def encode_bgr(frame, quality=75, ctx=None):
    """BGR frame [H, W, 3] uint8 -> the bytes of a baseline JPEG file (YCbCr 4:2:0, Annex-K tables, a restart interval of
    one MCU row), encoded on the GPU (csrc/jpegenc.hip) with libjpeg's arithmetic: the file equals Pillow's
    `save(..., quality=quality, subsampling=2, restart_marker_rows=1)` byte for byte.
    ctx: the HipContext to encode on (default: the process-wide one).  ValueError for a quality outside 1..100 or a
    width / height outside 1..16384."""
    if not 1 <= int(quality) <= 100:
        raise ValueError(f'quality {quality} outside 1..100')
    if ctx is None:
        from ..runtime import get_context
        ctx = get_context()
    return ctx.jpeg_encode_bgr(frame, quality)


def encode_bound(width, height):
    """Largest file a width x height frame can become (0: a size the encoder does not take)."""
    from .. import _lib
    return _lib.load().fm_jpeg_encode_bound(C.c_int(width), C.c_int(height))


def encode_tables(quality):
    """(luminance, chrominance) quantisation tables of a quality, 64 values each, row-major (csrc/jpegenc_host.hip)."""
    from .. import _lib
    qt = np.zeros(128, np.uint16)
    _lib.check(_lib.load().fm_jpeg_encode_tables(C.c_int(quality), _lib._ptr(qt)))
    return qt[:64].copy(), qt[64:].copy()


def encode_header(width, height, quality, capacity=None):
    """The marker segments SOI .. SOS of the file the encoder writes for such a frame -> bytes."""
    from .. import _lib
    out = np.zeros(1024 if capacity is None else capacity, np.uint8)
    n = C.c_size_t(0)
    _lib.check(_lib.load().fm_jpeg_encode_header(C.c_int(width), C.c_int(height), C.c_int(quality), _lib._ptr(out), C.c_size_t(out.size), C.byref(n)))
    return out[:n.value].tobytes()


def encode_assemble(width, height, quality, segments, capacity=None):
    """The file from its entropy-coded, byte-stuffed MCU-row segments (a list of bytes) -> bytes (csrc/jpegenc_host.hip)."""
    from .. import _lib
    lens = np.array([len(s) for s in segments], np.uint32)
    segs = np.zeros(max(sum((len(s) + 15) & ~15 for s in segments), 16), np.uint8)
    at = 0
    for s in segments:
        segs[at:at + len(s)] = np.frombuffer(s, np.uint8)
        at += (len(s) + 15) & ~15
    cap = encode_bound(width, height) if capacity is None else capacity
    out = np.zeros(max(cap, 1), np.uint8)
    n = C.c_size_t(0)
    _lib.check(_lib.load().fm_jpeg_encode_assemble(C.c_int(width), C.c_int(height), C.c_int(quality), _lib._ptr(lens), _lib._ptr(segs),
                                                   C.c_size_t(segs.size), _lib._ptr(out), C.c_size_t(cap), C.byref(n)))
    return out[:n.value].tobytes()
