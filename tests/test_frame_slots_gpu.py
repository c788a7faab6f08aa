"""GPU: frames of different formats through the same slots (csrc/frames.hip).  The per-format tests send one format
through the three entry points; here every format meets the look-ahead buffers, staging and events another one has just
used, because the promotes swap them.  Every comparison is np.array_equal between ctx.frame_read() and the frame's numpy
judge, the one its per-format test uses."""
import numpy as np
import pytest
import torch

import jpeg_cases as jc
from fastmot_amd import BayerFrame, DeepFrame, DeviceArrayFrame, JPEGFrame, NV12Frame, PackedFrame, PlanarFrame, SourceFrame
from fastmot_amd.utils import devarray as D
from fastmot_amd.utils.nv12 import nv12_to_bgr
from fastmot_amd.utils.packed import row_bytes
from fastmot_amd.videoio import resize_bgr

pytestmark = pytest.mark.gpu

W, H = 32, 16


def padded(rng, rows, cols, pad, dtype=np.uint8, top=256):
    """Random (rows, cols) samples in pageable memory whose rows lie `pad` samples further apart (the padding random too)."""
    return rng.integers(0, top, (rows, cols + pad), dtype=dtype)[:, :cols]


def packed(rng, w, h, fmt, pad):
    return PackedFrame(padded(rng, h, row_bytes(w, fmt), pad), fmt, (w, h))


def pool_of(ctx, rng):
    """(name, frame, judge): one frame per kind in pageable memory, rows padded where the format has a pitch, so that every
    staging and event path runs."""
    bgr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    nv12 = NV12Frame(padded(rng, H, W, 6), padded(rng, H // 2, W, 6))
    planar = PlanarFrame(padded(rng, H, W, 3), padded(rng, H // 2, W // 2, 3), padded(rng, H // 2, W // 2, 3), '420')
    yuy2, bgrx = packed(rng, W, H, 'yuy2', 4), packed(rng, W, H, 'bgrx', 4)
    bayer = BayerFrame(padded(rng, H, W, 5), 'rggb')
    deep = DeepFrame(padded(rng, H, W, 2, np.uint16, 1024), padded(rng, H // 2, W // 2, 2, np.uint16, 1024),
                     padded(rng, H // 2, W // 2, 2, np.uint16, 1024), '420', 10)
    host = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    device = DeviceArrayFrame(torch.from_numpy(host).to(torch.device('cuda', ctx.device)), 'rgb', layout='hwc')
    data = jc.encode(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), '420', 75, 0)
    src_bgr = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)
    src_packed = packed(rng, 37, 21, 'uyvy', 5)
    return [('bgr', bgr, bgr),
            ('nv12', nv12, nv12_to_bgr(nv12.y, nv12.uv, nv12.matrix)),
            ('planar 420', planar, planar.to_bgr()),
            ('packed yuy2', yuy2, yuy2.to_bgr()),
            ('packed bgrx', bgrx, bgrx.to_bgr()),
            ('bayer rggb', bayer, bayer.to_bgr()),
            ('deep 420 10 bit', deep, deep.to_bgr()),
            ('device hwc', device, D.to_bgr(host, 'rgb', layout='hwc')),
            ('jpeg', JPEGFrame(data), jc.pillow_bgr(data)),
            ('source bgr 40x24', SourceFrame(src_bgr), resize_bgr(src_bgr, (W, H))),
            ('source packed 37x21', SourceFrame(src_packed), resize_bgr(src_packed.to_bgr(), (W, H)))]


def test_formats_share_the_slots(ctx):
    ctx.frame_configure(W, H, 2)
    ctx.next_frame, ctx.ahead_frames, ctx.bound_frame = None, [], None
    pool = pool_of(ctx, np.random.default_rng(11))
    assert len(pool) == 11

    def through_the_slots(entries, tag):
        for k, i in enumerate(entries, 1):
            ctx.frame_upload_ahead(k, pool[i][1])
        for i in entries:
            ctx.frame_promote_next()
            assert np.array_equal(ctx.frame_read(), pool[i][2]), (tag, pool[i][0])

    # after round 0 the promotes have swapped the slots' buffers: each physical buffer and event meets a new format
    for r in range(3):
        through_the_slots([(r + 3 * j) % len(pool) for j in range(3)], f'round {r}')
    # (the rounds' formula leaves the two off-size sources out: their staging stays with the slot number at a promote)
    through_the_slots([9, 10, 8], 'off-size sources')

    ctx.frame_ring_store(1, pool[10][1])
    ctx.frame_ring_store(0, pool[6][1])
    ctx.frame_upload(pool[3][1])
    assert np.array_equal(ctx.frame_read(), pool[3][2]), 'upload'
    for index, i in ((1, 10), (0, 6)):
        ctx.frame_ring_select(index)
        assert np.array_equal(ctx.frame_read(), pool[i][2]), ('ring', index, pool[i][0])
    ctx.frame_configure(16, 16)
