"""GPU: frames that lie in device memory (fm_frame_upload_device / fm_frame_upload_ahead_device /
fm_frame_ring_store_device), csrc/devsrc.hip.  The device memory is torch's, on the context's device; every conversion
is exact, so every comparison is np.array_equal against fastmot_amd.utils.devarray.to_bgr (pinned by independent
statements in test_devarray_host.py).

Sizes: those of test_packed_gpu.py -- 1x1 and 2x2 (a single thread), 3x5 (ragged runs only), 34x18 (3 W = 102: rows whose
BGR bytes begin 8-byte aligned, 4-byte aligned and neither), 33x7 (odd, several threads a row), 130x6 (17 threads a
row), 1920x2 (a second workgroup, which begins inside a row), 12x3 (a whole run beside one of four pixels); NV12 takes
the even ones and 6x4.  Every case runs on a contiguous tensor (the 16- / 8-byte loads) and on a view of a wider tensor
that begins an odd number of elements into it with an odd number of elements between its rows (the element-wise
loads, and for float32 the 4-byte ones)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch as _torch       # before the library is loaded: the HIP runtime that is loaded first serves both, see DeviceArrayFrame

from fastmot_amd import DeviceArrayFrame, LensMap, NV12Frame, SourceFrame, _lib
from fastmot_amd.utils import devarray as D
from fastmot_amd.utils.lens import remap_bgr
from fastmot_amd.utils.nv12 import bgr_to_nv12
from fastmot_amd.videoio import resize_bgr

pytestmark = pytest.mark.gpu

FM_ERR_ARG = -2
SIZES = [(1, 1), (2, 2), (3, 5), (34, 18), (33, 7), (130, 6), (1920, 2), (12, 3)]
NV12_SIZES = [s for s in SIZES if not (s[0] | s[1]) & 1] + [(6, 4)]
HWC_ORDERS = ['rgb', 'bgr', 'rgbx', 'bgrx', 'xrgb', 'xbgr']
CHW_KINDS = [(dt, order, fr) for dt in ('uint8', 'float16', 'float32') for order in ('rgb', 'bgr')
             for fr in (((0, 1), (0, 255)) if dt != 'uint8' else ((0, 1),))]
ids = lambda s: f'{s[0]}x{s[1]}'


@pytest.fixture(scope='module')
def torch():
    assert _torch.cuda.is_available()
    return _torch


def configure(ctx, w, h, ring=0):
    ctx.frame_configure(w, h, ring)
    ctx.next_frame, ctx.ahead_frames, ctx.bound_frame = None, [], None


def on_device(torch, ctx, host, view, hwc=False):
    """The host array on the context's device: contiguous, or -- `view` -- inside a wider tensor, an odd number of elements
    from its start, an odd number of elements between its rows and any number between its planes.  `hwc`: the last two
    axes are one row."""
    dev = torch.device('cuda', ctx.device)
    src = torch.from_numpy(np.ascontiguousarray(host))
    if not view:
        return src.to(dev)
    shape = tuple(host.shape)
    row = shape[1] * shape[2] if hwc else shape[-1]
    pitch = row + 1 + (row & 1)                                   # odd
    if hwc:
        strides, total = (pitch, shape[2], 1), shape[0] * pitch
    elif host.ndim == 2:
        strides, total = (pitch, 1), shape[0] * pitch
    else:
        plane = shape[1] * pitch + 5
        strides, total = (plane, pitch, 1), 3 * plane
    offset = 3
    buf = torch.full((offset + total + 7,), 77, dtype=src.dtype, device=dev)
    out = torch.as_strided(buf, shape, strides, offset)
    out.copy_(src)
    es = host.dtype.itemsize
    assert (out.data_ptr() // es) % 2 == 1 and out.data_ptr() - buf.data_ptr() == offset * es and pitch % 2 == 1
    return out


def floats(rng, shape, dtype, float_range):
    """Values over and beyond the range, with exact halves, NaN, infinities and zeros of both signs among them."""
    top = float_range[1]
    x = rng.uniform(-0.1 * top, 1.1 * top, shape).astype(np.float32)
    flat = x.reshape(-1)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, top, 0.5 * top / 255, 1.5 * top / 255, 2.5 * top / 255, 254.5 * top / 255], np.float32)
    n = min(len(special), flat.size)
    flat[rng.choice(flat.size, n, replace=False)] = special[:n]
    if top == 255:
        half = rng.choice(flat.size, max(1, flat.size // 8), replace=False)
        flat[half] = rng.integers(0, 256, len(half)) + 0.5
    return x.astype(dtype)


def hwc_case(torch, ctx, rng, w, h, order, view):
    c = 3 if order in ('rgb', 'bgr') else 4
    host = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    t = on_device(torch, ctx, host, view, hwc=True)
    return DeviceArrayFrame(t, order, layout='hwc'), D.to_bgr(host, order, layout='hwc')    # (H = 3 is a (3, H, W) shape too)


def chw_case(torch, ctx, rng, w, h, dtype, order, float_range, view):
    host = rng.integers(0, 256, (3, h, w), dtype=np.uint8) if dtype == 'uint8' else floats(rng, (3, h, w), dtype, float_range)
    t = on_device(torch, ctx, host, view)
    return DeviceArrayFrame(t, order, float_range, layout='chw'), D.to_bgr(host, order, float_range, layout='chw')    # (W = 3 ...)


def nv12_case(torch, ctx, rng, w, h, matrix, view):
    y, uv = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
    if h > 1:
        y[0], y[-1] = 0, 255
    ty, tuv = on_device(torch, ctx, y, view), on_device(torch, ctx, uv, view)
    return DeviceArrayFrame.nv12(ty, tuv, matrix), D.to_bgr((y, uv), matrix=matrix)


def four_kinds(torch, ctx, rng, w, h, view=False):
    """One frame of each of the four conversions at w x h (w, h even) -> [(name, frame, expected BGR)]."""
    return [('hwc', *hwc_case(torch, ctx, rng, w, h, 'bgrx', view)),
            ('chw-u8', *chw_case(torch, ctx, rng, w, h, 'uint8', 'rgb', (0, 1), view)),
            ('chw-f16', *chw_case(torch, ctx, rng, w, h, 'float16', 'rgb', (0, 1), view)),
            ('chw-f32', *chw_case(torch, ctx, rng, w, h, 'float32', 'bgr', (0, 255), view)),
            ('nv12', *nv12_case(torch, ctx, rng, w, h, 'bt709', view))]


# ---- 1. bit-exact for every layout
@pytest.mark.parametrize('view', [False, True], ids=['contiguous', 'odd-view'])
@pytest.mark.parametrize('size', SIZES, ids=ids)
def test_hwc_and_chw_equal_to_bgr(ctx, torch, size, view):
    w, h = size
    rng = np.random.default_rng(w * 131 + h + view)
    configure(ctx, w, h)
    for order in HWC_ORDERS:
        f, want = hwc_case(torch, ctx, rng, w, h, order, view)
        ctx.frame_upload(f)
        assert np.array_equal(ctx.frame_read(), want), ('hwc', order)
        assert f.done()
    for dtype, order, fr in CHW_KINDS:
        f, want = chw_case(torch, ctx, rng, w, h, dtype, order, fr, view)
        ctx.frame_upload(f)
        assert np.array_equal(ctx.frame_read(), want), ('chw', dtype, order, fr)


@pytest.mark.parametrize('view', [False, True], ids=['contiguous', 'odd-view'])
@pytest.mark.parametrize('size', NV12_SIZES, ids=ids)
def test_nv12_equals_to_bgr(ctx, torch, size, view):
    w, h = size
    rng = np.random.default_rng(w * 139 + h + view)
    configure(ctx, w, h)
    for matrix in ('bt601', 'bt709'):
        f, want = nv12_case(torch, ctx, rng, w, h, matrix, view)
        ctx.frame_upload(f)
        assert np.array_equal(ctx.frame_read(), want), matrix
    # one decoder surface: the UV plane right behind the Y plane, one pitch
    pitch = w + 10
    y, uv = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
    surf = torch.zeros((h + h // 2, pitch), dtype=torch.uint8, device=torch.device('cuda', ctx.device))
    surf[:h, :w] = torch.from_numpy(y).to(surf.device)
    surf[h:, :w] = torch.from_numpy(uv).to(surf.device)
    ctx.frame_upload(DeviceArrayFrame.nv12(surf[:h, :w], surf[h:, :w]))
    assert np.array_equal(ctx.frame_read(), D.to_bgr((y, uv)))


def test_every_float16_value_on_the_device(ctx, torch):
    """All 65536 bit patterns through the kernel, with both scales: the device's conversion, multiply and rounding are
    numpy's."""
    x = np.arange(65536, dtype=np.uint16).view(np.float16).reshape(1, 64, 1024).repeat(3, axis=0)
    configure(ctx, 1024, 64)
    for fr in ((0, 1), (0, 255)):
        ctx.frame_upload(DeviceArrayFrame(on_device(torch, ctx, x, False), 'bgr', fr))
        assert np.array_equal(ctx.frame_read(), D.to_bgr(x, 'bgr', fr)), fr


# ---- 2. entry points
@pytest.mark.parametrize('size', [(34, 18), (130, 6)], ids=ids)
def test_other_entry_points(ctx, torch, size):
    w, h = size
    rng = np.random.default_rng(w * 137 + h)
    configure(ctx, w, h, 2)
    for view in (False, True):
        kinds = four_kinds(torch, ctx, rng, w, h, view)
        for (na, a, want_a), (nb, b, want_b) in zip(kinds, kinds[1:] + kinds[:1]):
            ctx.frame_upload(a)
            assert np.array_equal(ctx.frame_read(), want_a), (na, 'upload')
            ctx.frame_upload_ahead(1, a)
            ctx.frame_upload_ahead(2, b)
            for name, want in ((na, want_a), (nb, want_b)):
                ctx.frame_promote_next()
                assert np.array_equal(ctx.frame_read(), want), (name, 'ahead')
            ctx.frame_upload_next(b)
            ctx.frame_promote_next()
            assert np.array_equal(ctx.frame_read(), want_b), (nb, 'next')
            ctx.frame_ring_store(1, b)
            ctx.frame_ring_store(0, a)
            for k, (name, want) in enumerate(((na, want_a), (nb, want_b))):
                ctx.frame_ring_select(k)
                assert np.array_equal(ctx.frame_read(), want), (name, 'ring', k)
            assert a.wait().done() and b.wait().done()
    assert ctx.pending_device_frames() == []


def test_a_slot_alternates_between_host_and_device_frames(ctx, torch):
    w, h = 34, 18
    rng = np.random.default_rng(11)
    configure(ctx, w, h)
    host = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(3)]
    nv = NV12Frame(*bgr_to_nv12(host[1]))
    def through(k, frame):
        """The current frame after `frame` went through look-ahead slot k (the slots below it filled with a host frame)."""
        for j in range(1, k):
            ctx.frame_upload_ahead(j, host[2])
        ctx.frame_upload_ahead(k, frame)
        for _ in range(k):
            ctx.frame_promote_next()
        return ctx.frame_read()

    for name, f, want in four_kinds(torch, ctx, rng, w, h):
        for k in (1, 2):
            assert np.array_equal(through(k, host[0]), host[0]), (name, k, 'host first')
            assert np.array_equal(through(k, f), want), (name, k, 'device after host')
            assert np.array_equal(through(k, nv), D.to_bgr((nv.y, nv.uv))), (name, k, 'host after device')
            assert np.array_equal(through(k, f), want), (name, k, 'device again')
        ctx.frame_upload(f)
        ctx.frame_upload(host[2])
        assert np.array_equal(ctx.frame_read(), host[2])
        ctx.frame_upload(f)
        assert np.array_equal(ctx.frame_read(), want)


# ---- 3. off size
@pytest.mark.parametrize('src,dst', [((40, 24), (20, 12)), ((37, 21), (34, 18))], ids=['exact2x', 'linear'])
def test_source_frame_of_another_size(ctx, torch, src, dst):
    rng = np.random.default_rng(src[0])
    configure(ctx, dst[0], dst[1], 1)
    w, h = src
    for view in (False, True):
        cases = [('hwc', *hwc_case(torch, ctx, rng, w, h, 'rgb', view)), ('hwc4', *hwc_case(torch, ctx, rng, w, h, 'xbgr', view)),
                 ('chw-u8', *chw_case(torch, ctx, rng, w, h, 'uint8', 'bgr', (0, 1), view)),
                 ('chw-f16', *chw_case(torch, ctx, rng, w, h, 'float16', 'rgb', (0, 255), view)),
                 ('chw-f32', *chw_case(torch, ctx, rng, w, h, 'float32', 'rgb', (0, 1), view))]
        if not (w | h) & 1:
            cases.append(('nv12', *nv12_case(torch, ctx, rng, w, h, 'bt601', view)))
        for name, f, bgr in cases:
            want = resize_bgr(bgr, dst)
            ctx.frame_upload(SourceFrame(f))
            assert np.array_equal(ctx.frame_read(), want), (name, 'upload')
            for k in (1, 2):
                ctx.frame_upload_ahead(k, SourceFrame(f))
            for k in (1, 2):
                ctx.frame_promote_next()
                assert np.array_equal(ctx.frame_read(), want), (name, 'ahead', k)
            ctx.frame_ring_store(0, SourceFrame(f))
            ctx.frame_ring_select(0)
            assert np.array_equal(ctx.frame_read(), want), (name, 'ring')
    with pytest.raises(ValueError):                              # a bare frame of another size is not resized silently
        ctx.frame_upload(f)
    on_size, want = hwc_case(torch, ctx, rng, dst[0], dst[1], 'bgrx', False)
    ctx.frame_upload(SourceFrame(on_size))                       # a SourceFrame of the configured size is the plain upload
    assert np.array_equal(ctx.frame_read(), want)


def test_source_frame_with_a_lens_map(ctx, torch):
    src, dst = (37, 29), (64, 48)
    rng = np.random.default_rng(9)
    lens = LensMap.from_arrays(rng.uniform(-2., src[0] + 1., dst[::-1]), rng.uniform(-2., src[1] + 1., dst[::-1]), src, (7, 130, 255))
    configure(ctx, dst[0], dst[1], 1)
    try:
        for view in (False, True):
            for name, f, bgr in (('hwc', *hwc_case(torch, ctx, rng, src[0], src[1], 'rgb', view)),
                                 ('chw-f32', *chw_case(torch, ctx, rng, src[0], src[1], 'float32', 'rgb', (0, 1), view))):
                want = remap_bgr(bgr, lens)
                ctx.frame_upload(SourceFrame(f, lens=lens))
                assert np.array_equal(ctx.frame_read(), want), (name, 'upload')
                ctx.frame_upload_ahead(1, SourceFrame(f, lens=lens))
                ctx.frame_promote_next()
                assert np.array_equal(ctx.frame_read(), want), (name, 'ahead')
                ctx.frame_ring_store(0, SourceFrame(f, lens=lens))
                ctx.frame_ring_select(0)
                assert np.array_equal(ctx.frame_read(), want), (name, 'ring')
    finally:
        ctx.frame_set_lens(None)


# ---- 4. producer ordering
def busy(torch, dev, stream, ms=40):
    """Queues work of a few tens of milliseconds on `stream`: passes over a 1 GiB tensor (2 GiB of traffic each, a
    fraction of a millisecond at HBM rate)."""
    with torch.cuda.stream(stream):
        big = torch.zeros(1 << 28, dtype=torch.float32, device=dev)
        for _ in range(3 * ms):
            big.add_(1.0)
    return big


@pytest.mark.parametrize('ready', [False, True], ids=['stream', 'ready'])
def test_the_conversion_waits_for_the_producer(ctx, torch, ready):
    w, h = 130, 6
    rng = np.random.default_rng(21)
    configure(ctx, w, h)
    dev = torch.device('cuda', ctx.device)
    final = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    final_dev = torch.from_numpy(final).to(dev)
    t = torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(device=dev)
    big = busy(torch, dev, side)
    with torch.cuda.stream(side):
        t.copy_(final_dev)                                       # behind the queued work: not there yet
    if ready:
        side.synchronize()
        f = DeviceArrayFrame(t, 'bgr', ready=True)
    else:
        assert not side.query()                                  # the work is still running: the hand-over races it
        f = DeviceArrayFrame(t, 'bgr', stream=side.cuda_stream)
    ctx.frame_upload_ahead(1, f)
    ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), final)
    assert f.wait().done()
    # the synchronous entry point orders itself the same way
    t.zero_()
    torch.cuda.synchronize(dev)
    big = busy(torch, dev, side, 10)
    with torch.cuda.stream(side):
        t.copy_(final_dev)
    if ready:
        side.synchronize()
    ctx.frame_upload(DeviceArrayFrame(t, 'bgr', stream=side.cuda_stream, ready=ready))
    assert np.array_equal(ctx.frame_read(), final)
    del big


# ---- 5. lifetime
def test_the_context_keeps_the_source_alive(ctx, torch):
    w, h = 256, 64
    rng = np.random.default_rng(23)
    configure(ctx, w, h)
    dev = torch.device('cuda', ctx.device)
    host = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    side = torch.cuda.Stream(device=dev)
    for keep_frame in (False, True):
        t = torch.from_numpy(host).to(dev)
        ptr = t.data_ptr()
        torch.cuda.synchronize(dev)
        big = busy(torch, dev, side)                             # the conversion is held back behind this ...
        f = DeviceArrayFrame(t, 'rgbx', stream=side.cuda_stream)
        ctx.frame_upload_ahead(1, f)
        assert not f.done() and ctx.pending_device_frames() == [f]
        del t                                                    # ... while the caller lets go of the tensor
        if not keep_frame:
            del f
        gc.collect()
        # the caching allocator would hand the block to the first of these had it been released
        others = [torch.full((h, w, 4), 255 - i, dtype=torch.uint8, device=dev) for i in range(8)]
        assert all(o.data_ptr() != ptr for o in others)
        ctx.frame_promote_next()
        assert np.array_equal(ctx.frame_read(), D.to_bgr(host, 'rgbx'))
        if keep_frame:
            assert f.wait().done()
            assert ctx.pending_device_frames() == []
        else:
            ctx.frame_upload(host[..., :3].copy())               # any later frame call prunes
            assert ctx._dev_pending == []
        del big, others


def test_old_tickets_are_consumed(ctx, torch):
    w, h = 34, 18
    rng = np.random.default_rng(29)
    configure(ctx, w, h)
    frames = [hwc_case(torch, ctx, rng, w, h, 'rgb', False) for _ in range(20)]
    lib, tickets = ctx.lib, []
    for f, _ in frames:                                          # more than FM_DEV_TICKETS of them
        t = C.c_uint64(0)
        assert lib.fm_frame_upload_ahead_device(ctx.handle, C.c_int(1), C.byref(f.descriptor()), C.byref(t)) == 0
        tickets.append(t.value)
    assert tickets == list(range(tickets[0], tickets[0] + 20))
    ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), frames[-1][1])
    for t in tickets:
        assert lib.fm_frame_device_done(ctx.handle, C.c_uint64(t), C.c_int(1)) == 1
        assert lib.fm_frame_device_done(ctx.handle, C.c_uint64(t), C.c_int(0)) == 1
    for t in (0, tickets[-1] + 1):
        assert lib.fm_frame_device_done(ctx.handle, C.c_uint64(t), C.c_int(0)) == FM_ERR_ARG


# ---- 6. refusals
class Claims:
    """An object that claims, through __cuda_array_interface__, memory it may not have."""

    def __init__(self, ptr, shape, typestr='|u1', strides=None, keep=None):
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), strides=strides, version=2)
        self.keep = keep


def test_refusals(ctx, torch):
    lib = ctx.lib
    w, h = 64, 16
    configure(ctx, w, h, 1)
    dev = torch.device('cuda', ctx.device)
    rng = np.random.default_rng(3)
    before = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    ctx.frame_upload(before)
    ctx.frame_ring_store(0, before)
    host = np.zeros((h, w, 3), np.uint8)
    pinned = _lib.pinned_empty(lib, (h, w, 3), np.uint8)
    small = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)              # 3 KiB of a 2 MiB block at most
    f32 = torch.zeros((3 * h * w + 4,), dtype=torch.float32, device=dev)
    y, uv = torch.zeros((h, w), dtype=torch.uint8, device=dev), torch.zeros((h // 2, w), dtype=torch.uint8, device=dev)
    refused = {
        'a numpy array\'s address': DeviceArrayFrame(Claims(host.ctypes.data, (h, w, 3), keep=host)),
        'page-locked host memory': DeviceArrayFrame(Claims(pinned.ctypes.data, (h, w, 3), keep=pinned)),
        # 16384 rows of 192 bytes are 3 MiB: past the end of whatever block the allocator put the tensor in
        'an extent past its allocation': SourceFrame(DeviceArrayFrame(Claims(small.data_ptr(), (16384, w, 3), keep=small))),
        'a pitch past its allocation': DeviceArrayFrame(Claims(small.data_ptr(), (h, w, 3), strides=(1 << 22, 3, 1), keep=small)),
    }
    for name, f in refused.items():
        for call in (lambda: ctx.frame_upload(f), lambda: ctx.frame_upload_ahead(1, f), lambda: ctx.frame_ring_store(0, f)):
            with pytest.raises(ValueError, match='device frame refused'):
                call()
            assert b'bad argument' in lib.fm_last_error(), name
    assert b'runs past its allocation' in lib.fm_last_error()
    with pytest.raises(ValueError, match='fm_frame_upload'):                     # the message names the host calls
        ctx.frame_upload(refused['a numpy array\'s address'])
    # what the description itself gives away never reaches the library
    with pytest.raises(ValueError):                                              # misaligned float32
        DeviceArrayFrame(Claims(f32.data_ptr() + 2, (3, h, w), '<f4', keep=f32))
    with pytest.raises(ValueError):                                              # odd NV12 dims
        DeviceArrayFrame.nv12(Claims(y.data_ptr(), (h - 1, w)), Claims(uv.data_ptr(), ((h - 1) // 2, w)))
    # ... and the library refuses the same two by itself
    good32 = DeviceArrayFrame(f32[:3 * h * w].view(3, h, w))
    d = D.FrameDevice.from_buffer_copy(good32.descriptor())
    d.plane[1] = d.plane[1] + 2
    odd = D.FrameDevice.from_buffer_copy(DeviceArrayFrame.nv12(y, uv).descriptor())
    odd.height = h - 1
    for desc in (d, odd):
        for rc in (lib.fm_frame_upload_device(ctx.handle, C.byref(desc)),
                   lib.fm_frame_upload_ahead_device(ctx.handle, C.c_int(1), C.byref(desc), None),
                   lib.fm_frame_ring_store_device(ctx.handle, C.c_int(0), C.byref(desc))):
            assert rc == FM_ERR_ARG and b'bad argument' in lib.fm_last_error()
    # a size other than the map's while a lens is set
    lens = LensMap.from_arrays(*np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)), (w, h))
    other = DeviceArrayFrame(torch.zeros((h + 2, w, 3), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        SourceFrame(other, lens=lens)
    ctx.frame_set_lens(lens)
    try:
        for rc in (lib.fm_frame_upload_device(ctx.handle, C.byref(other.descriptor())),
                   lib.fm_frame_upload_ahead_device(ctx.handle, C.c_int(1), C.byref(other.descriptor()), None),
                   lib.fm_frame_ring_store_device(ctx.handle, C.c_int(0), C.byref(other.descriptor()))):
            assert rc == FM_ERR_ARG and b'remap_takes' in lib.fm_last_error()
        wrapped = SourceFrame(DeviceArrayFrame(torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)), lens=lens)
        wrapped.frame = other                                    # (what SourceFrame's own check keeps from happening)
        with pytest.raises(ValueError, match='device frame refused'):
            ctx.frame_upload(wrapped)
    finally:
        ctx.frame_set_lens(None)
    # nothing was launched: no frame in slot 1, the current frame and the ring as they were, nothing pending
    with pytest.raises(_lib.FastMOTHipError):
        ctx.frame_promote_next()
    assert np.array_equal(ctx.frame_read(), before)
    ctx.frame_ring_select(0)
    assert np.array_equal(ctx.frame_read(), before)
    assert ctx.pending_device_frames() == []
    # the same memory, described truthfully, is accepted
    ctx.frame_upload(DeviceArrayFrame(small, 'bgr'))
    ctx.frame_upload(good32)
    ctx.frame_upload(DeviceArrayFrame.nv12(y, uv))
    assert np.array_equal(ctx.frame_read(), D.to_bgr((np.zeros((h, w), np.uint8), np.zeros((h // 2, w), np.uint8))))


# ---- 7. tracking
SIZE = (960, 540)          # the smallest size the MOT tests run the tracker at


def run_mot(video, frames):
    from fastmot_amd import Track
    from test_mot_gpu import build_mot
    mot = build_mot(SIZE, video, 1)
    Track._count = 0
    mot.reset(1 / 30.)
    rows, jpegs = [], []
    try:
        for i, frame in enumerate(frames):
            mot.detector._frame_idx = i
            mot.step(frame, next_frame=frames[i + 1] if i + 1 < len(frames) else None)
            rows.append([(t.trk_id, tuple(t.tlbr), t.confirmed, t.active, t.age, t.hits) for t in mot.tracker.tracks.values()])
            if i in (0, len(frames) - 1):
                jpegs.append(mot.encode_frame())
    finally:
        mot.tracker._clear_tracks()
    return rows, jpegs


def test_tracks_on_device_frames_equal_host_frames(ctx, torch):
    from synthetic import SyntheticVideo
    video = SyntheticVideo(SIZE, n_ids=8, n_frames=8, seed=4)
    dev = torch.device('cuda', ctx.device)
    bgr = [np.ascontiguousarray(f) for f in video.frames]
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    want = run_mot(video, bgr)
    assert len(want[0][-1]) >= 6 and len(want[1]) == 2
    hwc = [DeviceArrayFrame(put(f), 'bgr') for f in bgr]
    assert run_mot(video, hwc) == want
    chw = [DeviceArrayFrame(put(f[..., ::-1].transpose(2, 0, 1)), 'rgb') for f in bgr]
    assert run_mot(video, chw) == want
    # k / 255 in float16 is k / 255 (1 + e), |e| <= 2^-11: times 255, within 0.07 of k
    f16 = [DeviceArrayFrame(put((f[..., ::-1].transpose(2, 0, 1) / 255.).astype(np.float16)), 'rgb', (0, 1)) for f in bgr]
    assert run_mot(video, f16) == want
    nv12 = [bgr_to_nv12(f) for f in bgr]
    got = run_mot(video, [DeviceArrayFrame.nv12(put(y), put(uv)) for y, uv in nv12])
    assert got == run_mot(video, [NV12Frame(y, uv) for y, uv in nv12])
    assert ctx.pending_device_frames() == []


def test_draw_refuses_device_frames(ctx, torch):
    from synthetic import SyntheticVideo
    from test_mot_gpu import build_mot
    video = SyntheticVideo(SIZE, n_ids=2, n_frames=1, seed=4)
    mot = build_mot(SIZE, video, 1)
    mot.draw = True
    mot.reset(1 / 30.)
    try:
        with pytest.raises(TypeError):
            mot.step(DeviceArrayFrame(torch.from_numpy(np.ascontiguousarray(video.frames[0])).to(torch.device('cuda', ctx.device)), 'bgr'))
    finally:
        mot.tracker._clear_tracks()
