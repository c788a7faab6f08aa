"""CPU: the 27 frame-ingest entry points (csrc/frames.hip: 9 families x upload, upload-ahead and ring-store) refuse a
null context, and a null description where they take one, before any HIP call -- this runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

from fastmot_amd import BayerFrame, DeepFrame, DeviceArrayFrame, PackedFrame, PlanarFrame, SourceFrame, _lib
from fastmot_amd.utils.jpeg import JpegInfo

FM_ERR_ARG = -2
PTR = 0x7f0000100000          # an address no test dereferences


class FakeDeviceArray:
    __cuda_array_interface__ = dict(shape=(6, 8, 3), typestr='|u1', data=(PTR, False), strides=None, version=2)


def _u8(*shape):
    return np.zeros(shape, np.uint8)


def _families():
    """suffix -> the argument lists to try behind the context (and k / index): the valid one first, then -- for a family
    that takes a description -- the null one.  The arrays and structures live as long as the returned dict."""
    keep = [_u8(4, 6, 3), _u8(4, 6), _u8(2, 6), np.zeros(64, np.int16), np.zeros(192, np.uint16), JpegInfo(),
            SourceFrame(_u8(5, 7, 3)).describe(), PlanarFrame(_u8(4, 6), _u8(2, 3), _u8(2, 3)).describe(),
            PackedFrame(_u8(3, 5, 3), 'rgb').describe(), BayerFrame(_u8(4, 6), 'rggb').describe(),
            DeepFrame(np.zeros((4, 6), np.uint16), np.zeros((2, 3), np.uint16), np.zeros((2, 3), np.uint16)).describe(),
            DeviceArrayFrame(FakeDeviceArray()).descriptor()]
    bgr, y, uv, coef, qt, info, src, planar, packed, bayer, deep, device = keep
    p = _lib._ptr
    i = C.c_int
    described = {'_src': src, '_planar': planar, '_packed': packed, '_bayer': bayer, '_deep': deep, '_device': device}
    table = {'': [(p(bgr),), (None,)],
             '_nv12': [(p(y), p(uv), i(6), i(0)), (None, None, i(6), i(0))],
             '_jpeg': [(C.byref(info), p(coef), p(qt)), (None, p(coef), p(qt))]}
    table.update({suffix: [(C.byref(d),), (None,)] for suffix, d in described.items()})
    return table, keep


FAMILIES, _KEEP = _families()
STEMS = {'upload': (), 'upload_ahead': (C.c_int(1),), 'ring_store': (C.c_int(0),)}


def test_there_are_27_entry_points():
    assert len(FAMILIES) == 9 and len(STEMS) == 3
    lib = _lib.load()
    for suffix in FAMILIES:
        for stem in STEMS:
            assert hasattr(lib, f'fm_frame_{stem}{suffix}')


@pytest.mark.parametrize('stem', STEMS)
@pytest.mark.parametrize('suffix', FAMILIES, ids=lambda s: s.lstrip('_') or 'bgr')
def test_entry_point_refuses_null_arguments(suffix, stem):
    lib = _lib.load()
    fn = getattr(lib, f'fm_frame_{stem}{suffix}')
    ticket = C.c_uint64(77)
    tail = (C.byref(ticket),) if (stem, suffix) == ('upload_ahead', '_device') else ()
    for args in FAMILIES[suffix]:
        assert fn(None, *STEMS[stem], *args, *tail) == FM_ERR_ARG
        err = lib.fm_last_error()
        assert b'bad argument' in err and b'frames.hip' in err, err
    assert ticket.value == 77
