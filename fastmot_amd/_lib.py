"""ctypes binding of libfastmot_hip.so (include/fastmot_hip.h).

This is the ONLY native boundary of the package.  There is no CPU fallback: if the
shared library is missing or a call fails, an exception is raised (the reference raises
RuntimeError when its plugin/engine is missing, fastmot/utils/inference.py:50-63).
"""
import ctypes as C
import os
import sys
import weakref
from pathlib import Path

import numpy as np
from types import SimpleNamespace

from .utils.nv12 import NV12Frame
from .utils.jpeg import JPEGFrame, QT_ENTRIES, max_coefficients
from .utils.source import SourceFrame
from .utils.yuv import PlanarFrame, frame_bytes
from .utils.packed import PackedFrame, row_bytes
from .utils.bayer import BayerFrame
from .utils.deep import DeepFrame, deep_frame_bytes
from .utils.devarray import DeviceArrayFrame

LIB_PATH = Path(os.environ.get('FASTMOT_LIB_PATH', Path(__file__).parent / 'libfastmot_hip.so'))

c_int_p = C.POINTER(C.c_int)
_lib = None


class FastMOTHipError(RuntimeError):
    pass


class KFParams(C.Structure):
    _fields_ = [('dt', C.c_double),
                ('std_factor_acc', C.c_double), ('std_offset_acc', C.c_double),
                ('std_factor_det', C.c_double * 2), ('std_factor_klt', C.c_double * 2),
                ('min_std_det', C.c_double * 2), ('min_std_klt', C.c_double * 2),
                ('init_pos_weight', C.c_double), ('init_vel_weight', C.c_double),
                ('vel_coupling', C.c_double), ('vel_half_life', C.c_double)]


def load():
    """Loads the shared library once; raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(f'{LIB_PATH} not found: build it with `python -m fastmot_amd.build` '
                           '(hipcc --offload-arch=gfx950); there is no CPU fallback')
    try:
        lib = C.CDLL(str(LIB_PATH), mode=os.RTLD_NOW | os.RTLD_LOCAL)
    except OSError as err:
        raise RuntimeError(f'Unable to load {LIB_PATH}') from err
    lib.fm_last_error.restype = C.c_char_p
    lib.fm_jpeg_encode_bound.restype = C.c_size_t
    lib.fm_i420_bound.restype = C.c_size_t
    lib.fm_jpeg_encode_regions_bound.restype = C.c_size_t
    _lib = lib
    return lib


def _ptr(arr, ctype=None):
    """Raw data pointer of a C-contiguous array that the CALLER keeps alive for the duration of the call
    (`arr.ctypes.data_as` would hold a reference but costs 2.4 us per argument; ~60 arguments per frame)."""
    if arr is None:
        return None
    return C.c_void_p(arr.__array_interface__['data'][0])


def _as(arr, dtype, shape=None):
    out = np.ascontiguousarray(arr, dtype=dtype)
    if shape is not None:
        out = out.reshape(shape)
    return out


def check(rc):
    if rc != 0:
        raise FastMOTHipError(f'libfastmot_hip error {rc}: {load().fm_last_error().decode()}')


# fm_overlay_cmd (32 bytes): one primitive of an overlay command list (utils/overlay.py builds them)
OVERLAY_CMD_DTYPE = np.dtype([('kind', '<i4'), ('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4'),
                              ('color', 'u1', (3,)), ('thickness', 'u1'), ('mask_off', '<u4'), ('reserved', '<i4')])
assert OVERLAY_CMD_DTYPE.itemsize == 32
OVL_RECT_FILL, OVL_RECT_OUTLINE, OVL_LINE, OVL_DOT, OVL_MASK = range(5)
FM_OVERLAY_MAX_CMDS = 65536
FM_OVERLAY_MAX_MASK_BYTES = 4 << 20
FM_OVERLAY_MAX_COORD = 1 << 20


def _overlay_args(cmds, masks):
    cmds = np.ascontiguousarray(cmds, dtype=OVERLAY_CMD_DTYPE).reshape(-1)
    masks = np.frombuffer(bytes(masks), np.uint8) if not isinstance(masks, np.ndarray) else np.ascontiguousarray(masks, np.uint8).reshape(-1)
    return cmds, masks, (_ptr(cmds) if len(cmds) else None, C.c_int(len(cmds)), _ptr(masks) if len(masks) else None,
                         C.c_size_t(len(masks)))


def overlay_check(cmds, masks, width, height):
    """fm_overlay_check's return code (0: well formed) for a command list on a width x height frame."""
    cmds, masks, args = _overlay_args(cmds, masks)
    return load().fm_overlay_check(*args, C.c_int(width), C.c_int(height))


def overlay_render_host(frame, cmds, masks=b''):
    """Applies an overlay command list to host pixels [H, W, 3] uint8 BGR IN PLACE on the CPU, with the functions the kernel
    is compiled from (csrc/overlay_pixel.h).  No GPU."""
    if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3 or \
            frame.strides[1:] != (3, 1) or frame.strides[0] < 3 * frame.shape[1] or not frame.flags.writeable:
        raise ValueError('frame must be a writeable uint8 HxWx3 array with packed pixels')
    cmds, masks, args = _overlay_args(cmds, masks)
    check(load().fm_overlay_render_host(_ptr(frame), C.c_int(frame.shape[1]), C.c_int(frame.shape[0]), C.c_size_t(frame.strides[0]), *args))
    return frame


# fm_redact_region (32 bytes): one region of a redaction list (utils/redact.py builds them)
REDACT_REGION_DTYPE = np.dtype([('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4'), ('mode', '<i4'), ('shape', '<i4'),
                                ('cell', '<i4'), ('color', 'u1', (3,)), ('reserved', 'u1')])
assert REDACT_REGION_DTYPE.itemsize == 32
REDACT_PIXELATE, REDACT_SMOOTH, REDACT_FILL = range(3)
REDACT_RECT, REDACT_ELLIPSE = range(2)
FM_REDACT_MAX_REGIONS = 4096
FM_REDACT_MAX_CELLS = 1 << 20
FM_SRC_MAX_DIM = 16384


# fm_crop_rect / fm_crop_plan / fm_crop_totals: object crops as JPEG files, many in one pass (fm_frame_encode_regions)
CROP_RECT_DTYPE = np.dtype([('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4')])
CROP_PLAN_DTYPE = np.dtype([('width', '<i4'), ('height', '<i4'), ('mcus_x', '<i4'), ('mcus_y', '<i4'), ('first_mcu', '<i4'),
                            ('first_block', '<i4'), ('first_row', '<i4'), ('reserved', '<i4'), ('raw_offset', '<u8'), ('bound', '<u8')])
CROP_TOTALS_DTYPE = np.dtype([('mcus', '<i4'), ('blocks', '<i4'), ('rows', '<i4'), ('reserved', '<i4'), ('raw_bytes', '<u8'),
                              ('bound', '<u8')])
assert CROP_RECT_DTYPE.itemsize == 16 and CROP_PLAN_DTYPE.itemsize == 48 and CROP_TOTALS_DTYPE.itemsize == 32
FM_OBJENC_MAX_REGIONS = 1024
FM_OBJENC_MAX_MCUS = 16384
OBJENC_SHRINKS = (1, 2, 4)


def _crop_rects(rects):
    """An (n, 4) integer array of inclusive corners -> the C list."""
    arr = np.asarray(rects)
    if arr.size and not np.issubdtype(arr.dtype, np.integer):
        raise ValueError('rects must be integers')
    return np.ascontiguousarray(arr.reshape(-1, 4), dtype=np.int32)


def encode_regions_plan(rects, shrink=1):
    """fm_jpeg_encode_regions_plan: (plans, totals) of one call -- where every image lies in the launches' index spaces and
    how much its file can take; FastMOTHipError, naming the limit, for a list the library refuses.  No GPU."""
    arr = _crop_rects(rects)
    plans = np.zeros(len(arr), CROP_PLAN_DTYPE)
    totals = np.zeros(1, CROP_TOTALS_DTYPE)
    check(load().fm_jpeg_encode_regions_plan(_ptr(arr) if len(arr) else None, C.c_int(len(arr)), C.c_int(int(shrink)),
                                             _ptr(plans) if len(arr) else None, _ptr(totals)))
    return plans, totals[0]


def encode_regions_assemble(plans, quality, segments, capacity=None, segs_bytes=None):
    """fm_jpeg_encode_regions_assemble: the files of a call from the byte-stuffed segments of all its MCU rows (a list of
    bytes in row order) -> list of bytes.  No GPU."""
    plans = np.ascontiguousarray(plans, dtype=CROP_PLAN_DTYPE)
    lens = np.array([len(s) for s in segments], np.uint32)
    segs = np.zeros(max(sum((len(s) + 15) & ~15 for s in segments), 16), np.uint8)
    at = 0
    for s in segments:
        segs[at:at + len(s)] = np.frombuffer(s, np.uint8)
        at += (len(s) + 15) & ~15
    cap = int(plans['bound'].sum()) if capacity is None else capacity
    out = np.zeros(max(cap, 1), np.uint8)
    offsets = np.zeros(len(plans) + 1, np.uintp)
    check(load().fm_jpeg_encode_regions_assemble(_ptr(plans), C.c_int(len(plans)), C.c_int(int(quality)), _ptr(lens), _ptr(segs),
                                                 C.c_size_t(segs.size if segs_bytes is None else segs_bytes), _ptr(out), C.c_size_t(cap),
                                                 _ptr(offsets)))
    return [out[int(a):int(b)].tobytes() for a, b in zip(offsets[:-1], offsets[1:])]


def _redact_args(regions):
    regions = np.ascontiguousarray(regions, dtype=REDACT_REGION_DTYPE).reshape(-1)
    return regions, (_ptr(regions) if len(regions) else None, C.c_int(len(regions)))


def redact_check(regions, width, height):
    """fm_redact_check's return code (0: well formed) for a region list on a width x height frame."""
    regions, args = _redact_args(regions)
    return load().fm_redact_check(*args, C.c_int(width), C.c_int(height))


def redact_render_host(frame, regions):
    """Redacts host pixels [H, W, 3] uint8 BGR IN PLACE on the CPU by a region list, with the functions the kernels are
    compiled from (csrc/redact_pixel.h); every region reads the original pixels.  No GPU."""
    if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3 or \
            frame.strides[1:] != (3, 1) or frame.strides[0] < 3 * frame.shape[1] or not frame.flags.writeable:
        raise ValueError('frame must be a writeable uint8 HxWx3 array with packed pixels')
    regions, args = _redact_args(regions)
    check(load().fm_redact_render_host(_ptr(frame), C.c_int(frame.shape[1]), C.c_int(frame.shape[0]), C.c_size_t(frame.strides[0]), *args))
    return frame


def device_count():
    n = load().fm_device_count()
    if n < 0:
        raise FastMOTHipError(load().fm_last_error().decode())
    return n


def device_pci_bus_id(device):
    buf = C.create_string_buffer(64)
    check(load().fm_device_pci_bus_id(C.c_int(device), buf, C.c_int(64)))
    return buf.value.decode().lower()


class HipContext:
    """One context = one GPU = one video stream (fm_ctx)."""

    def __init__(self, device=0):
        self._dev_pending = []             # (DeviceArrayFrame, ticket) of the look-ahead uploads that may still read their source
        self.lib = load()
        self._ctx = C.c_void_p()
        check(self.lib.fm_ctx_create(C.c_int(device), C.byref(self._ctx)))
        self.device = device
        self.feat_dim = 512

    def close(self):
        if getattr(self, '_ctx', None) is not None and self._ctx:
            self.lib.fm_ctx_destroy(self._ctx)     # (waits for every device frame that is still being read)
            self._ctx = C.c_void_p()
        for frame, _ in self._dev_pending:
            frame._pending = [(ref, t) for ref, t in frame._pending if ref() is not self]
        self._dev_pending = []

    def __del__(self):
        # at interpreter shutdown the HIP runtime may already be gone: the orderly path is the atexit hook
        # registered by runtime.get_context(), which runs while the runtime is still alive
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._ctx

    def synchronize(self):
        check(self.lib.fm_ctx_synchronize(self._ctx))

    def set_option(self, key, value):
        """Tunables of the context: 'zero_copy_tracks', 'host_lap_elems' (include/fastmot_hip.h)."""
        check(self.lib.fm_ctx_set_option(self._ctx, key.encode(), C.c_int(int(value))))

    def get_option(self, key):
        """The front-ahead options 'det_front_ahead', 'det_front_layers', 'det_front_stream' as they stand."""
        v = C.c_int(0)
        check(self.lib.fm_ctx_get_option(self._ctx, key.encode(), C.byref(v)))
        return v.value

    def front_info(self):
        """-> (cut, bytes, passes): the detector network's front-ahead cut as prepared (0: none), the device memory it
        costs, and the number of passes that ran a front so far (fm_net_front_info)."""
        k, b, n = C.c_int(0), C.c_longlong(0), C.c_longlong(0)
        check(self.lib.fm_net_front_info(self._ctx, C.byref(k), C.byref(b), C.byref(n)))
        return k.value, b.value, n.value

    def trace_start(self, cap=20000):
        """Arms the library's stage-boundary event trace; -> host CLOCK_MONOTONIC ns of the trace's zero."""
        t0 = C.c_int64(0)
        check(self.lib.fm_trace_start(self._ctx, C.c_int(cap), C.byref(t0)))
        self._trace_cap = cap
        return t0.value

    def trace_read(self):
        """-> (tags int32[n], ms float32[n]): GPU time of every recorded stage boundary since the trace's zero."""
        cap = self._trace_cap
        tags = np.zeros(cap, np.int32)
        ms = np.zeros(cap, np.float32)
        n = C.c_int(0)
        check(self.lib.fm_trace_read(self._ctx, C.c_int(cap), _ptr(tags), _ptr(ms), C.byref(n)))
        return tags[:n.value], ms[:n.value]

    def bind_thread(self):
        """Called once by every additional host thread that drives this context."""
        check(self.lib.fm_ctx_bind_thread(self._ctx))

    def device_info(self):
        buf = C.create_string_buffer(256)
        check(self.lib.fm_device_info(self._ctx, buf, 256))
        # gcnArchName itself contains ':' (gfx950:sramecc+:xnack-) -> parse from the right
        parts = buf.value.decode().split(':')
        return {'name': parts[0], 'arch': ':'.join(parts[1:-3]), 'cus': int(parts[-3]),
                'clock_mhz': int(parts[-2]), 'hbm_bytes': int(parts[-1])}

    # ------------------------------------------------------------------ Kalman
    def kf_configure(self, dt, std_factor_acc, std_offset_acc, std_factor_det, std_factor_klt,
                     min_std_det, min_std_klt, init_pos_weight, init_vel_weight, vel_coupling,
                     vel_half_life):
        p = KFParams(dt, std_factor_acc, std_offset_acc, (C.c_double * 2)(*std_factor_det),
                     (C.c_double * 2)(*std_factor_klt), (C.c_double * 2)(*min_std_det),
                     (C.c_double * 2)(*min_std_klt), init_pos_weight, init_vel_weight, vel_coupling,
                     vel_half_life)
        check(self.lib.fm_kf_configure(self._ctx, C.byref(p)))

    def set_frame_rect(self, tlbr):
        a = _as(tlbr, np.float64, (4,))
        check(self.lib.fm_set_frame_rect(self._ctx, _ptr(a)))

    def trk_create(self, slots, det_tlbr):
        s = _as(slots, np.int32)
        b = _as(det_tlbr, np.float64, (-1, 4))
        assert len(s) == len(b)
        check(self.lib.fm_trk_create(self._ctx, C.c_int(len(s)), _ptr(s), _ptr(b)))

    def trk_step(self, slots, H, klt_tlbr, has_klt, mult):
        s = _as(slots, np.int32)
        n = len(s)
        Hm = _as(H, np.float64, (9,))
        k = _as(klt_tlbr, np.float64, (-1, 4)) if n else np.zeros((0, 4))
        hk = _as(has_klt, np.uint8)
        mu = _as(mult, np.float64)
        assert len(k) == n and len(hk) == n and len(mu) == n
        tlbr = np.empty((n, 4), np.float64)
        lost = np.empty(n, np.uint8)
        check(self.lib.fm_trk_step(self._ctx, C.c_int(n), _ptr(s), _ptr(Hm), _ptr(k), _ptr(hk),
                                   _ptr(mu), _ptr(tlbr), _ptr(lost)))
        return tlbr, lost.astype(bool)

    def trk_step_ops(self, ops, slots, H, klt_tlbr, has_klt, mult):
        s = _as(slots, np.int32)
        n = len(s)
        Hm = _as(H, np.float64, (9,))
        k = _as(klt_tlbr, np.float64, (-1, 4)) if n else np.zeros((0, 4))
        hk = _as(has_klt, np.uint8)
        mu = _as(mult, np.float64)
        tlbr = np.empty((n, 4), np.float64)
        lost = np.empty(n, np.uint8)
        check(self.lib.fm_trk_step_ops(self._ctx, C.c_int(ops), C.c_int(n), _ptr(s), _ptr(Hm), _ptr(k),
                                       _ptr(hk), _ptr(mu), _ptr(tlbr), _ptr(lost)))
        return tlbr, lost.astype(bool)

    def trk_update_det(self, slots, det_tlbr):
        s = _as(slots, np.int32)
        n = len(s)
        b = _as(det_tlbr, np.float64, (-1, 4)) if n else np.zeros((0, 4))
        assert len(b) == n
        tlbr = np.empty((n, 4), np.float64)
        lost = np.empty(n, np.uint8)
        check(self.lib.fm_trk_update_det(self._ctx, C.c_int(n), _ptr(s), _ptr(b), _ptr(tlbr), _ptr(lost)))
        return tlbr, lost.astype(bool)

    def trk_get_state(self, slots):
        s = _as(slots, np.int32)
        mean = np.empty((len(s), 8), np.float64)
        cov = np.empty((len(s), 8, 8), np.float64)
        check(self.lib.fm_trk_get_state(self._ctx, C.c_int(len(s)), _ptr(s), _ptr(mean), _ptr(cov)))
        return mean, cov

    def trk_set_state(self, slots, mean, cov):
        s = _as(slots, np.int32)
        m = _as(mean, np.float64, (-1, 8))
        c = _as(cov, np.float64, (-1, 8, 8))
        assert len(m) == len(s) and len(c) == len(s)
        check(self.lib.fm_trk_set_state(self._ctx, C.c_int(len(s)), _ptr(s), _ptr(m), _ptr(c)))

    def trk_copy_state(self, dst, src):
        check(self.lib.fm_trk_copy_state(self._ctx, C.c_int(dst), C.c_int(src)))

    # ------------------------------------------------------------------ features
    def feat_configure(self, dim):
        check(self.lib.fm_feat_configure(self._ctx, C.c_int(dim)))
        self.feat_dim = dim

    def emb_upload(self, emb):
        if emb is None:
            raise ValueError('emb is None; use emb_use_device(n)')
        e = _as(emb, np.float32)
        if e.ndim != 2 or (len(e) and e.shape[1] != self.feat_dim):
            raise ValueError('embeddings must be [n][feat_dim]')
        check(self.lib.fm_emb_upload(self._ctx, C.c_int(len(e)), _ptr(e)))

    def emb_use_device(self, n):
        check(self.lib.fm_emb_upload(self._ctx, C.c_int(n), None))

    def feat_update(self, slots, emb_rows):
        s = _as(slots, np.int32)
        r = _as(emb_rows, np.int32)
        assert len(s) == len(r)
        check(self.lib.fm_feat_update(self._ctx, C.c_int(len(s)), _ptr(s), _ptr(r)))

    def feat_merge(self, dst, src):
        check(self.lib.fm_feat_merge(self._ctx, C.c_int(dst), C.c_int(src)))

    def feat_reset(self, slots):
        s = _as(slots, np.int32)
        check(self.lib.fm_feat_reset(self._ctx, C.c_int(len(s)), _ptr(s)))

    def feat_get(self, slot):
        fsum = np.empty(self.feat_dim, np.float32)
        avg = np.empty(self.feat_dim, np.float32)
        cnt = C.c_int32(0)
        check(self.lib.fm_feat_get(self._ctx, C.c_int(slot), _ptr(fsum), _ptr(avg), C.byref(cnt)))
        return fsum, avg, cnt.value

    def feat_read(self, slots):
        s = _as(slots, np.int32)
        avg = np.empty((len(s), self.feat_dim), np.float32)
        cnt = np.zeros(len(s), np.int32)
        check(self.lib.fm_feat_read(self._ctx, C.c_int(len(s)), _ptr(s), _ptr(avg), _ptr(cnt)))
        return avg, cnt

    def feat_write(self, slots, avg, count):
        s = _as(slots, np.int32)
        a = _as(avg, np.float32).reshape(len(s), self.feat_dim)
        c = _as(count, np.int32)
        check(self.lib.fm_feat_write(self._ctx, C.c_int(len(s)), _ptr(s), _ptr(a), _ptr(c)))

    # ------------------------------------------------------------------ association
    def find_occluded(self, tlbr, thresh):
        b = _as(tlbr, np.float64, (-1, 4)) if len(tlbr) else np.zeros((0, 4))
        out = np.zeros(len(b), np.uint8)
        check(self.lib.fm_find_occluded(self._ctx, C.c_int(len(b)), _ptr(b), C.c_double(thresh), _ptr(out)))
        return out.astype(bool)

    def iou_dist(self, a, b):
        a = _as(a, np.float64, (-1, 4))
        b = _as(b, np.float64, (-1, 4))
        out = np.empty((len(a), len(b)), np.float64)
        check(self.lib.fm_iou_dist(self._ctx, C.c_int(len(a)), _ptr(a), C.c_int(len(b)), _ptr(b), _ptr(out)))
        return out

    def assoc_prepare(self, metric, slots, trk_tlbr, trk_label, det_tlbr, det_label, det_occluded,
                      trk_feat_f32=None, after_extractor=False):
        """All pairwise terms of this frame in one launch (fm_assoc_prepare2).  after_extractor: the embeddings are the
        batch extract_async enqueued last and may still be in flight (ordered on the device).  Returns True when the
        terms also reach page-locked host memory, i.e. `assoc_cascade` solves every stage on the host."""
        s = _as(slots, np.int32)
        nT = len(s)
        tb = _as(trk_tlbr, np.float64).reshape(nT, 4)
        tl = _as(trk_label, np.int64)
        db = _as(det_tlbr, np.float64).reshape(-1, 4)
        nD = len(db)
        dl = _as(det_label, np.int64)
        do = _as(det_occluded, np.uint8)
        f32 = np.zeros(nT, np.uint8) if trk_feat_f32 is None else _as(trk_feat_f32, np.uint8)
        assert len(tl) == nT and len(dl) == nD and len(do) == nD and len(f32) == nT
        host = C.c_int(0)
        check(self.lib.fm_assoc_prepare2(self._ctx, C.c_int(metric), C.c_int(nT), _ptr(s), _ptr(tb),
                                         _ptr(tl), C.c_int(nD), _ptr(db), _ptr(dl), _ptr(do), _ptr(f32),
                                         C.c_int(1 if after_extractor else 0), C.byref(host)))
        return bool(host.value)

    def cascade_pack(self, group_sizes, conf_rows, conf_active, unconf_rows, hist_rows, hist_labels, det_conf,
                     motion_weight, max_assoc_cost, fill_val, max_iou_cost, conf_thresh, max_reid_cost, per_stage=False):
        """Packs the arguments of `assoc_cascade` (fm_cascade_in); everything here is known before the embeddings are.
        per_stage: every stage the device way (FM_CASCADE_PER_STAGE) even where the terms reached the host."""
        off = np.zeros(len(group_sizes) + 1, np.int32)
        np.cumsum(group_sizes, out=off[1:])
        arrs = (off, _as(conf_rows, np.int32), _as(conf_active, np.uint8), _as(unconf_rows, np.int32),
                _as(hist_rows, np.int32), _as(hist_labels, np.int64), _as(det_conf, np.float64))
        cin = CascadeIn(len(group_sizes), len(arrs[3]), len(arrs[4]), CASCADE_PER_STAGE if per_stage else 0,
                        *(a.__array_interface__['data'][0] for a in arrs),
                        motion_weight, max_assoc_cost, fill_val, max_iou_cost, conf_thresh, max_reid_cost)
        n_trk = len(arrs[1]) + len(arrs[3])
        out = np.empty(CASCADE_HEADER + 3 * n_trk + 3 * len(arrs[6]), np.int32)
        return cin, arrs, out

    def assoc_cascade(self, pack):
        """The association cascade in one call (fm_assoc_cascade); returns the output words as a list."""
        cin, _, out = pack
        check(self.lib.fm_assoc_cascade(self._ctx, C.byref(cin), _ptr(out), C.c_int(len(out))))
        return out[:out[9]].tolist()

    def assoc_get_pairwise(self, nT, nD):
        feat = np.empty((nT, nD), np.float64)
        maha = np.empty((nT, nD), np.float64)
        iou = np.empty((nT, nD), np.float64)
        check(self.lib.fm_assoc_get_pairwise(self._ctx, _ptr(feat), _ptr(maha), _ptr(iou)))
        return feat, maha, iou

    def assoc_stage(self, stage, solver, rows, cols, motion_weight=0., max_cost=0., fill_val=1.,
                    row_labels=None, want_cost=False):
        r = _as(rows, np.int32)
        c = _as(cols, np.int32)
        nr, nc = len(r), len(c)
        mn = min(nr, nc)
        m_rows = np.empty(mn, np.int32)
        m_cols = np.empty(mn, np.int32)
        gated = np.zeros(mn, np.uint8)
        n_match = C.c_int(0)
        cost = np.empty((nr, nc), np.float64) if want_cost else None
        rl = _as(row_labels, np.int64) if row_labels is not None else None
        check(self.lib.fm_assoc_stage(self._ctx, C.c_int(stage), C.c_int(solver), C.c_int(nr), _ptr(r),
                                      C.c_int(nc), _ptr(c), C.c_double(motion_weight),
                                      C.c_double(max_cost), C.c_double(fill_val), _ptr(rl), _ptr(m_rows),
                                      _ptr(m_cols), _ptr(gated), C.byref(n_match), _ptr(cost)))
        k = n_match.value
        return m_rows[:k], m_cols[:k], gated[:k].astype(bool), cost

    def lap(self, cost):
        cm = _as(cost, np.float64)
        nr, nc = cm.shape
        mn = min(nr, nc)
        m_rows = np.empty(mn, np.int32)
        m_cols = np.empty(mn, np.int32)
        n_match = C.c_int(0)
        check(self.lib.fm_lap(self._ctx, _ptr(cm), C.c_int(nr), C.c_int(nc), _ptr(m_rows), _ptr(m_cols),
                              C.byref(n_match)))
        return m_rows[:n_match.value], m_cols[:n_match.value]

    def greedy(self, cost, max_cost):
        cm = _as(cost, np.float64)
        nr, nc = cm.shape
        mn = min(nr, nc)
        m_rows = np.empty(mn, np.int32)
        m_cols = np.empty(mn, np.int32)
        n_match = C.c_int(0)
        check(self.lib.fm_greedy(self._ctx, _ptr(cm), C.c_int(nr), C.c_int(nc), C.c_double(max_cost),
                                 _ptr(m_rows), _ptr(m_cols), C.byref(n_match)))
        return m_rows[:n_match.value], m_cols[:n_match.value]


CASCADE_HEADER = 16
CASCADE_PER_STAGE = 1          # fm_cascade_in.flags


class CascadeIn(C.Structure):          # fm_cascade_in
    _fields_ = [('n_groups', C.c_int32), ('n_unconf', C.c_int32), ('n_hist', C.c_int32), ('flags', C.c_int32),
                ('group_off', C.c_void_p), ('conf_rows', C.c_void_p), ('conf_active', C.c_void_p),
                ('unconf_rows', C.c_void_p), ('hist_rows', C.c_void_p), ('hist_labels', C.c_void_p),
                ('det_conf', C.c_void_p),
                ('motion_weight', C.c_double), ('max_assoc_cost', C.c_double), ('fill_val', C.c_double),
                ('max_iou_cost', C.c_double), ('conf_thresh', C.c_double), ('max_reid_cost', C.c_double)]


METRIC_EUCLIDEAN = 0
METRIC_COSINE = 1
STAGE_MATCHING = 0
STAGE_IOU = 1
STAGE_REID = 2
SOLVER_LAP = 0
SOLVER_GREEDY = 1


# ---------------------------------------------------------------------- detector / extractor
FM_MAX_HEADS, FM_MAX_ANCHORS = 4, 6
FM_EXPORT_FRAME, FM_EXPORT_OVERLAY = 0, 1     # fm_frame_export_i420's `which` (fastmot_hip.h)
FM_MAX_DET_BATCH = 4         # frames of one batched detector pass (fastmot_hip.h)


FM_MAX_SSD_TILES, FM_MAX_SSD_HEADS = 16, 6      # (fastmot_hip.h)


class SsdCfg(C.Structure):           # fm_ssd_cfg
    _fields_ = [('input_tensor', C.c_int32), ('in_w', C.c_int32), ('in_h', C.c_int32), ('n_heads', C.c_int32),
                ('head_tensor', C.c_int32 * FM_MAX_SSD_HEADS), ('map_w', C.c_int32 * FM_MAX_SSD_HEADS),
                ('map_h', C.c_int32 * FM_MAX_SSD_HEADS), ('n_anchors', C.c_int32 * FM_MAX_SSD_HEADS),
                ('anchors', C.c_void_p), ('n_anchor_rows', C.c_int32), ('box_scales', C.c_float * 4),
                ('num_classes', C.c_int32), ('topk', C.c_int32), ('nms_thresh', C.c_float), ('n_tiles', C.c_int32),
                ('tile_x', C.c_int32 * FM_MAX_SSD_TILES), ('tile_y', C.c_int32 * FM_MAX_SSD_TILES),
                ('region_w', C.c_int32), ('region_h', C.c_int32)]


class YoloCfg(C.Structure):
    _fields_ = [('in_w', C.c_int32), ('in_h', C.c_int32),
                ('roi_x', C.c_int32), ('roi_y', C.c_int32), ('roi_w', C.c_int32), ('roi_h', C.c_int32),
                ('input_tensor', C.c_int32), ('n_heads', C.c_int32),
                ('head_tensor', C.c_int32 * FM_MAX_HEADS),
                ('grid_w', C.c_int32 * FM_MAX_HEADS), ('grid_h', C.c_int32 * FM_MAX_HEADS),
                ('n_anchors', C.c_int32 * FM_MAX_HEADS),
                ('anchors', (C.c_float * (2 * FM_MAX_ANCHORS)) * FM_MAX_HEADS),
                ('scale_xy', C.c_float * FM_MAX_HEADS),
                ('num_classes', C.c_int32), ('new_coords', C.c_int32),
                ('label_mask', C.c_uint8 * 128),
                ('conf_thresh', C.c_double), ('nms_thresh', C.c_double), ('max_area', C.c_double),
                ('min_aspect_ratio', C.c_double),
                ('size', C.c_double * 2), ('offset', C.c_double * 2),
                ('max_candidates', C.c_int32)]


class DflHeads(C.Structure):
    """fm_dfl_heads: per level the box / class tensor ids with their first channels, and the level's stride."""
    _fields_ = [('n_levels', C.c_int32),
                ('box_tensor', C.c_int32 * FM_MAX_HEADS), ('box_coff', C.c_int32 * FM_MAX_HEADS),
                ('cls_tensor', C.c_int32 * FM_MAX_HEADS), ('cls_coff', C.c_int32 * FM_MAX_HEADS),
                ('stride', C.c_float * FM_MAX_HEADS)]


DET_DTYPE = np.dtype([('tlbr', float, 4), ('label', int), ('conf', float)], align=True)
assert DET_DTYPE.itemsize == 48


def merge_tiles(dets, tile_ids, n_tiles, thresh):
    """fm_detect_merge_tiles: the cross-tile merge of SSDDetector.merge_dets in the library (host code, no device call)."""
    d = np.ascontiguousarray(np.asarray(dets, DET_DTYPE))
    t = np.ascontiguousarray(np.asarray(tile_ids, np.int32))
    assert len(d) == len(t)
    out = np.zeros(max(len(d), 1), DET_DTYPE)
    n = C.c_int(0)
    check(load().fm_detect_merge_tiles(d.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), C.c_int(len(d)),
                                       C.c_int(int(n_tiles)), C.c_double(thresh), out.ctypes.data_as(C.c_void_p),
                                       C.byref(n)))
    return out[:n.value].view(np.recarray)


class _PinnedBlock:
    def __init__(self, lib, nbytes):
        self._lib = lib
        p = C.c_void_p()
        check(lib.fm_host_alloc(C.c_size_t(nbytes), C.byref(p)))
        self.ptr = p.value

    def __del__(self):
        if getattr(self, 'ptr', None):
            try:
                self._lib.fm_host_free(C.c_void_p(self.ptr))
            except Exception:
                pass
            self.ptr = None


def pinned_empty(lib, shape, dtype):
    """ndarray in page-locked host memory obtained from fm_host_alloc (freed with the array)."""
    dtype = np.dtype(dtype)
    nbytes = int(np.prod(shape)) * dtype.itemsize
    block = _PinnedBlock(lib, nbytes)
    buf = (C.c_uint8 * nbytes).from_address(block.ptr)
    buf._pinned_block = block              # keeps the allocation alive as long as any view exists
    return np.frombuffer(buf, dtype=dtype).reshape(shape)


def _bind_device_io(cls):
    def frame_configure(self, width, height, ring_size=0):
        check(self.lib.fm_frame_configure(self._ctx, C.c_int(width), C.c_int(height), C.c_int(ring_size)))
        self.frame_size = (width, height)
        self.ring_size = ring_size
        self._lens = None                  # (fm_frame_configure drops the map)

    def frame_set_lens(self, lens):
        """Sets the correction map of the described-source calls (a LensMap whose dst_size is the context's frame size),
        or none.  A per-stream setting: it synchronises the detector and ReID streams and uploads the map, so it may
        change but should not alternate per frame.  The SourceFrame branches of frame_upload / frame_upload_next /
        frame_upload_ahead / frame_ring_store call it when a frame carries another LensMap object than the one set."""
        if lens is None:
            check(self.lib.fm_frame_remap_clear(self._ctx))
            self._lens = None
            return
        if lens.dst_size != tuple(self.frame_size):
            raise ValueError(f'the lens map gives {lens.dst_size[0]}x{lens.dst_size[1]} frames, the context\'s are '
                             f'{self.frame_size[0]}x{self.frame_size[1]}')
        check(self.lib.fm_frame_remap_set(self._ctx, C.c_int(lens.src_size[0]), C.c_int(lens.src_size[1]), _ptr(lens.xy),
                                          (C.c_uint8 * 3)(*lens.border)))
        self._lens = lens

    def _described(self, frame):
        """Before a described-source call (fm_frame_*_src / _planar / _packed / _bayer / _deep) on `frame`: the context's map is
        the one the frame carries -- none for a frame that is not a SourceFrame."""
        lens = getattr(frame, 'lens', None)
        if lens is not getattr(self, '_lens', None):
            self.frame_set_lens(lens)

    def _nv12_args(self, frame):
        if frame.size != tuple(self.frame_size):
            raise ValueError(f'NV12 frame is {frame.size[0]}x{frame.size[1]}, the context\'s frames {self.frame_size[0]}x{self.frame_size[1]}')
        return _ptr(frame.y), _ptr(frame.uv), C.c_int(frame.pitch), C.c_int(frame.matrix_id)

    def _jpeg_args(self, frame):
        if frame.size != tuple(self.frame_size):
            raise ValueError(f'JPEG frame is {frame.size[0]}x{frame.size[1]}, the context\'s frames {self.frame_size[0]}x{self.frame_size[1]}')
        return C.byref(frame.info), _ptr(frame.coef), _ptr(frame.qt)

    def _frame_kind(self, frame):
        """The symbol suffix and the ctypes arguments of the fm_frame_* calls that take `frame`; ('', None) for everything
        else, which is a BGR ndarray's business.  A planar, packed, Bayer, deep or device frame is taken at the context's
        size, or inside a SourceFrame at any size (the call resizes it on the device).  The described kinds have the
        context's map set to the one the frame carries."""
        inner = frame.frame if isinstance(frame, SourceFrame) else frame
        for cls, suffix, name in ((DeviceArrayFrame, '_device', 'device'), (PlanarFrame, '_planar', 'planar'), (PackedFrame, '_packed', 'packed'),
                                  (BayerFrame, '_bayer', 'Bayer'), (DeepFrame, '_deep', 'deep')):
            if isinstance(inner, cls):
                if inner is frame and frame.size != tuple(self.frame_size):
                    raise ValueError(f'{name} frame is {frame.size[0]}x{frame.size[1]}, the context\'s frames '
                                     f'{self.frame_size[0]}x{self.frame_size[1]}: wrap it in a SourceFrame to have it resized')
                self._described(frame)
                return suffix, (C.byref(inner.descriptor() if cls is DeviceArrayFrame else inner.describe()),)
        if isinstance(frame, NV12Frame):
            return '_nv12', self._nv12_args(frame)
        if isinstance(frame, JPEGFrame):
            return '_jpeg', self._jpeg_args(frame)
        if isinstance(frame, SourceFrame):      # any size: resized to the frame size on the device (csrc/resize.hip)
            self._described(frame)
            return '_src', (C.byref(frame.describe()),)
        return '', None

    def _frame_call(self, stem, lead, frame):
        """fm_frame_<stem><the frame kind's suffix>(ctx, *lead, <the frame's arguments>): stem 'upload', 'upload_ahead' or
        'ring_store'."""
        self.device_frames_prune()
        suffix, args = self._frame_kind(frame)
        fn = getattr(self.lib, f'fm_frame_{stem}{suffix}')
        if suffix == '_device':
            if stem != 'upload_ahead':
                self._device_check(fn(self._ctx, *lead, *args))
                return
            dev = frame.frame if isinstance(frame, SourceFrame) else frame
            ticket = C.c_uint64(0)
            self._device_check(fn(self._ctx, *lead, *args, C.byref(ticket)))
            # the conversion runs behind this call: the frame (and the array it holds) stays referenced until it has run
            dev._pending.append((weakref.ref(self), ticket.value))
            self._dev_pending.append((dev, ticket.value))
            return
        if args is None:
            if stem == 'ring_store':            # (set-up work: converted, not checked)
                f = np.ascontiguousarray(frame, np.uint8)
            else:
                w, h = self.frame_size
                if frame.shape != (h, w, 3) or frame.dtype != np.uint8:
                    raise ValueError(f'frame must be uint8 {h}x{w}x3')
                f = np.ascontiguousarray(frame)
            args = (_ptr(f),)                   # (`f` lives until the call has returned)
        check(fn(self._ctx, *lead, *args))

    def _device_check(self, rc):
        """check() for the device-frame calls: a description the library refuses (FM_ERR_ARG: not device memory of this
        device, an extent past its allocation, a misaligned plane ...) is the caller's ValueError."""
        if rc == -2:
            raise ValueError(f'device frame refused: {self.lib.fm_last_error().decode()}')
        check(rc)

    def device_frame_done(self, ticket, wait=False):
        """fm_frame_device_done: the look-ahead upload `ticket` has finished reading its source (`wait`: block until then)."""
        if not self._ctx:
            return True                    # (close() waited for all of them)
        rc = self.lib.fm_frame_device_done(self._ctx, C.c_uint64(ticket), C.c_int(int(wait)))
        if rc < 0:
            check(rc)
        return rc == 1

    def device_frames_prune(self):
        """Drops the references to device frames whose memory has been read (every frame call does this first)."""
        if self._dev_pending:
            self._dev_pending = [(f, t) for f, t in self._dev_pending if not self.device_frame_done(t)]

    def pending_device_frames(self):
        """The DeviceArrayFrames this context still holds because an upload may be reading them, oldest first."""
        self.device_frames_prune()
        return [f for f, _ in self._dev_pending]

    def frame_upload(self, frame):
        self._frame_call('upload', (), frame)

    def pinned_frames(self, n):
        """n frames (n, H, W, 3) uint8 in page-locked host memory (fm_host_alloc): frames stored here are
        uploaded without a staging copy.  The buffer lives as long as the returned array's base object."""
        w, h = self.frame_size
        return pinned_empty(self.lib, (n, h, w, 3), np.uint8)

    def pinned_source_frames(self, n, size):
        """n BGR frames (n, H, W, 3) uint8 of the SOURCE size `size` = (W, H) in page-locked host memory (fm_host_alloc):
        `SourceFrame(buf[i])` is uploaded without a staging copy.  The buffer lives as long as the returned array's base object."""
        w, h = size
        if not (1 <= w <= 16384 and 1 <= h <= 16384):
            raise ValueError(f'source size {w}x{h} outside 1..16384')
        return pinned_empty(self.lib, (n, h, w, 3), np.uint8)

    def pinned_nv12_frames(self, n, matrix='bt601'):
        """n NV12Frames whose planes (pitch = width, UV behind Y) lie in page-locked host memory (fm_host_alloc): fill
        `f.y[...]` / `f.uv[...]`; they are uploaded without a staging copy.  The buffer lives as long as any of them."""
        w, h = self.frame_size
        buf = pinned_empty(self.lib, (n, h + h // 2, w), np.uint8)
        return [NV12Frame(buf[i, :h], buf[i, h:], matrix) for i in range(n)]

    def pinned_jpeg_buffers(self, n):
        """n int16 buffers in page-locked host memory (fm_host_alloc), each large enough for the coefficients and tables of
        any supported JPEG of the context's frame size: `JPEGFrame(data, buffer=b)` decodes into one, and the frame is
        uploaded without a staging copy.  The memory lives as long as any of them."""
        w, h = self.frame_size
        buf = pinned_empty(self.lib, (n, max_coefficients(w, h) + QT_ENTRIES), np.int16)
        return [buf[i] for i in range(n)]

    def pinned_planar_frames(self, n, chroma='420', matrix='bt601'):
        """n PlanarFrames of the context's frame size, each one contiguous Y, U, V surface in page-locked host memory
        (fm_host_alloc): fill `f.y[...]` / `f.u[...]` / `f.v[...]`; they are uploaded in one copy, without a staging copy.
        The buffer lives as long as any of them."""
        size = tuple(self.frame_size)
        buf = pinned_empty(self.lib, (n, frame_bytes(size, chroma)), np.uint8)
        return [PlanarFrame.from_buffer(buf[i], size, chroma, matrix) for i in range(n)]

    def pinned_packed_frames(self, n, fmt, matrix='bt601', size=None):
        """n PackedFrames of layout `fmt` and the context's frame size (or the SOURCE size `size` = (W, H), for
        `SourceFrame(f)`), each one surface with pitch = its row bytes in page-locked host memory (fm_host_alloc): fill
        `f.rows[...]`; they are uploaded without a staging copy.  The buffer lives as long as any of them."""
        w, h = tuple(self.frame_size) if size is None else size
        buf = pinned_empty(self.lib, (n, h, row_bytes(w, fmt)), np.uint8)
        return [PackedFrame(buf[i], fmt, (w, h), matrix) for i in range(n)]

    def pinned_bayer_frames(self, n, pattern, depth=8, size=None, method='mhc', wb=(1., 1., 1.), black=0):
        """n BayerFrames of the context's frame size (or the SOURCE size `size` = (W, H), for `SourceFrame(f)`), each one
        surface with pitch = its row bytes in page-locked host memory (fm_host_alloc): fill `f.rows[...]` (uint8 for
        depth 8, uint16 above); they are uploaded without a staging copy.  The buffer lives as long as any of them."""
        w, h = tuple(self.frame_size) if size is None else size
        if w < 2 or h < 2:
            raise ValueError(f'a mosaic is at least 2x2, not {w}x{h}')
        buf = pinned_empty(self.lib, (n, h, w), np.uint8 if depth == 8 else np.dtype('<u2'))
        return [BayerFrame(buf[i], pattern, (w, h), depth, method, wb, black) for i in range(n)]

    def pinned_deep_frames(self, n, chroma='420', depth=10, matrix='bt709', semiplanar=False):
        """n DeepFrames of the context's frame size, each one contiguous surface of 16-bit samples -- Y, U, V, or for
        `semiplanar` (P010 / P012 / P016; chroma '420') Y and interleaved UV -- in page-locked host memory (fm_host_alloc):
        fill `f.y[...]` and `f.u[...]` / `f.v[...]` (`f.uv[...]`); they are uploaded in one copy, without a staging copy.
        The buffer lives as long as any of them."""
        size = tuple(self.frame_size)
        if semiplanar and chroma != '420':
            raise ValueError(f"a semi-planar frame is '420', not {chroma!r}")
        buf = pinned_empty(self.lib, (n, deep_frame_bytes(size, chroma)), np.uint8)
        if semiplanar:
            return [DeepFrame.semiplanar_from_buffer(buf[i], size, depth=depth, matrix=matrix) for i in range(n)]
        return [DeepFrame.from_buffer(buf[i], size, chroma, depth, matrix) for i in range(n)]

    def frame_ring_store(self, index, frame):
        self._frame_call('ring_store', (C.c_int(index),), frame)

    def frame_ring_select(self, index):
        check(self.lib.fm_frame_ring_select(self._ctx, C.c_int(index)))

    def frame_upload_next(self, frame):
        if isinstance(frame, (NV12Frame, JPEGFrame, SourceFrame, PlanarFrame, PackedFrame, BayerFrame, DeepFrame, DeviceArrayFrame)):
            return self.frame_upload_ahead(1, frame)
        w, h = self.frame_size
        if frame.shape != (h, w, 3) or frame.dtype != np.uint8:
            raise ValueError(f'frame must be uint8 {h}x{w}x3')
        f = np.ascontiguousarray(frame)
        check(self.lib.fm_frame_upload_next(self._ctx, _ptr(f)))

    def frame_ring_select_next(self, index):
        check(self.lib.fm_frame_ring_select_next(self._ctx, C.c_int(index)))

    def frame_promote_next(self):
        check(self.lib.fm_frame_promote_next(self._ctx))

    def detect_async_next(self):
        check(self.lib.fm_detect_async_next(self._ctx))

    def frame_upload_ahead(self, k, frame):
        """Host frame for the step k steps ahead (look-ahead slot k, 1 <= k <= FM_MAX_DET_BATCH; k = 1: frame_upload_next)."""
        self._frame_call('upload_ahead', (C.c_int(k),), frame)

    def frame_ring_select_ahead(self, k, index):
        check(self.lib.fm_frame_ring_select_ahead(self._ctx, C.c_int(k), C.c_int(index)))

    def detect_async_ahead(self, n):
        """One detector pass at batch n over look-ahead slots 1..n; each of the next n detect_sync calls returns one frame."""
        check(self.lib.fm_detect_async_ahead(self._ctx, C.c_int(n)))

    def frame_read(self):
        w, h = self.frame_size
        out = np.empty((h, w, 3), np.uint8)
        check(self.lib.fm_frame_read(self._ctx, _ptr(out)))
        return out

    def _jpeg_out(self, width, height):
        """The buffer encoded files are written to before they become `bytes`: the worst case for the size, kept across calls
        (untouched pages of it cost nothing)."""
        bound = self.lib.fm_jpeg_encode_bound(C.c_int(width), C.c_int(height))
        if not bound:
            raise ValueError(f'frame size {width}x{height} outside 1..16384')
        out = getattr(self, '_jpeg_out_buf', None)
        if out is None or out.size < bound:
            out = self._jpeg_out_buf = np.empty(bound, np.uint8)
        return out

    def frame_encode_jpeg(self, quality=75):
        """The frame the context holds on the device (the one bound last) as a baseline JPEG file -> bytes."""
        if getattr(self, 'frame_size', None) is None:
            raise FastMOTHipError('no frame on the device yet')
        out = self._jpeg_out(*self.frame_size)
        n = C.c_size_t(0)
        check(self.lib.fm_frame_encode_jpeg(self._ctx, C.c_int(int(quality)), _ptr(out), C.c_size_t(out.size), C.byref(n)))
        return out[:n.value].tobytes()

    def jpeg_encode_bgr(self, frame, quality=75):
        """Host pixels [H, W, 3] uint8 BGR (rows may be strided) as a baseline JPEG file -> bytes."""
        if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError('frame must be a uint8 HxWx3 array')
        if frame.strides[1:] != (3, 1) or frame.strides[0] < 3 * frame.shape[1]:
            frame = np.ascontiguousarray(frame)
        h, w = frame.shape[:2]
        out = self._jpeg_out(w, h)
        n = C.c_size_t(0)
        check(self.lib.fm_jpeg_encode_bgr(self._ctx, _ptr(frame), C.c_int(w), C.c_int(h), C.c_size_t(frame.strides[0]), C.c_int(int(quality)),
                                          _ptr(out), C.c_size_t(out.size), C.byref(n)))
        return out[:n.value].tobytes()

    def frame_encode_regions(self, rects, quality=85, shrink=1, overlay=False):
        """Rectangles of the frame the context holds (overlay=True: of the overlay buffer) as baseline JPEG files, all in
        one pass of the encoder -> list of bytes, one per rectangle.  rects: an (n, 4) integer array of inclusive corners
        (x0, y0, x1, y1) inside the frame (utils.redact.region_rect clips).  shrink 2 / 4: every crop reduced by that factor
        first (block means, fastmot_hip.h).  File i equals utils.jpeg.encode_bgr(picture[y0:y1 + 1, x0:x1 + 1], quality).
        A list beyond what one library call takes (FM_OBJENC_MAX_REGIONS rectangles, FM_OBJENC_MAX_MCUS MCUs) is split into
        several calls; a single rectangle above the MCU limit is refused."""
        if getattr(self, 'frame_size', None) is None:
            raise FastMOTHipError('no frame on the device yet')
        if not 1 <= int(quality) <= 100:
            raise ValueError(f'quality {quality} outside 1..100')
        if shrink not in OBJENC_SHRINKS:
            raise ValueError(f'shrink {shrink!r}: one of {OBJENC_SHRINKS}')
        arr = _crop_rects(rects)
        which = FM_EXPORT_OVERLAY if overlay else FM_EXPORT_FRAME
        files = []
        start = 0
        while start < len(arr):
            # the longest run from `start` that one call takes: MCUs of a rect as the plan counts them
            w = (arr[start:, 2] - arr[start:, 0] + int(shrink)) // int(shrink)
            h = (arr[start:, 3] - arr[start:, 1] + int(shrink)) // int(shrink)
            mcus = np.cumsum(np.maximum((w.astype(np.int64) + 15) // 16, 0) * np.maximum((h.astype(np.int64) + 15) // 16, 0))
            take = max(1, min(int(np.searchsorted(mcus, self.OBJENC_CHUNK_MCUS, side='right')), self.OBJENC_CHUNK_REGIONS))
            files += self._encode_regions_call(arr[start:start + take], which, int(quality), int(shrink))
            start += take
        return files

    def _encode_regions_call(self, arr, which, quality, shrink):
        n = len(arr)
        bound = self.lib.fm_jpeg_encode_regions_bound(_ptr(arr), C.c_int(n), C.c_int(shrink))
        if not bound:
            raise FastMOTHipError(f'libfastmot_hip error: {self.lib.fm_last_error().decode()}')
        out = getattr(self, '_objenc_out_buf', None)
        if out is None or out.size < bound:
            out = self._objenc_out_buf = np.empty(bound, np.uint8)       # (untouched pages of it cost nothing)
        offsets = np.zeros(n + 1, np.uintp)
        check(self.lib.fm_frame_encode_regions(self._ctx, C.c_int(which), _ptr(arr), C.c_int(n), C.c_int(shrink), C.c_int(quality),
                                               _ptr(out), C.c_size_t(out.size), _ptr(offsets)))
        return [out[int(a):int(b)].tobytes() for a, b in zip(offsets[:-1], offsets[1:])]

    def _i420_out(self, width, height):
        bound = self.lib.fm_i420_bound(C.c_int(width), C.c_int(height))
        if not bound:
            raise ValueError(f'frame size {width}x{height} outside 1..16384')
        return np.empty(bound, np.uint8)

    def _export_i420(self, which):
        if getattr(self, 'frame_size', None) is None:
            raise FastMOTHipError('no frame on the device yet')
        out = self._i420_out(*self.frame_size)
        n = C.c_size_t(0)
        check(self.lib.fm_frame_export_i420(self._ctx, C.c_int(which), _ptr(out), C.c_size_t(out.size), C.byref(n)))
        return out[:n.value]

    def frame_export_i420(self):
        """The frame the context holds on the device (the one bound last) as planar 4:2:0 -> 1-D uint8 array: Y, then U,
        then V (utils.yuv.bgr_to_planar420 of frame_read(), converted on the GPU; 1.5 bytes per pixel come back)."""
        return self._export_i420(FM_EXPORT_FRAME)

    def overlay_export_i420(self):
        """The overlay buffer of the last frame_render_overlay as planar 4:2:0 (frame_export_i420's format)."""
        return self._export_i420(FM_EXPORT_OVERLAY)

    def i420_from_bgr(self, frame):
        """Host pixels [H, W, 3] uint8 BGR (rows may be strided) as planar 4:2:0, converted on the GPU -> 1-D uint8 array."""
        if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError('frame must be a uint8 HxWx3 array')
        if frame.strides[1:] != (3, 1) or frame.strides[0] < 3 * frame.shape[1]:
            frame = np.ascontiguousarray(frame)
        h, w = frame.shape[:2]
        out = self._i420_out(w, h)
        n = C.c_size_t(0)
        check(self.lib.fm_i420_from_bgr(self._ctx, _ptr(frame), C.c_int(w), C.c_int(h), C.c_size_t(frame.strides[0]), _ptr(out),
                                        C.c_size_t(out.size), C.byref(n)))
        return out[:n.value]

    def jpeg_encode_stream_ms(self):
        """HIP-event time of the kernels of the last encode, or None before the first."""
        ms = C.c_float(0)
        check(self.lib.fm_jpeg_encode_stream_ms(self._ctx, C.byref(ms)))
        return ms.value if ms.value >= 0 else None

    def frame_render_overlay(self, cmds, masks=b''):
        """The frame the context holds on the device + an overlay command list (utils/overlay.py) -> the context's overlay
        buffer; the frame itself is not written."""
        cmds, masks, args = _overlay_args(cmds, masks)
        check(self.lib.fm_frame_render_overlay(self._ctx, *args))

    def overlay_read(self):
        """The overlay buffer of the last frame_render_overlay -> ndarray [H, W, 3] uint8 BGR."""
        if getattr(self, 'frame_size', None) is None:
            raise FastMOTHipError('no frame on the device yet')
        w, h = self.frame_size
        out = np.empty((h, w, 3), np.uint8)
        check(self.lib.fm_overlay_read(self._ctx, _ptr(out)))
        return out

    def overlay_encode_jpeg(self, quality=75):
        """The overlay buffer as a baseline JPEG file -> bytes (frame_encode_jpeg's format)."""
        if getattr(self, 'frame_size', None) is None:
            raise FastMOTHipError('no frame on the device yet')
        out = self._jpeg_out(*self.frame_size)
        n = C.c_size_t(0)
        check(self.lib.fm_overlay_encode_jpeg(self._ctx, C.c_int(int(quality)), _ptr(out), C.c_size_t(out.size), C.byref(n)))
        return out[:n.value].tobytes()

    def overlay_stream_ms(self):
        """HIP-event time of the last render's kernel, or None before the first."""
        ms = C.c_float(0)
        check(self.lib.fm_overlay_stream_ms(self._ctx, C.byref(ms)))
        return ms.value if ms.value >= 0 else None

    def frame_render_redacted(self, regions, cmds=(), masks=b''):
        """The frame the context holds on the device, redacted by a region list (utils/redact.py) and then drawn on by an
        overlay command list (may be empty) -> the context's overlay buffer, which overlay_read / overlay_encode_jpeg /
        overlay_export_i420 serve; the frame itself is not written."""
        regions, rargs = _redact_args(regions)
        cmds, masks, args = _overlay_args(cmds if len(cmds) else np.zeros(0, OVERLAY_CMD_DTYPE), masks)
        check(self.lib.fm_frame_render_redacted(self._ctx, *rargs, *args))

    def redact_stream_ms(self):
        """HIP-event time of the last frame_render_redacted's kernels (cell means + tile pass), or None before the first."""
        ms = C.c_float(0)
        check(self.lib.fm_redact_stream_ms(self._ctx, C.byref(ms)))
        return ms.value if ms.value >= 0 else None

    def detect_configure(self, cfg):
        check(self.lib.fm_detect_configure(self._ctx, C.byref(cfg)))

    def detect_configure_dfl(self, cfg, heads):
        """fm_detect_configure_dfl: `cfg` as for detect_configure (its anchor fields are ignored), `heads` a DflHeads."""
        check(self.lib.fm_detect_configure_dfl(self._ctx, C.byref(cfg), C.byref(heads)))

    def detect_async(self):
        check(self.lib.fm_detect_async(self._ctx))

    def detect_net_ms(self):
        """HIP-event time of the detector network of the pass collected last, or None when that pass was not timed
        (option 'net_timing' = N: every N-th pass carries the event pair; 0, the default: none)."""
        ms = C.c_float(0)
        check(self.lib.fm_detect_net_ms(self._ctx, C.byref(ms)))
        return ms.value if ms.value >= 0 else None

    def detect_preprocess_only(self):
        check(self.lib.fm_detect_preprocess_only(self._ctx))

    def detect_sync(self, cap=4096):
        # (a staging array kept across calls: a fresh 196 KB np.zeros per frame cost ~10 us on the step's critical chain)
        out = getattr(self, '_det_stage', None)
        if out is None or len(out) < cap:
            out = self._det_stage = np.zeros(cap, DET_DTYPE)
        n = C.c_int(0)
        check(self.lib.fm_detect_sync(self._ctx, _ptr(out), C.c_int(cap), C.byref(n)))
        return out[:n.value].copy().view(np.recarray)

    def filter_dets(self, rows, cap=8192):
        r = _as(rows, np.float32).reshape(-1, 7)
        out = np.zeros(cap, DET_DTYPE)
        n = C.c_int(0)
        check(self.lib.fm_filter_dets(self._ctx, _ptr(r), C.c_int(len(r)), _ptr(out), C.c_int(cap), C.byref(n)))
        return out[:n.value].view(np.recarray)

    def detect_last_counts(self):
        nc, nd = C.c_int(0), C.c_int(0)
        check(self.lib.fm_detect_last_counts(self._ctx, C.byref(nc), C.byref(nd)))
        return nc.value, nd.value

    def detect_configure_tiles(self, origins, region, offsets, merge_thresh):
        """Makes the configured detector tiled (fm_detect_configure_tiles): `origins` [n][2] tile corners in the tiling
        region `region` = (w, h); `offsets` [n][2]: the decode's box offset per tile (its scale is the configuration's
        `size`).  No origins: untiled again."""
        o = _as(origins, np.int32).reshape(-1, 2)
        off = _as(offsets, np.float64).reshape(-1, 2)
        assert len(off) == len(o)
        check(self.lib.fm_detect_configure_tiles(self._ctx, C.c_int(len(o)), _ptr(o), C.c_int(int(region[0])),
                                                 C.c_int(int(region[1])), _ptr(off), C.c_double(merge_thresh)))

    def detect_last_tiles(self):
        """The per-tile detections of the frame detect_sync collected last, before the cross-tile merge: a list of record
        arrays (DET_DTYPE), one per tile."""
        cap = max(self.detect_last_counts()[1], 1)          # (tiled: the detections summed over the tiles)
        out = np.zeros(cap, DET_DTYPE)
        counts = np.zeros(FM_MAX_DET_BATCH, np.int32)
        n = C.c_int(0)
        check(self.lib.fm_detect_last_tiles(self._ctx, _ptr(out), C.c_int(cap), _ptr(counts), C.byref(n)))
        ends = np.cumsum(counts[:n.value])
        return [out[e - c:e].copy().view(np.recarray) for c, e in zip(counts[:n.value], ends)]

    def detect_decode_us(self, iters=20):
        """fm_detect_decode_us: mean HIP-event time of the decode kernel alone over the last pass's head tensors."""
        us = C.c_float(0)
        check(self.lib.fm_detect_decode_us(self._ctx, C.c_int(iters), C.byref(us)))
        return us.value

    def detect_raw_candidates(self, cap=65536):
        rows = np.empty((cap, 8), np.float32)
        n = C.c_int(0)
        check(self.lib.fm_detect_raw_candidates(self._ctx, _ptr(rows), C.c_int(cap), C.byref(n)))
        return rows[:n.value]

    def ssd_configure(self, map_shapes, anchors_per_cell, anchors, box_scales, num_classes, topk, nms_thresh, tile_origins,
                      region, in_wh, input_tensor=0, head_tensors=None):
        """fm_ssd_configure.  map_shapes [(h, w)], anchors_per_cell [A] per head; anchors float32 [n, 4] (cy, cx, h, w);
        tile_origins [(x, y)] in the tiling region `region` = (w, h); in_wh: the network input (w, h).  head_tensors: the
        head tensor ids of the detector network (None: only ssd_postprocess_host_heads will be used)."""
        cfg = SsdCfg()
        a = _as(anchors, np.float32).reshape(-1, 4)
        cfg.input_tensor, cfg.in_w, cfg.in_h, cfg.n_heads = input_tensor, int(in_wh[0]), int(in_wh[1]), len(map_shapes)
        for k, ((h, w), na) in enumerate(zip(map_shapes, anchors_per_cell)):
            cfg.head_tensor[k] = head_tensors[k] if head_tensors is not None else -1
            cfg.map_w[k], cfg.map_h[k], cfg.n_anchors[k] = int(w), int(h), int(na)
        cfg.anchors, cfg.n_anchor_rows = a.ctypes.data, len(a)
        cfg.box_scales[:] = [float(v) for v in box_scales]
        cfg.num_classes, cfg.topk, cfg.nms_thresh, cfg.n_tiles = int(num_classes), int(topk), float(nms_thresh), len(tile_origins)
        for t, (x, y) in enumerate(tile_origins):
            cfg.tile_x[t], cfg.tile_y[t] = int(x), int(y)
        cfg.region_w, cfg.region_h = int(region[0]), int(region[1])
        check(self.lib.fm_ssd_configure(self._ctx, C.byref(cfg)))
        self._ssd_n_tiles = len(tile_origins)
        self._ssd_rows = np.zeros((len(tile_origins) * int(topk), 7), np.float32)
        self._ssd_heads = [(int(h) * int(w), int(na) * (4 + int(num_classes))) for (h, w), na in zip(map_shapes, anchors_per_cell)]

    def ssd_detect_async(self):
        check(self.lib.fm_ssd_detect_async(self._ctx))

    def ssd_stage_ms(self):
        """(preprocess, network, decode / NMS) HIP-event times in ms of the last collected pass, or None when it was not timed
        (option 'net_timing' > 0)."""
        ms = (C.c_float * 3)()
        check(self.lib.fm_ssd_stage_ms(self._ctx, ms))
        return tuple(ms) if ms[0] >= 0 else None

    def ssd_preprocess_only(self):
        check(self.lib.fm_ssd_preprocess_only(self._ctx))

    def ssd_detect_sync(self):
        """-> float32 [n_tiles * topk, 7] rows (tile, label, conf, xmin, ymin, xmax, ymax) of the pass in flight"""
        n = C.c_int(0)
        check(self.lib.fm_ssd_detect_sync(self._ctx, _ptr(self._ssd_rows), C.c_int(len(self._ssd_rows)), C.byref(n)))
        return self._ssd_rows[:n.value].copy()

    def ssd_postprocess_host_heads(self, heads):
        """Decode + NMS + top-K of host head tensors: heads[k] float32 [n_tiles, map_h * map_w, A * (4 + num_classes)]."""
        n_tiles = self._ssd_n_tiles               # (the library reads the configured number of tiles from every pointer)
        hs = [_as(h, np.float32) for h in heads]
        if len(hs) != len(self._ssd_heads):
            raise ValueError(f'{len(hs)} head tensors, the configuration has {len(self._ssd_heads)}')
        for h, (hw, cs) in zip(hs, self._ssd_heads):
            if h.shape != (n_tiles, hw, cs):
                raise ValueError(f'head tensor of shape {h.shape}, the configuration needs {(n_tiles, hw, cs)}')
        ptrs = (C.c_void_p * len(hs))(*[h.ctypes.data for h in hs])
        n = C.c_int(0)
        check(self.lib.fm_ssd_postprocess_host_heads(self._ctx, ptrs, _ptr(self._ssd_rows), C.c_int(len(self._ssd_rows)), C.byref(n)))
        return self._ssd_rows[:n.value].copy()

    def extract_configure(self, input_tensor, in_w, in_h):
        check(self.lib.fm_extract_configure(self._ctx, C.c_int(input_tensor), C.c_int(in_w), C.c_int(in_h)))

    def extract_async(self, tlbrs):
        b = _as(tlbrs, np.float64).reshape(-1, 4)
        check(self.lib.fm_extract_async(self._ctx, C.c_int(len(b)), _ptr(b)))
        return len(b)

    def extract_sync(self, n):
        out = np.empty((n, self.feat_dim), np.float32)
        check(self.lib.fm_extract_sync(self._ctx, C.c_int(n), _ptr(out)))
        return out

    def extract_read_input(self, n, in_w, in_h):
        out = np.empty((n, in_h, in_w, 3), np.float32)
        check(self.lib.fm_extract_read_input(self._ctx, C.c_int(n), _ptr(out)))
        return out

    for fn in (frame_configure, frame_set_lens, _described, _frame_kind, _frame_call, _device_check, device_frame_done, device_frames_prune, pending_device_frames, _nv12_args, _jpeg_args, pinned_deep_frames, pinned_planar_frames, pinned_packed_frames, pinned_bayer_frames, _i420_out, _export_i420, frame_export_i420,
               overlay_export_i420, i420_from_bgr, frame_upload, pinned_frames, pinned_source_frames, pinned_nv12_frames, pinned_jpeg_buffers, frame_ring_store, frame_ring_select, frame_read, frame_upload_next,
               _jpeg_out, frame_encode_jpeg, jpeg_encode_bgr, jpeg_encode_stream_ms, frame_encode_regions, _encode_regions_call,
               frame_render_overlay, overlay_read, overlay_encode_jpeg, overlay_stream_ms, frame_render_redacted, redact_stream_ms,
               frame_ring_select_next, frame_promote_next, detect_async_next, frame_upload_ahead, frame_ring_select_ahead,
               detect_async_ahead,
               detect_configure, detect_configure_dfl, detect_async, detect_net_ms, detect_preprocess_only, detect_sync, filter_dets,
               detect_raw_candidates, detect_decode_us, detect_last_counts, detect_configure_tiles, detect_last_tiles,
               ssd_configure, ssd_detect_async, ssd_stage_ms, ssd_preprocess_only, ssd_detect_sync, ssd_postprocess_host_heads,
               extract_configure, extract_async, extract_sync, extract_read_input):
        setattr(cls, fn.__name__, fn)
    # what frame_encode_regions hands to ONE library call at most (the library's limits)
    cls.OBJENC_CHUNK_REGIONS, cls.OBJENC_CHUNK_MCUS = FM_OBJENC_MAX_REGIONS, FM_OBJENC_MAX_MCUS


_bind_device_io(HipContext)


# ---------------------------------------------------------------------- optical flow
class FlowPredictParams(C.Structure):
    _fields_ = [('feat_density', C.c_double), ('feat_dist_factor', C.c_double),
                ('opt_scale', C.c_float * 2), ('bg_scale', C.c_float * 2),
                ('max_error', C.c_double), ('ransac_max_iter', C.c_int32), ('ransac_conf', C.c_double),
                ('inlier_thresh', C.c_int32), ('frame_w', C.c_int32), ('frame_h', C.c_int32)]


FLOW_OK, FLOW_NO_BACKGROUND, FLOW_NO_HOMOGRAPHY = 0, 1, 2


class FlowCfg(C.Structure):
    _fields_ = [('small_w', C.c_int32), ('small_h', C.c_int32), ('bg_w', C.c_int32), ('bg_h', C.c_int32),
                ('win_size', C.c_int32), ('max_level', C.c_int32), ('max_count', C.c_int32),
                ('epsilon', C.c_double), ('fast_thresh', C.c_int32), ('max_corners', C.c_int32),
                ('block_size', C.c_int32), ('quality_level', C.c_double), ('gray_coeff_bits', C.c_int32)]


def _bind_flow(cls):
    def flow_configure(self, cfg):
        check(self.lib.fm_flow_configure(self._ctx, C.byref(cfg)))

    def flow_init(self):
        check(self.lib.fm_flow_init(self._ctx))

    def flow_begin(self):
        check(self.lib.fm_flow_begin(self._ctx))

    def flow_swap(self):
        check(self.lib.fm_flow_swap(self._ctx))

    def flow_targets(self, inside_tlbr, kps, kp_off):
        r = _as(inside_tlbr, np.float64).reshape(-1, 4)
        nT = len(r)
        off = _as(kp_off, np.int32)
        k = _as(kps, np.float32).reshape(-1, 2)
        assert len(off) == nT + 1 and off[-1] == len(k)
        area = np.zeros(nT, np.int32)
        keep = np.zeros(len(k), np.uint8)
        check(self.lib.fm_flow_targets(self._ctx, C.c_int(nT), _ptr(r), _ptr(k), _ptr(off), _ptr(area), _ptr(keep)))
        return area, keep.astype(bool)

    def flow_prepare(self, inside_tlbr, full_tlbr, kps, kp_off, feat_density, feat_dist_factor,
                     pts_cap=65536, bg_cap=8192):
        r = _as(inside_tlbr, np.float64).reshape(-1, 4)
        nT = len(r)
        fb = _as(full_tlbr, np.float64).reshape(nT, 4)
        off = _as(kp_off, np.int32)
        k = _as(kps, np.float32).reshape(-1, 2)
        assert len(off) == nT + 1 and off[-1] == len(k)
        area = np.zeros(nT, np.int32)
        keep = np.zeros(len(k), np.uint8)
        needy = np.zeros(nT, np.uint8)
        if not hasattr(self, '_flow_bufs') or self._flow_bufs[0].shape[0] < pts_cap or self._flow_bufs[1].shape[0] < bg_cap:
            self._flow_bufs = (np.empty((pts_cap, 2), np.float32), np.empty((bg_cap, 2), np.float32))
        new_pts, bg = self._flow_bufs
        new_off = np.zeros(nT, np.int32)
        new_cnt = np.zeros(nT, np.int32)
        n_new, n_bg = C.c_int(0), C.c_int(0)
        check(self.lib.fm_flow_prepare(self._ctx, C.c_int(nT), _ptr(r), _ptr(fb), _ptr(k), _ptr(off),
                                       C.c_double(feat_density), C.c_double(feat_dist_factor), _ptr(area), _ptr(keep),
                                       _ptr(needy), C.c_int(pts_cap), _ptr(new_pts), _ptr(new_off), _ptr(new_cnt),
                                       C.byref(n_new), C.c_int(bg_cap), _ptr(bg), C.byref(n_bg)))
        return area, keep.astype(bool), needy.astype(bool), new_pts, new_off, new_cnt, bg[:n_bg.value].copy()

    def flow_predict(self, inside_tlbr, full_tlbr, kps, kp_off, params, pts_cap=65536):
        """fm_flow_predict: -> (status, H, result, est_tlbr, n_matched, prev_pts, cur_pts, trk_off, bg_range);
        prev/cur are the compacted RANSAC-inlier keypoints (views of per-call arrays)."""
        r = _as(inside_tlbr, np.float64).reshape(-1, 4)
        nT = len(r)
        fb = _as(full_tlbr, np.float64).reshape(nT, 4)
        off = _as(kp_off, np.int32)
        k = _as(kps, np.float32).reshape(-1, 2)
        assert len(off) == nT + 1 and off[-1] == len(k)
        prev = np.empty((pts_cap, 2), np.float32)
        cur = np.empty((pts_cap, 2), np.float32)
        trk_off = np.zeros(nT + 1, np.int32)
        bg_range = np.zeros(2, np.int32)
        H = np.zeros((3, 3))
        status = C.c_int(0)
        result = np.zeros(nT, np.int32)
        est = np.zeros((nT, 4))
        n_matched = np.zeros(nT, np.int32)
        check(self.lib.fm_flow_predict(self._ctx, C.c_int(nT), _ptr(r), _ptr(fb), _ptr(k), _ptr(off), C.byref(params),
                                       C.c_int(pts_cap), _ptr(prev), _ptr(cur), _ptr(trk_off), _ptr(bg_range),
                                       _ptr(H), C.byref(status), _ptr(result), _ptr(est), _ptr(n_matched)))
        return status.value, H, result, est, n_matched, prev, cur, trk_off, bg_range

    def track_predict_async(self, inside_tlbr, full_tlbr, kps, kp_off, params, slots, ages, sorted_idx, age_penalty,
                            pts_cap=65536):
        """fm_track_predict_async: fm_flow_predict + the Kalman step on the library's worker thread.  Returns a job
        (it owns every buffer the worker reads or writes) for track_predict_wait."""
        job = SimpleNamespace()
        job.r = _as(inside_tlbr, np.float64).reshape(-1, 4)
        nT = len(job.r)
        job.fb = _as(full_tlbr, np.float64).reshape(nT, 4)
        job.off = _as(kp_off, np.int32)
        job.k = _as(kps, np.float32).reshape(-1, 2)
        assert len(job.off) == nT + 1 and job.off[-1] == len(job.k)
        job.prev = np.empty((pts_cap, 2), np.float32)
        job.cur = np.empty((pts_cap, 2), np.float32)
        job.trk_off = np.zeros(nT + 1, np.int32)
        job.bg_range = np.zeros(2, np.int32)
        job.H = np.zeros((3, 3))
        job.result = np.zeros(nT, np.int32)
        job.est = np.zeros((nT, 4))
        job.n_matched = np.zeros(nT, np.int32)
        job.slots = _as(slots, np.int32)
        nK = len(job.slots)
        job.ages = _as(ages, np.int32)
        job.sorted_idx = _as(sorted_idx, np.int32)
        assert len(job.ages) == nK and len(job.sorted_idx) == nK
        job.tlbr = np.empty((nK, 4), np.float64)
        job.lost = np.zeros(nK, np.uint8)
        job.params = params
        check(self.lib.fm_track_predict_async(
            self._ctx, C.c_int(nT), _ptr(job.r), _ptr(job.fb), _ptr(job.k), _ptr(job.off), C.byref(params),
            C.c_int(pts_cap), _ptr(job.prev), _ptr(job.cur), _ptr(job.trk_off), _ptr(job.bg_range), _ptr(job.H),
            _ptr(job.result), _ptr(job.est), _ptr(job.n_matched), C.c_int(nK), _ptr(job.slots), _ptr(job.ages),
            _ptr(job.sorted_idx), C.c_double(float(age_penalty)), _ptr(job.tlbr), _ptr(job.lost)))
        return job

    def track_predict_wait(self, job):
        """-> (the tuple ctx.flow_predict returns, next_tlbrs, lost) ; the last two are None when no Kalman step ran."""
        status, kalman = C.c_int(0), C.c_int(0)
        check(self.lib.fm_track_predict_wait(self._ctx, C.byref(status), C.byref(kalman)))
        pred = (status.value, job.H, job.result, job.est, job.n_matched, job.prev, job.cur, job.trk_off, job.bg_range)
        if kalman.value:
            return pred, job.tlbr, job.lost.astype(bool)
        return pred, None, None

    def flow_detect(self, track_idx, track_tlbr, min_dist, cap=1000):
        idx = _as(track_idx, np.int32)
        n = len(idx)
        tb = _as(track_tlbr, np.float64).reshape(n, 4)
        md = _as(min_dist, np.int32)
        pts = np.empty((n, cap, 2), np.float32)
        cnt = np.zeros(n, np.int32)
        check(self.lib.fm_flow_detect(self._ctx, C.c_int(n), _ptr(idx), _ptr(tb), _ptr(md), C.c_int(cap),
                                      _ptr(pts), _ptr(cnt)))
        return pts, cnt

    def flow_background(self, cap=8192):
        pts = np.empty((cap, 2), np.float32)
        n = C.c_int(0)
        check(self.lib.fm_flow_background(self._ctx, C.c_int(cap), _ptr(pts), C.byref(n)))
        return pts[:n.value]

    def flow_lk(self, prev_pts):
        p = _as(prev_pts, np.float32).reshape(-1, 2)
        n = len(p)
        nxt = np.empty((n, 2), np.float32)
        status = np.zeros(n, np.uint8)
        err = np.zeros(n, np.float32)
        check(self.lib.fm_flow_lk(self._ctx, C.c_int(n), _ptr(p), _ptr(nxt), _ptr(status), _ptr(err)))
        return nxt, status, err

    def gallery_unique_id(self):
        buf = C.create_string_buffer(128)
        check(self.lib.fm_gallery_unique_id(buf))
        return buf.raw

    def gallery_init(self, channel, world, rank, unique_id, row_bytes):
        assert len(unique_id) == 128
        check(self.lib.fm_gallery_init(self._ctx, C.c_int(channel), C.c_int(world), C.c_int(rank), C.c_char_p(unique_id),
                                       C.c_size_t(row_bytes)))

    def gallery_allgather_async(self, channel, row):
        row = np.ascontiguousarray(row, np.uint8)
        check(self.lib.fm_gallery_allgather_async(self._ctx, C.c_int(channel), _ptr(row)))

    def gallery_allgather_wait(self, channel, world, row_bytes):
        out = np.empty(world * row_bytes, np.uint8)
        ms = C.c_float(0)
        check(self.lib.fm_gallery_allgather_wait(self._ctx, C.c_int(channel), _ptr(out), C.byref(ms)))
        return out, float(ms.value)

    def gallery_destroy(self, channel=0):
        check(self.lib.fm_gallery_destroy(self._ctx, C.c_int(channel)))

    def flow_estimate(self, prev_pts, cur_pts, status, begins, ends, bg_begin, bg_end, track_tlbr, size,
                      ransac_max_iter, ransac_conf, inlier_thresh):
        p = _as(prev_pts, np.float32).reshape(-1, 2)
        c = _as(cur_pts, np.float32).reshape(-1, 2)
        st = _as(status, np.uint8)
        n = len(p)
        b, e = _as(begins, np.int32), _as(ends, np.int32)
        nT = len(b)
        tb = _as(track_tlbr, np.float64).reshape(nT, 4)
        H = np.zeros((3, 3))
        ok = C.c_int(0)
        result = np.zeros(nT, np.int32)
        est = np.zeros((nT, 4))
        n_matched = np.zeros(nT, np.int32)
        inl = np.zeros(n, np.uint8)
        check(self.lib.fm_flow_estimate(self._ctx, C.c_int(n), _ptr(p), _ptr(c), _ptr(st), C.c_int(nT), _ptr(b),
                                        _ptr(e), C.c_int(bg_begin), C.c_int(bg_end), _ptr(tb), C.c_int(size[0]),
                                        C.c_int(size[1]), C.c_int(ransac_max_iter), C.c_double(ransac_conf),
                                        C.c_int(inlier_thresh), _ptr(H), C.byref(ok), _ptr(result), _ptr(est),
                                        _ptr(n_matched), _ptr(inl)))
        return (H if ok.value else None), result, est, n_matched, inl.astype(bool)

    def flow_read_image(self, which):
        w, h = C.c_int(0), C.c_int(0)
        buf = np.empty(self.frame_size[0] * self.frame_size[1] * 4, np.uint8)
        check(self.lib.fm_flow_read_image(self._ctx, C.c_int(which), _ptr(buf), C.byref(w), C.byref(h)))
        return buf[:w.value * h.value].reshape(h.value, w.value).copy()

    for fn in (flow_configure, flow_init, flow_begin, track_predict_async,
               track_predict_wait, flow_swap, flow_targets, flow_prepare, flow_predict, flow_detect,
               flow_background,
               flow_lk, gallery_unique_id, gallery_init,
               gallery_allgather_async, gallery_allgather_wait, gallery_destroy, flow_estimate, flow_read_image):
        setattr(cls, fn.__name__, fn)


_bind_flow(HipContext)
