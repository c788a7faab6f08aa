"""Lens correction maps: the geometry between the sensor and the tracker.

Everything behind the frame assumes a pinhole picture -- the Kalman filter's box model, the homography `flow` fits, the
aspect ratios the detector was trained on -- while surveillance and embedded cameras ship with wide-angle and fisheye
lenses.  A `LensMap` holds, for every pixel of the tracker's `size` frame, where in the captured frame it comes from;
`SourceFrame(frame, lens=...)` has the frame corrected on the GPU by the gather that already resizes capture-resolution
frames (csrc/remap.hip takes the place of csrc/resize.hip: one kernel, no pass of its own), and `remap_bgr` is the same
arithmetic in numpy -- the device frame equals `remap_bgr(frame, lens)` bit for bit.

The arithmetic (csrc/remap_pixel.h states it once for the kernel and for fm_remap_bgr_host): a map entry is a source
coordinate in fixed point with 5 fractional bits, X = rint(32 x), Y = rint(32 y) (round half to even), clipped to
[-64, 32 (sw + 1)] and [-64, 32 (sh + 1)]; NaN and +-inf become -64, which is fully outside.  With ix = X >> 5, fx = X & 31
and the same for y, the taps are (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1); a tap outside the source
contributes the border colour, chosen per tap, and per channel

    v = ((32 - fy) ((32 - fx) p00 + fx p01) + fy ((32 - fx) p10 + fx p11) + 512) >> 10

which is the float64 bilinear value of the quantised coordinate rounded half up.  It is not `videoio.resize_bgr`'s
arithmetic (11-bit separable coefficients): an identity-geometry map gives pixels near the resize's, not equal to them."""
import numpy as np

FRAC_BITS = 5
ONE = 1 << FRAC_BITS
OUTSIDE = -2 * ONE          # two whole pixels left of / above the source: all four taps outside
MAX_DIM = 16384             # FM_SRC_MAX_DIM of include/fastmot_hip.h
MAX_ITER, STEP_TOL = 100, 1e-12      # to_destination: iterations, and the step (normalised units) it stops below


def _size(size, what):
    w, h = (int(v) for v in size)
    if not (1 <= w <= MAX_DIM and 1 <= h <= MAX_DIM):
        raise ValueError(f'{what} size {w}x{h} outside 1..{MAX_DIM}')
    return w, h


def _border(border):
    b = tuple(int(v) for v in border)
    if len(b) != 3 or not all(0 <= v <= 255 for v in b):
        raise ValueError(f'border must be a BGR triple of 0..255, not {border!r}')
    return b


def quantise(map_x, map_y, src_size):
    """Float source coordinates (two arrays of one shape (dh, dw)) -> the int32 (dh, dw, 2) fixed-point map."""
    sw, sh = _size(src_size, 'source')
    map_x, map_y = np.asarray(map_x, np.float64), np.asarray(map_y, np.float64)
    if map_x.ndim != 2 or map_x.shape != map_y.shape:
        raise ValueError(f'map_x and map_y must be two (H, W) arrays of one shape, not {map_x.shape} and {map_y.shape}')
    out = np.empty(map_x.shape + (2,), np.int32)
    for c, (m, n) in enumerate(((map_x, sw), (map_y, sh))):
        finite = np.isfinite(m)
        with np.errstate(over='ignore'):
            q = np.rint(np.where(finite, m, 0.) * float(ONE))
        out[..., c] = np.where(finite, np.clip(q, OUTSIDE, ONE * (n + 1)), OUTSIDE)
    return out


def _intrinsics(camera_matrix, what='camera_matrix'):
    k = np.asarray(camera_matrix, np.float64)
    if k.shape == (3, 3):
        fx, fy, cx, cy = k[0, 0], k[1, 1], k[0, 2], k[1, 2]
    elif k.shape == (4,):
        fx, fy, cx, cy = k
    else:
        raise ValueError(f'{what} must be 3x3 or (fx, fy, cx, cy), not shape {k.shape}')
    if not (np.all(np.isfinite([fx, fy, cx, cy])) and fx > 0 and fy > 0):
        raise ValueError(f'{what} needs finite entries and positive focal lengths')
    return float(fx), float(fy), float(cx), float(cy)


def _poly_fisheye(theta, k):
    t2 = theta * theta
    return theta * (1. + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))


def _distort(model, k, x, y):
    """Normalised pinhole coordinates -> normalised coordinates in the raw picture (float64, vectorised)."""
    if model == 'pinhole':
        k1, k2, p1, p2, k3, k4, k5, k6 = k
        r2 = x * x + y * y
        kr = (1. + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1. + r2 * (k4 + r2 * (k5 + r2 * k6)))
        return (x * kr + 2. * p1 * x * y + p2 * (r2 + 2. * x * x),
                y * kr + p1 * (r2 + 2. * y * y) + 2. * p2 * x * y)
    r = np.sqrt(x * x + y * y)
    theta = np.arctan(r)
    with np.errstate(invalid='ignore', divide='ignore'):
        scale = np.where(r > 0, _poly_fisheye(theta, k) / r, 1.)
    return x * scale, y * scale


def _undistort(model, k, xd, yd):
    """The inverse of `_distort`, iteratively: normalised raw coordinates -> normalised pinhole coordinates."""
    if model == 'pinhole':
        k1, k2, p1, p2, k3, k4, k5, k6 = k
        x, y = xd.copy(), yd.copy()
        for _ in range(MAX_ITER):                       # fixed-point iteration (cv2.undistortPoints')
            r2 = x * x + y * y
            icd = (1. + r2 * (k4 + r2 * (k5 + r2 * k6))) / (1. + r2 * (k1 + r2 * (k2 + r2 * k3)))
            nx = (xd - (2. * p1 * x * y + p2 * (r2 + 2. * x * x))) * icd
            ny = (yd - (p1 * (r2 + 2. * y * y) + 2. * p2 * x * y)) * icd
            step = max(np.max(np.abs(nx - x), initial=0.), np.max(np.abs(ny - y), initial=0.))
            x, y = nx, ny
            if not step >= STEP_TOL:
                break
        return x, y
    rd = np.sqrt(xd * xd + yd * yd)
    theta = rd.copy()
    for _ in range(MAX_ITER):                           # Newton on theta: theta (1 + k1 theta^2 + ...) = rd
        t2 = theta * theta
        f = _poly_fisheye(theta, k) - rd
        df = 1. + t2 * (3. * k[0] + t2 * (5. * k[1] + t2 * (7. * k[2] + t2 * 9. * k[3])))
        d = f / df
        theta = theta - d
        if not np.max(np.abs(d), initial=0.) >= STEP_TOL:
            break
    with np.errstate(invalid='ignore', divide='ignore'):
        scale = np.where(rd > 0, np.tan(theta) / rd, 1.)
    return xd * scale, yd * scale


class LensMap:
    """A correction map for frames of `src_size` = (sw, sh), giving frames of `dst_size` = (dw, dh).

    xy: int32 (dh, dw, 2), the quantised source coordinate of every destination pixel (module docstring); kept
    C-contiguous and read-only.  border: the BGR colour of everything the map takes from outside the source.
    One object per stream: the context compares the object a frame carries with the one it has set, and setting
    another one synchronises -- a setting that may change, not one to alternate per frame."""

    def __init__(self, xy, src_size, border=(0, 0, 0)):
        self.src_size = _size(src_size, 'source')
        if not isinstance(xy, np.ndarray) or xy.dtype != np.int32:
            raise ValueError('xy must be an int32 ndarray (quantise float maps with LensMap.from_arrays)')
        if xy.ndim != 3 or xy.shape[2] != 2 or xy.shape[0] < 1 or xy.shape[1] < 1:
            raise ValueError(f'xy must have shape (H, W, 2), not {xy.shape}')
        self.dst_size = _size(xy.shape[1::-1], 'destination')
        sw, sh = self.src_size
        x, y = xy[..., 0], xy[..., 1]
        if x.min() < OUTSIDE or y.min() < OUTSIDE or x.max() > ONE * (sw + 1) or y.max() > ONE * (sh + 1):
            raise ValueError(f'map entries must lie in [{OUTSIDE}, {ONE * (sw + 1)}] x [{OUTSIDE}, {ONE * (sh + 1)}]')
        self.border = _border(border)
        xy = np.array(xy, np.int32, order='C')          # (a copy: the caller's array may change, this one must not)
        xy.flags.writeable = False
        self.xy = xy
        self._model = None

    @classmethod
    def from_arrays(cls, map_x, map_y, src_size, border=(0, 0, 0)):
        """Float maps as cv2.remap takes them: map_x[v, u], map_y[v, u] = the source coordinate of destination pixel (u, v)."""
        return cls(quantise(map_x, map_y, src_size), src_size, border)

    @classmethod
    def _from_model(cls, model, camera_matrix, k, src_size, dst_size, new_camera_matrix, zoom, border):
        sw, sh = _size(src_size, 'source')
        dw, dh = _size(dst_size, 'destination')
        fx, fy, cx, cy = _intrinsics(camera_matrix)
        if new_camera_matrix is None:
            if not (np.isfinite(zoom) and zoom > 0):
                raise ValueError(f'zoom must be positive, not {zoom!r}')
            # the camera matrix carried to dst_size with the pixel-centre convention (a pixel's centre is at its index)
            new = (fx * dw / sw * zoom, fy * dh / sh * zoom, (cx + 0.5) * dw / sw - 0.5, (cy + 0.5) * dh / sh - 0.5)
        else:
            new = _intrinsics(new_camera_matrix, 'new_camera_matrix')
        model_t = (model, (fx, fy, cx, cy), tuple(float(v) for v in k), new)
        u, v = np.meshgrid(np.arange(dw, dtype=np.float64), np.arange(dh, dtype=np.float64))
        mx, my = cls._model_to_source(model_t, u, v)
        lens = cls(quantise(mx, my, (sw, sh)), (sw, sh), border)
        lens._model = model_t
        return lens

    @classmethod
    def pinhole(cls, camera_matrix, dist_coeffs, src_size, dst_size, new_camera_matrix=None, zoom=1.0, border=(0, 0, 0)):
        """The map cv2.initUndistortRectifyMap describes for R = I (float64): dist_coeffs = k1 k2 p1 p2 [k3 [k4 k5 k6]]
        (4, 5 or 8 entries).  camera_matrix / new_camera_matrix: 3x3 (fx, fy, cx, cy are read; no skew) or (fx, fy, cx, cy).
        Default new matrix: the camera matrix carried to dst_size, fx' = fx dw / sw zoom, cx' = (cx + 0.5) dw / sw - 0.5
        and the same for y; zoom < 1 shows more of the raw picture's edge, zoom > 1 less."""
        d = np.asarray(dist_coeffs, np.float64).reshape(-1)
        if d.size not in (4, 5, 8) or not np.all(np.isfinite(d)):
            raise ValueError(f'dist_coeffs must be 4, 5 or 8 finite numbers, not {d.size}')
        k = np.zeros(8)
        k[:d.size] = d
        return cls._from_model('pinhole', camera_matrix, k, src_size, dst_size, new_camera_matrix, zoom, border)

    @classmethod
    def fisheye(cls, camera_matrix, dist_coeffs, src_size, dst_size, new_camera_matrix=None, zoom=1.0, border=(0, 0, 0)):
        """The equidistant model (cv2.fisheye): theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8),
        dist_coeffs = k1 k2 k3 k4.  Other arguments as `pinhole`'s."""
        d = np.asarray(dist_coeffs, np.float64).reshape(-1)
        if d.size != 4 or not np.all(np.isfinite(d)):
            raise ValueError(f'dist_coeffs must be 4 finite numbers, not {d.size}')
        return cls._from_model('fisheye', camera_matrix, d, src_size, dst_size, new_camera_matrix, zoom, border)

    @classmethod
    def from_config(cls, cfg, src_size, dst_size):
        """The `"lens"` dictionary of stream_cfg: {"model": "pinhole" | "fisheye", "camera_matrix": ..., "dist_coeffs": ...,
        "new_camera_matrix": None, "zoom": 1.0, "border": [b, g, r]}."""
        cfg = dict(cfg)
        model = cfg.pop('model', 'pinhole')
        if model not in ('pinhole', 'fisheye'):
            raise ValueError(f'lens model {model!r}: "pinhole" or "fisheye"')
        args = dict(new_camera_matrix=cfg.pop('new_camera_matrix', None), zoom=cfg.pop('zoom', 1.0), border=cfg.pop('border', (0, 0, 0)))
        try:
            camera_matrix, dist_coeffs = cfg.pop('camera_matrix'), cfg.pop('dist_coeffs')
        except KeyError as err:
            raise ValueError(f'lens configuration needs {err.args[0]!r}') from None
        if cfg:
            raise ValueError(f'unknown lens settings {sorted(cfg)}')
        return getattr(cls, model)(camera_matrix, dist_coeffs, src_size, dst_size, **args)

    @staticmethod
    def _model_to_source(model_t, u, v):
        model, (fx, fy, cx, cy), k, (nfx, nfy, ncx, ncy) = model_t
        xd, yd = _distort(model, k, (u - ncx) / nfx, (v - ncy) / nfy)
        return fx * xd + cx, fy * yd + cy

    def _points(self, points):
        if self._model is None:
            raise ValueError('this LensMap was built from arrays: only LensMap.pinhole / LensMap.fisheye know their model')
        p = np.asarray(points, np.float64)
        if p.shape[-1:] != (2,):
            raise ValueError(f'points must have shape (..., 2), not {p.shape}')
        return p

    def to_source(self, points):
        """Corrected pixels (..., 2) as (x, y) -> raw pixels, in closed form: the function the map was built with
        (before quantisation).  Host only."""
        p = self._points(points)
        x, y = self._model_to_source(self._model, p[..., 0], p[..., 1])
        return np.stack([x, y], axis=-1)

    def to_destination(self, points):
        """Raw pixels (..., 2) as (x, y) -> corrected pixels: a fixed-point iteration (pinhole) or Newton on theta
        (fisheye) that stops at a step below 1e-12 in normalised units or after 100 iterations.  Host only."""
        p = self._points(points)
        model, (fx, fy, cx, cy), k, (nfx, nfy, ncx, ncy) = self._model
        x, y = _undistort(model, k, (p[..., 0] - cx) / fx, (p[..., 1] - cy) / fy)
        return np.stack([x * nfx + ncx, y * nfy + ncy], axis=-1)


def remap_bgr(frame, lens):
    """`frame` (uint8 (sh, sw, 3) of lens.src_size) through the map -> uint8 (dh, dw, 3): the module docstring's
    arithmetic in numpy, what csrc/remap.hip writes bit for bit."""
    if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError('frame must be uint8 HxWx3')
    sh, sw = frame.shape[:2]
    if (sw, sh) != lens.src_size:
        raise ValueError(f'frame is {sw}x{sh}, the lens map is for {lens.src_size[0]}x{lens.src_size[1]}')
    X, Y = lens.xy[..., 0], lens.xy[..., 1]
    ix, iy = X >> FRAC_BITS, Y >> FRAC_BITS
    fx, fy = (X & (ONE - 1))[..., None], (Y & (ONE - 1))[..., None]
    border = np.array(lens.border, np.int32)

    def tap(x, y):
        inside = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
        p = frame[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)].astype(np.int32)
        return np.where(inside[..., None], p, border)

    top = (ONE - fx) * tap(ix, iy) + fx * tap(ix + 1, iy)
    bot = (ONE - fx) * tap(ix, iy + 1) + fx * tap(ix + 1, iy + 1)
    return (((ONE - fy) * top + fy * bot + 512) >> 10).astype(np.uint8)


def remap_bgr_host(frame, lens):
    """`remap_bgr` by the compiled twin of the kernel (fm_remap_bgr_host, csrc/remap_host.hip).  No GPU."""
    import ctypes as C
    from .._lib import check, load
    if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError('frame must be uint8 HxWx3')
    frame = np.ascontiguousarray(frame)
    sh, sw = frame.shape[:2]
    if (sw, sh) != lens.src_size:
        raise ValueError(f'frame is {sw}x{sh}, the lens map is for {lens.src_size[0]}x{lens.src_size[1]}')
    dw, dh = lens.dst_size
    out = np.empty((dh, dw, 3), np.uint8)
    addr = lambda a: C.c_void_p(a.__array_interface__['data'][0])
    check(load().fm_remap_bgr_host(addr(frame), C.c_int(sw), C.c_int(sh), addr(lens.xy), addr(out), C.c_int(dw), C.c_int(dh),
                                   (C.c_uint8 * 3)(*lens.border)))
    return out
