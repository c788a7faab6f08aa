"""MOT: the per-frame orchestrator (API of fastmot/mot.py:25-196).

Same stage schedule as the reference's MOT.step (mot.py:125-168) -- detector enqueue || KLT,
extractor enqueue || Kalman, then association -- but every stage is a set of kernels on its own HIP
stream of one shared device context, and the frame is uploaded once per step (or is already
resident: pass a detector.DeviceFrame)."""
from types import SimpleNamespace
from enum import Enum
import logging
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from .detector import SSDDetector, YOLODetector, PublicDetector, bind_frame, check_tiling
from .feature_extractor import FeatureExtractor
from .tracker import MultiTracker
from .flow import Flow
from .utils import Profiler
from .utils.source import SourceFrame
from .utils.visualization import Visualizer
from .utils.overlay import build_commands
from collections import namedtuple

from .utils.redact import Redact, build_regions, redact_bgr, region_rect, clip_rect, part_fractions

LOGGER = logging.getLogger(__name__)
# One entry of MOT.encode_objects: the track's id and label, the clipped frame rectangle (x0, y0, x1, y1, inclusive) the
# picture shows, the JPEG's (w, h) and the file's bytes
ObjectImage = namedtuple('ObjectImage', 'trk_id label rect size data')
_NATIVE_FLOW = True      # tests flip this to compare the native prediction worker with the Python-thread path


class _NativeFlowJob:
    """Future-like handle of MultiTracker.predict_async (same interface as the thread-pool future it replaces)."""

    def __init__(self, tracker, frame):
        self._tracker = tracker
        self._job = tracker.predict_async(frame)

    def result(self):
        job, self._job = self._job, None
        if job is not None:
            with Profiler('track'):
                self._tracker.predict_finish(job)


class DetectorLookahead:
    """Schedule of the detector look-ahead (MOT(detector_lookahead=k)): which upcoming frames a step hands to the
    detector as one batched pass.  A pass over frames t+1..t+k starts whenever none of the frames announced before is
    still to come; near the end of a sequence the batch is what is left.  A step whose frame is not the next announced
    one makes the announced frames stale (the detector drops their results)."""

    def __init__(self, k):
        self.k = k
        self.announced = []

    def consume(self, frame):
        """Called with the frame of each step; True when its detector pass was announced (already enqueued)."""
        if self.announced and self.announced[0] is frame:
            self.announced.pop(0)
            return True
        self.announced = []
        return False

    def to_enqueue(self, upcoming):
        """The frames (of `upcoming`, the next frames in order) to start one pass on in this step, or []."""
        if self.announced or not upcoming:
            return []
        self.announced = list(upcoming[:self.k])
        return list(self.announced)


class DetectorType(Enum):
    SSD = 0
    YOLO = 1
    PUBLIC = 2


class MOT:
    def __init__(self, size,
                 detector_type='YOLO',
                 detector_frame_skip=5,
                 class_ids=(1,),
                 ssd_detector_cfg=None,
                 yolo_detector_cfg=None,
                 public_detector_cfg=None,
                 feature_extractor_cfgs=None,
                 tracker_cfg=None,
                 visualizer_cfg=None,
                 draw=False,
                 detector_lookahead=1,
                 gpu_draw=False,
                 redact=None):
        """Top level module that integrates detection, feature extraction and tracking
        (parameters: fastmot/mot.py:37-67).  `draw=True` renders the overlays of `visualizer_cfg` onto every
        frame handed to `step` as a host ndarray, in place, after tracking (mot.py:166-167,191-196).
        `detector_lookahead=k` (not in the reference; YOLO with detector_frame_skip 1 only): the detector runs one
        network pass over the next k frames handed to `step` as `next_frames` (DetectorLookahead); results unchanged.
        `gpu_draw=True` (not in the reference; excludes `draw`): the same overlays, rendered on the GPU onto a COPY of the
        frame the tracker holds there -- whatever the frame was handed over as -- when `render_frame` or `encode_frame`
        asks for them; `step` itself draws nothing and the frame handed to it is not touched.
        `redact` (not in the reference; None, a utils.redact.Redact, or a dictionary of its settings -- `"redact": {...}`
        in `mot_cfg`): the tracked objects are pixelated, smoothed or painted over in EVERY picture this object hands out:
        `render_frame()`, `encode_frame()`, `export_frame_i420()` and `encode_objects()` always return the redacted picture
        (`overlays=False` then means "redacted, nothing drawn"; the object crops are cut from the redacted picture, never
        from the tracker's frame), made on the GPU inside the overlay pass (csrc/redact.hip, csrc/overlay.hip);
        with `draw=True` the host frame is redacted in place before the overlays are drawn on it.  The regions are this
        step's detections and every active track, confirmed or not (utils.redact.Redact says how boxes become regions).
        NOT covered, by design: `tracker.ctx.frame_read()`, the caller's own frame (unless `draw=True` writes it) and
        the ReID crops are the unredacted picture -- the tracker must see it, and its results do not change.  A region
        list the library refuses (more than 4096 regions or 2^20 cells) raises: no picture leaves unredacted."""
        if draw and gpu_draw:
            raise ValueError('draw=True renders on the host frame, gpu_draw=True on the GPU copy: choose one')
        self.gpu_draw = gpu_draw
        self.redact = Redact.coerce(redact)
        self._overlay_rendered = False      # False, or which picture the overlay buffer holds: True (drawn) / 'bare'
        self._redact_regions = None
        self.size = size
        self.detector_type = DetectorType[detector_type.upper()]
        assert detector_frame_skip >= 1
        if detector_lookahead != 1:
            if not 1 <= detector_lookahead <= _lib.FM_MAX_DET_BATCH:
                raise ValueError(f'detector_lookahead must be 1..{_lib.FM_MAX_DET_BATCH}')
            if self.detector_type != DetectorType.YOLO:
                raise ValueError('detector_lookahead > 1 needs the YOLO detector')
            if detector_frame_skip != 1:
                raise ValueError('detector_lookahead > 1 needs detector_frame_skip == 1')
        if self.detector_type == DetectorType.YOLO and yolo_detector_cfg is not None:
            # (a tiled YOLO detector uses the batch dimension for its tiles: checked here, before anything is built)
            check_tiling(getattr(yolo_detector_cfg, 'tiling_grid', (1, 1)), detector_lookahead=detector_lookahead)
        self.detector_lookahead = detector_lookahead
        self._lookahead = DetectorLookahead(detector_lookahead)
        self.detector_frame_skip = detector_frame_skip
        self.class_ids = tuple(np.unique(class_ids))
        self.draw = draw

        if ssd_detector_cfg is None:
            ssd_detector_cfg = SimpleNamespace()
        if yolo_detector_cfg is None:
            yolo_detector_cfg = SimpleNamespace()
        if public_detector_cfg is None:
            public_detector_cfg = SimpleNamespace()
        if feature_extractor_cfgs is None:
            feature_extractor_cfgs = (SimpleNamespace(),)
        if tracker_cfg is None:
            tracker_cfg = SimpleNamespace()
        if visualizer_cfg is None:
            visualizer_cfg = SimpleNamespace()
        if len(feature_extractor_cfgs) != len(class_ids):
            raise ValueError('Number of feature extractors must match length of class IDs')
        self.visualizer = Visualizer(**vars(visualizer_cfg))

        LOGGER.info('Loading detector model...')
        if self.detector_type == DetectorType.SSD:
            self.detector = SSDDetector(self.size, self.class_ids, **vars(ssd_detector_cfg))
        elif self.detector_type == DetectorType.YOLO:
            extra = {'max_batch': detector_lookahead} if detector_lookahead > 1 else {}
            self.detector = YOLODetector(self.size, self.class_ids, **vars(yolo_detector_cfg), **extra)
        elif self.detector_type == DetectorType.PUBLIC:
            self.detector = PublicDetector(self.size, self.class_ids, self.detector_frame_skip,
                                           **vars(public_detector_cfg))

        LOGGER.info('Loading feature extractor models...')
        self.extractors = [FeatureExtractor(size=self.size, resident=(i == 0), **vars(cfg))
                           for i, cfg in enumerate(feature_extractor_cfgs)]
        self.tracker = MultiTracker(self.size, self.extractors[0].metric, **vars(tracker_cfg))
        self.frame_count = 0
        self._next_frame = None
        self._next_frames = []
        # KLT + Kalman run on a second host thread while this one drives detector -> ReID network (the
        # C-ABI calls release the GIL; the stages use separate HIP streams and share no state)
        self._flow_thread = ThreadPoolExecutor(max_workers=1, thread_name_prefix='fastmot-flow',
                                               initializer=self.tracker.ctx.bind_thread)

    def visible_tracks(self):
        """Confirmed and active tracks (iterator of Track)."""
        return (track for track in self.tracker.tracks.values()
                if track.confirmed and track.active)

    def reset(self, cap_dt):
        """Resets multiple object tracker. Must be called before `step`."""
        self.frame_count = 0
        self.tracker.reset(cap_dt)

    def step(self, frame, next_frame=None, next_frames=None):
        """Runs multiple object tracker on the next frame (ndarray HxWx3 uint8 BGR, an NV12Frame, a PlanarFrame, a PackedFrame, a BayerFrame, a DeepFrame or a JPEGFrame -- converted to BGR
        on the GPU while it is uploaded --, a DeviceArrayFrame -- a torch / CuPy tensor or a decoder surface that lies in
        GPU memory already: converted where it lies, nothing crosses PCIe; it may be dropped right after the step, not
        overwritten before its `done()` --, a SourceFrame -- any of them at capture resolution, resized to `size` on
        the GPU --, or a detector.DeviceFrame that is already resident on the GPU).

        next_frame (optional, not in the reference): the frame the following `step` will receive, when
        the caller already has it (file sources, a capture queue).  The detector network is then started
        on it right behind this frame's own pass, so that it overlaps this frame's KLT, ReID and association
        stages; results are unchanged (the detector is stateless), per-frame latency too.
        next_frames (optional): the frames of the following steps in order (next_frame = next_frames[0]); with
        detector_lookahead = k the detector takes up to k of them in one network pass."""
        ctx = self.tracker.ctx
        if self.draw and isinstance(frame, SourceFrame):
            raise ValueError('draw=True needs host pixels at the tracker\'s size: a SourceFrame is resized on the GPU')
        bind_frame(ctx, frame, self.size, begin_step=True)
        self._overlay_rendered = False
        self._redact_regions = None
        ctx.in_step = True
        if next_frames is not None:
            next_frames = list(next_frames)
            if next_frame is None and next_frames:
                next_frame = next_frames[0]
        self._next_frame = next_frame
        self._next_frames = next_frames if next_frames is not None else ([] if next_frame is None else [next_frame])
        if self.detector_lookahead > 1:
            self._lookahead.consume(frame)
        try:
            self._step(frame)
        finally:
            ctx.in_step = False
            self._next_frame = None
            self._next_frames = []
        if self.draw:
            if self.redact is not None:
                if not isinstance(frame, np.ndarray):
                    raise TypeError('draw=True needs host frames (ndarray): overlays are rendered on the CPU')
                redact_bgr(frame, self._regions())
            self._draw(frame, self._last_detections)
        self.frame_count += 1

    def encode_frame(self, quality=75, overlays=None):
        """The frame of the last `step` as the bytes of a baseline JPEG file (YCbCr 4:2:0; utils.jpeg.encode_bgr's format
        and arithmetic), encoded from the copy the tracker used on the GPU -- whatever the frame was handed over as:
        ndarray, NV12Frame, JPEGFrame, SourceFrame (the resized frame), DeviceFrame.  Nothing is uploaded, the step's
        results and the frames prefetched for the next steps are untouched.  `overlays` (default: `gpu_draw`): encode the
        frame with the overlays of `render_frame` on it instead of the bare frame.  (`draw=True` renders on the host copy:
        write that one, VideoIO(gpu_encode=True) encodes it on the GPU as well.)"""
        if not 1 <= int(quality) <= 100:
            raise ValueError(f'quality {quality} outside 1..100')
        if self.frame_count == 0:
            raise RuntimeError('encode_frame needs a step before it')
        drawn = self.gpu_draw if overlays is None else overlays
        if drawn or self.redact is not None:
            self._render_overlay(drawn)
            return self.tracker.ctx.overlay_encode_jpeg(quality)
        return self.tracker.ctx.frame_encode_jpeg(quality)

    def export_frame_i420(self, overlays=None):
        """The frame of the last `step` as an utils.yuv.I420Image -- planar 4:2:0 bytes, the payload of a Y4M frame
        (VideoIO.write takes it for a '.y4m' output) --, converted from the copy the tracker used on the GPU
        (csrc/yuv.hip; utils.yuv.bgr_to_planar420's arithmetic): 1.5 bytes per pixel come back, nothing is uploaded.
        `overlays` (default: `gpu_draw`): the picture with the overlays of `render_frame` on it, as `encode_frame`
        chooses.  Valid until the next `step`."""
        from .utils.yuv import I420Image
        if self.frame_count == 0:
            raise RuntimeError('export_frame_i420 needs a step before it')
        ctx = self.tracker.ctx
        drawn = self.gpu_draw if overlays is None else overlays
        if drawn or self.redact is not None:
            self._render_overlay(drawn)
            return I420Image(ctx.overlay_export_i420(), self.size)
        return I420Image(ctx.frame_export_i420(), self.size)

    def encode_objects(self, quality=85, part='box', margin=0.0, shrink=1, confirmed=True, classes=None, overlays=None):
        """One small JPEG per tracked object of the last `step` -> list of ObjectImage(trk_id, label, rect, size, data), in
        `tracker.tracks` order: an alarm thumbnail, a gallery image, a row of an event database.  All crops of the frame
        are encoded in ONE pass of the GPU encoder from the frame the tracker holds there (ctx.frame_encode_regions;
        csrc/jpegenc.hip): nothing is uploaded, only compressed bytes come back, the step's results and the frames
        prefetched for the next steps are untouched.  `data` equals utils.jpeg.encode_bgr of the crop.

        confirmed  True (default): the visible tracks (confirmed and active); False: every active track.
        classes    labels to include (default None: every label).
        part, margin  which part of a track's box is shown, as in utils.redact.Redact: 'box' (default), 'head' (the upper
                   quarter, middle half: face-sized crops) or four fractions of the box; `margin` (default 0) widens it on
                   every side.  The rectangle (utils.redact.region_rect) is clipped to the frame; a track whose rectangle
                   misses the frame is omitted.
        shrink     1 (default), 2 or 4: the crop is reduced by that factor first (block means); `size` says what came out.
        overlays   (default: `gpu_draw`) crop the picture with the overlays of `render_frame` on it.  With
                   MOT(redact=...) the crops are ALWAYS cut from the redacted picture, as `encode_frame` decides.
        RuntimeError before the first step, ValueError for a bad quality, shrink, part or margin.  Valid until the next `step`."""
        if not 1 <= int(quality) <= 100:
            raise ValueError(f'quality {quality} outside 1..100')
        if shrink not in _lib.OBJENC_SHRINKS:
            raise ValueError(f'shrink {shrink!r}: one of {_lib.OBJENC_SHRINKS}')
        fractions = part_fractions(part)
        if not 0 <= float(margin) <= 4:
            raise ValueError('margin outside 0..4')
        if self.frame_count == 0:
            raise RuntimeError('encode_objects needs a step before it')
        classes = None if classes is None else frozenset(int(v) for v in classes)
        picked = []
        for track in self.tracker.tracks.values():
            if not track.active or (confirmed and not track.confirmed) or (classes is not None and int(track.label) not in classes):
                continue
            rect = clip_rect(region_rect(track.tlbr, fractions, float(margin), self.size), self.size)
            if rect is not None:
                picked.append((track, rect))
        drawn = self.gpu_draw if overlays is None else overlays
        from_overlay = bool(drawn or self.redact is not None)
        if from_overlay:
            self._render_overlay(drawn)
        files = self.tracker.ctx.frame_encode_regions(np.array([r for _, r in picked], np.int32).reshape(-1, 4), int(quality),
                                                      shrink, overlay=from_overlay)
        return [ObjectImage(track.trk_id, int(track.label), rect,
                            (-(-(rect[2] - rect[0] + 1) // shrink), -(-(rect[3] - rect[1] + 1) // shrink)), data)
                for (track, rect), data in zip(picked, files)]

    def render_frame(self):
        """The frame of the last `step` with the overlays of `visualizer_cfg` on it, as an HxWx3 uint8 BGR ndarray: what
        `draw=True` leaves in a host frame, rendered on the GPU (csrc/overlay.hip) from the state the step left, onto a
        copy of the frame the tracker holds there.  Works for every frame kind; the tracker's frame and the caller's
        array are not written.  Valid until the next `step`, like `encode_frame`; the list is built and rendered once
        per step, by whichever of the two comes first."""
        if self.frame_count == 0:
            raise RuntimeError('render_frame needs a step before it')
        self._render_overlay()
        return self.tracker.ctx.overlay_read()

    def redact_frame(self, frame):
        """Redacts a host frame of the tracker's size (HxWx3 uint8 BGR, e.g. the caller's copy of the frame of the last
        `step`) IN PLACE with that step's regions, on the CPU (utils.redact.redact_bgr), and returns it: for a caller that
        writes its own array instead of asking for `render_frame()` / `encode_frame()`."""
        if self.redact is None:
            raise RuntimeError('redact_frame needs MOT(redact=...)')
        if self.frame_count == 0:
            raise RuntimeError('redact_frame needs a step before it')
        if not isinstance(frame, np.ndarray) or frame.shape[:2] != (self.size[1], self.size[0]):
            raise ValueError(f'redact_frame needs an ndarray of the tracker\'s size {self.size[0]}x{self.size[1]}')
        return redact_bgr(frame, self._regions())

    def _regions(self):
        """The redaction regions of the last step: built once per step, from the state the step left."""
        if self._redact_regions is None:
            self._redact_regions = build_regions(self.tracker.tracks.values(), self._last_detections, self.redact, self.size)
        return self._redact_regions

    def _render_overlay(self, drawn=True):
        """Fills the context's overlay buffer: with the overlays (`drawn`), or -- only with `redact` -- with the redacted
        frame and nothing drawn on it."""
        want = True if drawn else 'bare'
        if self._overlay_rendered == want:
            return
        cmds, masks = (), b''
        if drawn:
            visible = list(self.visible_tracks())
            cmds, masks = build_commands(self.visualizer, visible, self._last_detections, self.tracker.klt_bboxes.values(),
                                         self.tracker.flow.prev_bg_keypoints, self.tracker.flow.bg_keypoints,
                                         f'visible: {len(visible)}', self.size)
        if self.redact is not None:
            self.tracker.ctx.frame_render_redacted(self._regions(), cmds, masks)
        else:
            self.tracker.ctx.frame_render_overlay(cmds, masks)
        self._overlay_rendered = want

    def _prefetch_next(self):
        if self.detector_lookahead > 1:
            batch = self._lookahead.to_enqueue(self._next_frames)
            self._next_frame, self._next_frames = None, []
            if len(batch) > 1:
                self.detector.prefetch_batch(batch)
            elif batch:
                self.detector.prefetch(batch[0])
            return
        nxt = self._next_frame
        if nxt is not None and (self.frame_count + 1) % self.detector_frame_skip == 0:
            self._next_frame = None
            self.detector.prefetch(nxt)

    def _step(self, frame):
        self._last_detections = []          # what _draw shows: this frame's detections, none on skipped frames
        if self.frame_count == 0:
            detections = self._last_detections = self.detector(frame)
            self._prefetch_next()
            self.tracker.init(frame, detections)
        elif self.frame_count % self.detector_frame_skip == 0:
            with Profiler('preproc'):
                self.detector.detect_async(frame)

            # Same stages as mot.py:138-161.  The reference overlaps its CPU optical flow with the
            # asynchronous TensorRT detector and its Kalman step with the ReID network; here the whole
            # KLT + Kalman chain (device pyramid / keypoints / LK, host RANSAC, Kalman launch) runs on a
            # second host thread and its own HIP streams, so the critical path of a step is
            # detector -> ReID network -> association.  The stages are independent exactly as in the
            # reference, so the results are identical.
            # next_frame known: its upload and detector pass are queued right behind this frame's pass (the detector
            # stream never idles; results are collected in order, detect.hip) -- and BEFORE the KLT job is started: the
            # detector chain is the longest of a step, and with the worker thread's launches in front of it the copy
            # and the pass reached the GPU late and at varying times (779 +- 70 -> 872 +- 25 frames/s over 8 runs each)
            self._prefetch_next()
            native = _NATIVE_FLOW and type(self.tracker.flow) is Flow      # (tests script the flow with a fake)
            if native:
                # KLT + Kalman on the library's worker thread: marshalled here, scattered in predict_finish -- no second
                # Python thread competing for the interpreter lock (fastmot_hip.h: fm_track_predict_async)
                flow_done = _NativeFlowJob(self.tracker, frame)
            else:
                flow_done = self._flow_thread.submit(self._flow_and_kalman, frame)
            try:
                with Profiler('detect'):
                    detections = self._last_detections = self.detector.postprocess()

                with Profiler('extract'):
                    if len(self.extractors) == 1:
                        self.extractors[0].extract_async(frame, detections.tlbr)
                    else:
                        # one extractor per class id (mot.py:147-157); _split_bboxes_by_cls keeps the
                        # reference's bisect_right, quirk included
                        cls_bboxes = self._split_bboxes_by_cls(detections.tlbr, detections.label, self.class_ids)
                        for extractor, bboxes in zip(self.extractors, cls_bboxes):
                            extractor.extract_async(frame, bboxes)
                    self.tracker.prepare_detections(detections)
                    # the embedding-independent part of the association (track grouping, cost-matrix row order,
                    # packed launch arguments) runs while the ReID network is still busy: it only needs the Kalman
                    # step, i.e. the KLT thread, to have finished
                    flow_done.result()
                    # exactly one extractor holds all of this frame's boxes (always so with one class; with several,
                    # whenever _split_bboxes_by_cls hands every box to the first): the pairwise-cost kernel of the
                    # association is enqueued now, behind the ReID network on the device (tracker.update_begin)
                    busy = [e for e in self.extractors if getattr(e, 'last_num_features', 0)]
                    in_flight = len(busy) == 1 and busy[0].last_num_features == len(detections) and \
                        getattr(busy[0], '_pending', False)
                    pre = self.tracker.update_begin(detections, embeddings_in_flight=in_flight)
                    if len(self.extractors) == 1:
                        embeddings = self.extractors[0].postprocess()
                    else:
                        parts = [extractor.postprocess() for extractor in self.extractors]
                        filled = [p for p in parts if len(p)]
                        # (a single non-empty part is passed through as it is: the association kernels then
                        # read the device-resident copy; the reference's np.concatenate with its float64 empty
                        # parts only changes the dtype of the same values)
                        embeddings = filled[0] if len(filled) == 1 else np.concatenate(parts)
            finally:
                flow_done.result()

            with Profiler('assoc'):
                self.tracker.update(self.frame_count, detections, embeddings, pre=pre)
        else:
            self._prefetch_next()
            with Profiler('track'):
                self.tracker.track(frame)

    @staticmethod
    def _bisect_right(arr, val, left=0):
        """fastmot/utils/numba.py:43-53, verbatim semantics: the test is `arr[mid] >= val` (not `>`), so on
        the ascending label array every probe moves `left` -- the search returns len(arr) whenever
        val <= arr[left:] (always true for the first class id, the labels being restricted to class_ids)."""
        right = len(arr)
        while left < right:
            mid = left + (right - left) // 2
            if arr[mid] >= val:
                left = mid + 1
            else:
                right = mid
        return left

    @classmethod
    def _split_bboxes_by_cls(cls, bboxes, labels, class_ids):
        """mot.py:180-189.  With the reference's bisect_right every box goes to the FIRST class's extractor
        and the others receive empty slices; reproduced, not repaired, so that embeddings (and with them the
        association) equal the reference's."""
        cls_bboxes = []
        begin = 0
        labels = np.asarray(labels).tolist()
        for cls_id in class_ids:
            end = cls._bisect_right(labels, cls_id, begin)
            cls_bboxes.append(bboxes[begin:end])
            begin = end
        return cls_bboxes

    def _draw(self, frame, detections):
        if not isinstance(frame, np.ndarray):
            raise TypeError('draw=True needs host frames (ndarray): overlays are rendered on the CPU')
        visible = list(self.visible_tracks())
        self.visualizer.render(frame, visible, detections, self.tracker.klt_bboxes.values(),
                               self.tracker.flow.prev_bg_keypoints, self.tracker.flow.bg_keypoints,
                               caption=f'visible: {len(visible)}')

    def _flow_and_kalman(self, frame):
        with Profiler('track'):
            self.tracker.compute_flow(frame)
            self.tracker.apply_kalman()

    @staticmethod
    def print_timing_info():
        LOGGER.debug('=================Timing Stats=================')
        LOGGER.debug(f"{'track time:':<37}{Profiler.get_avg_millis('track'):>6.3f} ms")
        LOGGER.debug(f"{'preprocess time:':<37}{Profiler.get_avg_millis('preproc'):>6.3f} ms")
        LOGGER.debug(f"{'detect/flow time:':<37}{Profiler.get_avg_millis('detect'):>6.3f} ms")
        LOGGER.debug(f"{'feature extract/kalman filter time:':<37}"
                     f"{Profiler.get_avg_millis('extract'):>6.3f} ms")
        LOGGER.debug(f"{'association time:':<37}{Profiler.get_avg_millis('assoc'):>6.3f} ms")
