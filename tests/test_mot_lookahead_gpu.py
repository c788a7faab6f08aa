"""GPU: MOT(detector_lookahead=k) -- one detector pass over the next k frames -- gives the tracks of strictly sequential
steps, frame by frame (modelled on test_mot_gpu.py::test_next_frame_prefetch_changes_nothing); track_stream with
read-ahead writes the same MOT rows."""
import io
from types import SimpleNamespace

import pytest

import scenes

pytestmark = pytest.mark.gpu


def build_mot(size, video, lookahead, real=False):
    import fastmot_amd.mot as mot_mod
    from fastmot_amd.models import YOLO
    from synthetic import InjectedYOLODetector, scripted_head_weights

    class LookaheadTiny(YOLO):
        NUM_CLASSES = 2
        INPUT_SHAPE = (3, 160, 288)
        LAYER_FACTORS = [8, 16, 32]
        SCALES = [1.2, 1.1, 1.05]
        ANCHORS = [[4, 7, 8, 15, 12, 30], [18, 40, 25, 60, 30, 80], [40, 90, 60, 70, 80, 95]]
    cfg = dict(model='LookaheadTiny', conf_thresh=0.25, nms_thresh=0.5, max_area=800000, min_aspect_ratio=1.2)
    if real:        # the tracker is fed the network's own detections (heads scripted so that NMS has work)
        cfg['weights'] = scripted_head_weights(size, 'LookaheadTiny', 1, video.frames[0], 200)
    else:
        mot_mod.YOLODetector = InjectedYOLODetector
    try:
        mot = mot_mod.MOT(size, detector_type='YOLO', detector_frame_skip=1, class_ids=(1,),
                          yolo_detector_cfg=SimpleNamespace(**cfg),
                          feature_extractor_cfgs=(SimpleNamespace(model='OSNet025', batch_size=16),),
                          tracker_cfg=SimpleNamespace(**scenes.tracker_kwargs()), detector_lookahead=lookahead)
    finally:
        from fastmot_amd.detector import YOLODetector
        mot_mod.YOLODetector = YOLODetector
    if not real:
        mot.detector.bind_video(video)
    return mot


def run_steps(ctx, mot, frames, lookahead):
    from fastmot_amd import Track
    Track._count = 0
    mot.reset(1 / 30.)
    rows = []
    for f in range(len(frames)):
        if hasattr(mot.detector, '_frame_idx'):
            mot.detector._frame_idx = f
        if lookahead > 1:
            mot.step(frames[f], next_frames=frames[f + 1:f + 1 + lookahead])
        else:
            mot.step(frames[f])
        rows.append([(t.trk_id, tuple(t.tlbr), t.confirmed, t.active, t.age, t.hits)
                     for t in mot.tracker.tracks.values()])
    mot.tracker._clear_tracks()
    return rows


@pytest.mark.parametrize('resident', [False, True])
def test_lookahead_changes_nothing(ctx, resident):
    from synthetic import SyntheticVideo
    from fastmot_amd.detector import DeviceFrame
    size = (960, 540)
    video = SyntheticVideo(size, n_ids=10, n_frames=13, seed=11)      # 13 frames: odd tails for k = 2 and 3
    if resident:
        ctx.frame_configure(size[0], size[1], video.n_frames)
        for i, fr in enumerate(video.frames):
            ctx.frame_ring_store(i, fr)
        frames = [DeviceFrame(i) for i in range(video.n_frames)]
    else:
        frames = video.frames
    ref = run_steps(ctx, build_mot(size, video, 1), frames, 1)
    assert len(ref[-1]) >= 8
    for k in (2, 3):
        mot = build_mot(size, video, k)
        assert mot.detector.max_batch == k
        assert run_steps(ctx, mot, frames, k) == ref, k


def test_lookahead_with_the_networks_own_detections(ctx):
    from synthetic import SyntheticVideo
    size = (960, 540)
    video = SyntheticVideo(size, n_ids=10, n_frames=9, seed=12)
    ref = run_steps(ctx, build_mot(size, video, 1, real=True), video.frames, 1)
    assert sum(len(r) for r in ref) > 0
    assert run_steps(ctx, build_mot(size, video, 2, real=True), video.frames, 2) == ref


class _Stream:
    def __init__(self, frames, size):
        self.frames, self.resolution, self.i = frames, size, 0

    def read(self):
        self.i += 1
        return self.frames[self.i - 1] if self.i <= len(self.frames) else None


def test_track_stream_lookahead_writes_the_same_rows(ctx):
    from synthetic import SyntheticVideo
    from fastmot_amd import Track
    from fastmot_amd.readahead import track_stream
    size = (960, 540)
    video = SyntheticVideo(size, n_ids=10, n_frames=11, seed=13)
    out = []
    for k in (1, 2):
        mot = build_mot(size, video, k)
        Track._count = 0
        mot.reset(1 / 30.)
        mot.detector._frame_idx = 0
        txt = io.StringIO()
        assert track_stream(_Stream(video.frames, size), mot, txt=txt, resize_to=size, lookahead=k) == video.n_frames
        mot.tracker._clear_tracks()
        out.append(txt.getvalue())
    assert out[0] == out[1] and out[0].count('\n') > 20
