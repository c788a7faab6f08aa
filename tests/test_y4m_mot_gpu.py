"""GPU: a '.y4m' file through VideoIO and MOT.step -- planar frames converted on the GPU (gpu_decode) against the same
file converted on the host, and a '.y4m' output written from the frames and overlays that live on the GPU (gpu_encode)."""
import numpy as np
import pytest

from fastmot_amd import PlanarFrame, VideoIO
from fastmot_amd.utils.yuv import I420Image, bgr_to_planar420, fps_ratio, planar_to_bgr, y4m_header

pytestmark = pytest.mark.gpu

SIZE = (960, 540)          # the smallest size the MOT tests run the tracker at


@pytest.fixture(scope='module')
def clip(tmp_path_factory):
    from synthetic import SyntheticVideo
    video = SyntheticVideo(SIZE, n_ids=8, n_frames=8, seed=4)
    path = tmp_path_factory.mktemp('y4m') / 'clip.y4m'
    with open(path, 'wb') as f:
        f.write(y4m_header(*SIZE, fps_ratio(30)))
        for frame in video.frames:
            f.write(b'FRAME\n')
            for plane in bgr_to_planar420(frame):
                f.write(plane.tobytes())
    return video, path


def fresh_mot(video):
    from fastmot_amd import Track
    from test_mot_gpu import build_mot
    mot = build_mot(SIZE, video, 1)
    Track._count = 0
    mot.reset(1 / 30.)
    return mot


def test_tracks_on_planar_frames_equal_host_converted_frames(ctx, clip):
    video, path = clip
    runs = {}
    for gpu in (True, False):
        stream = VideoIO(SIZE, str(path), buffer_size=4, gpu_decode=gpu)
        assert stream.cap_fps == 30
        stream.start_capture()
        mot = fresh_mot(video)
        rows = []
        try:
            for f in range(video.n_frames):
                frame = stream.read()
                assert isinstance(frame, PlanarFrame if gpu else np.ndarray)
                mot.detector._frame_idx = f
                mot.step(frame)
                rows.append([(t.trk_id, tuple(t.tlbr), t.confirmed, t.active, t.age, t.hits) for t in mot.tracker.tracks.values()])
            assert stream.read() is None
        finally:
            stream.release()
            mot.tracker._clear_tracks()
        runs[gpu] = rows
    assert runs[True] == runs[False]
    assert len(runs[False][-1]) >= 6


def test_y4m_output_from_gpu_only_frames(ctx, clip, tmp_path):
    from fastmot_amd.readahead import track_stream
    video, path = clip
    out = tmp_path / 'out.y4m'
    stream = VideoIO(SIZE, str(path), str(out), buffer_size=4, gpu_decode=True, gpu_encode=True)
    stream.start_capture()
    mot = fresh_mot(video)
    mot.gpu_draw = True
    want, kinds, bare = [], [], []

    class Spy:                                       # the stream, recording what is read and what the written picture must be
        resolution, gpu_encode, jpeg_quality, i420_output = stream.resolution, stream.gpu_encode, stream.jpeg_quality, stream.i420_output

        @staticmethod
        def read():
            frame = stream.read()
            kinds.append(type(frame))
            return frame

        @staticmethod
        def write(image):
            assert isinstance(image, I420Image) and image.size == SIZE
            want.append(planar_to_bgr(*bgr_to_planar420(mot.render_frame()), '420'))
            bare.append(mot.tracker.ctx.frame_read())
            stream.write(image)

    try:
        assert track_stream(Spy, mot, write_frames=True) == video.n_frames
    finally:
        stream.release()
        mot.tracker._clear_tracks()
    assert kinds[:video.n_frames] == [PlanarFrame] * video.n_frames
    back = VideoIO(SIZE, str(out))
    back.start_capture()
    try:
        for i in range(video.n_frames):
            assert np.array_equal(back.read(), want[i]), i
        assert back.read() is None
    finally:
        back.release()
    # the overlays are in the picture, and the tracker's frame is the clip's
    assert any((w != planar_to_bgr(*bgr_to_planar420(b), '420')).any() for w, b in zip(want, bare))
    assert np.array_equal(bare[0], planar_to_bgr(*bgr_to_planar420(video.frames[0]), '420'))
