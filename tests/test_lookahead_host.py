"""CPU: the detector look-ahead schedule of MOT.step (mot.DetectorLookahead), the option's checks, and the read-ahead
deque of readahead.track_stream."""
import pytest

from fastmot_amd.mot import MOT, DetectorLookahead
from fastmot_amd.readahead import track_stream


def schedule(k, n, upcoming_of=None):
    """Frames (indices) each step of an n-frame sequence enqueues, the step handing over up to k upcoming frames."""
    frames = [object() for _ in range(n)]
    la = DetectorLookahead(k)
    out = []
    for t in range(n):
        la.consume(frames[t])
        upcoming = frames[t + 1:t + 1 + k] if upcoming_of is None else [frames[i] for i in upcoming_of(t)]
        out.append([frames.index(f) for f in la.to_enqueue(upcoming)])
    return out


def test_one_pass_whenever_nothing_is_in_flight():
    assert schedule(2, 7) == [[1, 2], [], [3, 4], [], [5, 6], [], []]
    assert schedule(3, 7) == [[1, 2, 3], [], [], [4, 5, 6], [], [], []]


def test_sequence_end_gets_a_smaller_batch_or_a_single_prefetch():
    assert schedule(3, 6) == [[1, 2, 3], [], [], [4, 5], [], []]
    assert schedule(2, 4) == [[1, 2], [], [3], []]
    assert schedule(4, 2) == [[1], []]
    assert schedule(2, 1) == [[]]


def test_a_frame_that_was_not_announced_makes_the_announced_ones_stale():
    frames = [object() for _ in range(6)]
    la = DetectorLookahead(2)
    assert la.consume(frames[0]) is False
    assert la.to_enqueue(frames[1:3]) == frames[1:3]
    assert la.consume(frames[1]) is True
    assert la.to_enqueue(frames[2:4]) == []            # frames[2] is still to come
    other = object()
    assert la.consume(other) is False                  # not frames[2]: the pass on it is stale
    assert la.announced == []
    assert la.to_enqueue(frames[4:6]) == frames[4:6]
    assert la.consume(frames[4]) is True and la.consume(frames[5]) is True
    assert la.to_enqueue([]) == []


def test_no_upcoming_frames_no_pass():
    la = DetectorLookahead(3)
    la.consume(object())
    assert la.to_enqueue([]) == [] and la.announced == []


@pytest.mark.parametrize('kw', [dict(detector_type='YOLO', detector_frame_skip=2, detector_lookahead=2),
                                dict(detector_type='SSD', detector_frame_skip=1, detector_lookahead=2),
                                dict(detector_type='public', detector_frame_skip=1, detector_lookahead=3),
                                dict(detector_type='YOLO', detector_frame_skip=1, detector_lookahead=5),
                                dict(detector_type='YOLO', detector_frame_skip=1, detector_lookahead=0)])
def test_lookahead_option_is_checked_before_anything_is_built(kw):
    with pytest.raises(ValueError):
        MOT((640, 480), **kw)


class _Stream:
    resolution = (64, 48)

    def __init__(self, n):
        self.frames = [object() for _ in range(n)]
        self.reads = 0

    def read(self):
        self.reads += 1
        return self.frames[self.reads - 1] if self.reads <= len(self.frames) else None


class _Mot:
    def __init__(self):
        self.calls = []

    def step(self, frame, next_frame=None, next_frames=None):
        self.calls.append((frame, next_frame, next_frames))


@pytest.mark.parametrize('n', [0, 1, 2, 5, 6])
@pytest.mark.parametrize('lookahead', [1, 2, 3])
def test_track_stream_hands_over_the_upcoming_frames(n, lookahead):
    stream, mot = _Stream(n), _Mot()
    assert track_stream(stream, mot, lookahead=lookahead) == n
    fr = stream.frames
    assert [c[0] for c in mot.calls] == fr
    for t, (_, nxt, nxts) in enumerate(mot.calls):
        if lookahead == 1:
            assert nxts is None and nxt is (fr[t + 1] if t + 1 < n else None)
        else:
            assert nxt is None and nxts == fr[t + 1:t + 1 + lookahead]
    assert stream.reads == n + 1                       # every frame read once, then the end of the stream
