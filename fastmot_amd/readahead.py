"""The frame loop of the reference application (app.py:85-98) with ONE frame of read-ahead.

The reference's `app.py` is the command line -- it runs unmodified against this tree (`import fastmot`,
tests/test_dropin_app.py) and its loop calls `mot.step(frame)`.  A caller that already holds the following frame (a
file source, the capture queue of VideoIO) can hand it over as `next_frame`: the detector pass of frame t+1 then
overlaps the ReID / association stages of frame t, with identical results.  This function is
that loop; everything around it (arguments, configuration file, logging) is the reference's."""
from collections import deque

from .utils.motchallenge import write_rows


def track_stream(stream, mot=None, txt=None, resize_to=None, write_frames=False, lookahead=1, snapshots=None):
    """stream: a started VideoIO; mot: a reset MOT (None: frames are only passed through); txt: an open text file for
    MOT Challenge result rows (app.py:91-97), needs `resize_to`; write_frames: stream.write(frame) after each step
    (the frame carries the overlays when the MOT draws; a frame that lives on the GPU only -- VideoIO(gpu_encode=True) with
    gpu_decode / gpu_resize -- is written as mot.encode_frame(), or as mot.export_frame_i420() to a '.y4m' output; with
    MOT(redact=...) a host frame that the MOT did not draw on is redacted in place, mot.redact_frame, before it is written); lookahead: upcoming frames read ahead and handed to each step
    as `next_frames` (a MOT with detector_lookahead = k batches up to k of them); snapshots: a utils.snapshots.SnapshotWriter
    (or anything with update(mot) / close()), updated after each step and closed at the end -- one JPEG crop per tracked
    object, by its policy.  Returns the number of frames."""
    n = 0
    frame = stream.read()
    upcoming = deque()
    try:
        n = _track_loop(stream, mot, txt, resize_to, write_frames, lookahead, snapshots, frame, upcoming)
    finally:
        if snapshots is not None:
            snapshots.close()
    return n


def _track_loop(stream, mot, txt, resize_to, write_frames, lookahead, snapshots, frame, upcoming):
    n = 0
    while frame is not None:
        while len(upcoming) < max(lookahead, 1) and (not upcoming or upcoming[-1] is not None):
            upcoming.append(stream.read())
        ahead = [f for f in upcoming if f is not None]
        if mot is not None:
            if lookahead > 1:
                mot.step(frame, next_frames=ahead)
            else:
                mot.step(frame, next_frame=upcoming[0])
            if txt is not None:
                write_rows(txt, mot.frame_count, mot.visible_tracks(), resize_to, stream.resolution)
            if snapshots is not None:
                snapshots.update(mot)
        if write_frames:
            if mot is not None and getattr(stream, 'gpu_encode', False) and not hasattr(frame, '__array_interface__'):
                i420 = getattr(stream, 'i420_output', False)
                stream.write(mot.export_frame_i420() if i420 else mot.encode_frame(stream.jpeg_quality))
            else:
                if mot is not None and getattr(mot, 'redact', None) is not None and not mot.draw and hasattr(frame, '__array_interface__'):
                    mot.redact_frame(frame)          # (draw=True has redacted it in the step; this loop owns the array)
                stream.write(frame)
        frame = upcoming.popleft()
        n += 1
    return n
