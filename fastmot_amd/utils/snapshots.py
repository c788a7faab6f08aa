"""One JPEG crop per tracked object, written to a directory while a stream is tracked: the "object encoder" next to the
tracker.  A SnapshotWriter asks MOT.encode_objects() after each step -- every crop of a frame encoded in one pass on the
GPU, only compressed bytes on the host -- and decides by its policy which files reach the disk:

    'all'      <dir>/<trk_id:06d>/<frame:06d>.jpg for every visible track on every `every`-th frame
    'first'    <dir>/<trk_id:06d>.jpg the first time a track is visible (an alarm thumbnail)
    'largest'  <dir>/<trk_id:06d>.jpg, written at close(): of every track the crop with the largest clipped area so far
               (a "best shot"; kept in memory until then, the first of equally large ones)

`frame` is mot.frame_count after the step, as in the MOT Challenge rows of readahead.track_stream, which takes a writer as
`snapshots=`.  With MOT(redact=...) the crops are cut from the redacted picture (MOT.encode_objects)."""
from pathlib import Path

POLICIES = ('largest', 'first', 'all')


class SnapshotWriter:
    def __init__(self, directory, policy='largest', every=1, **encode_options):
        """directory: created if missing.  every: look at every `every`-th step only (default 1: each).  encode_options:
        keywords of MOT.encode_objects (quality, part, margin, shrink, confirmed, classes, overlays)."""
        if policy not in POLICIES:
            raise ValueError(f'snapshot policy {policy!r}: one of {POLICIES}')
        if int(every) < 1:
            raise ValueError('every must be at least 1')
        self.directory = Path(directory)
        self.policy, self.every, self.encode_options = policy, int(every), dict(encode_options)
        self.directory.mkdir(parents=True, exist_ok=True)
        self.written = []           # paths in the order they were written
        self._seen = set()          # 'first': tracks that have their file
        self._best = {}             # 'largest': trk_id -> (area, data)
        self._steps = 0
        self._closed = False

    def update(self, mot):
        """Call after a step of `mot`."""
        if self._closed:
            raise RuntimeError('SnapshotWriter is closed')
        self._steps += 1
        if (self._steps - 1) % self.every:
            return
        for obj in mot.encode_objects(**self.encode_options):
            if self.policy == 'all':
                sub = self.directory / f'{obj.trk_id:06d}'
                sub.mkdir(exist_ok=True)
                self._write(sub / f'{mot.frame_count:06d}.jpg', obj.data)
            elif self.policy == 'first':
                if obj.trk_id not in self._seen:
                    self._seen.add(obj.trk_id)
                    self._write(self.directory / f'{obj.trk_id:06d}.jpg', obj.data)
            else:
                area = (obj.rect[2] - obj.rect[0] + 1) * (obj.rect[3] - obj.rect[1] + 1)
                if obj.trk_id not in self._best or area > self._best[obj.trk_id][0]:
                    self._best[obj.trk_id] = (area, obj.data)

    def close(self):
        """Writes what the policy kept in memory; further calls do nothing."""
        if self._closed:
            return
        self._closed = True
        for trk_id in sorted(self._best):
            self._write(self.directory / f'{trk_id:06d}.jpg', self._best[trk_id][1])
        self._best = {}

    def _write(self, path, data):
        path.write_bytes(data)
        self.written.append(path)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
