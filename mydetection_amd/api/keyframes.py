"""`KeyFrames`: the `keyframes=` argument of Detector's tracked frame methods -- the network runs on every n-th frame only, and
one launch pair on the device carries the boxes of a key frame through the frames that follow by matching their pixels
(ops.carry_records; include/mydet.h: mydet_carry_records_rgb_u8 has the rules), so that the tracker, the zones and everything
that paints still get one record per frame.  The reference project has nothing like it; deployed pipelines do it with a
detector interval and a visual tracker behind it."""
from .. import ops
from .bound import Bound


class KeyFrames(Bound):
    """The settings of the carry, the frame counter of the streams and their state.

    every: frame c of a stream is a key frame when c % every == 0, 1 .. 16; the first frame after construction or reset() is
    one.  search: the coarse search range, 4 .. 16 cells of s pixels, s by the box size (a box whose smaller side is up to 21
    pixels has s = 1), so a step of up to search * s pixels per frame is followed; min_texture: the SAD range over the
    candidates below which a box sits on a flat region and is dropped; max_diff: the mean absolute difference per cell above
    which the best match is no match and the box is dropped as lost.  A dropped box stays dropped until the next key frame:
    its track coasts on the Kalman prediction, as on any miss.  Boxes keep their key-frame size and angle.
    All streams of a call have the same number of frames, so one counter serves them: `frames` is the number of frames every
    stream has seen.  Calls of any length continue each other: two calls of F1 and F2 frames leave what one call of F1 + F2
    leaves.  The first call binds the object to the tracker's streams, the frame size and the device; a later call with
    another is a ValueError.  `state` is then the int32 [streams, words] device buffer (ops.carry_state_views names its
    fields) and `last` the dict of the latest call on the device: 'how' int32 [streams, F, 512] (0 no box, 1 key, 2 carried,
    3 flat, 4 lost, 5 left the frame, 6 not carriable), 'offset' int32 [streams, F, 512, 2], 'sad' int32 [streams, F, 512, 2]
    (coarse smin, smax).  reset() forgets the counter and every carried box; Tracker.reset() does NOT touch this object, and
    reset() does not touch the tracker."""
    what = 'keyframes'

    def __init__(self, every=4, search=8, min_texture=1024, max_diff=24):
        super().__init__()
        self.set = ops.carry_set(every, search, min_texture, max_diff)           # the range checks, before any device is touched
        self.every, self.search, self.min_texture, self.max_diff = int(every), int(search), int(min_texture), int(max_diff)
        self.frames = 0

    def __repr__(self):
        return f'KeyFrames(every={self.every}, search={self.search}, min_texture={self.min_texture}, max_diff={self.max_diff})'

    def check_call(self, tracker, img_hw):
        """The argument rules of a call that need no device: the tracker's streams and the frame size are those of the first call."""
        self._key(tracker, img_hw)

    def _key(self, tracker, img_hw):
        return self._check_bound(tracker.streams, None, img_hw)      # no track slots in this state: max_tracks is not bound

    def _allocate(self, device):
        self.state = ops.carry_state(self.streams, device)

    def _reset_state(self):
        ops.carry_reset_(self.state)

    def reset(self):
        self.frames = 0
        super().reset()

    def key_mask(self, F):
        """Which of the next F frames of every stream are key frames: host arithmetic on the counter."""
        return [(self.frames + f) % self.every == 0 for f in range(F)]

    def run(self, image, yuv, key_records, tracker, img_hw, F, width, shift=None):
        """The carry launches on the frames of a call (image, yuv: what a frame source's image() returns) and the records of
        its key frames (None when key_mask(F) has none); width: 4, or 5 for rotated records.  No host synchronisation.  Returns
        the record dict of all frames, keeps how, offset and sad in `last` and moves the counter on by F."""
        self.check_call(tracker, img_hw)
        dev = self._image_device(image)
        state = self.bind(tracker, img_hw, dev)
        records = None
        if key_records is None:
            import torch
            records = torch.empty((self.streams * F, ops.record_words(width)), dtype=torch.int32, device=dev)
        rec = ops.carry_records(image, key_records, self.key_mask(F), state, self.set, frames_per_stream=F,
                                layout=yuv.get('layout') if yuv else None, shift=shift, records=records)
        self.last = {k: rec.pop(k) for k in ('how', 'offset', 'sad')}
        self.frames += F
        return rec
