"""`Appearance`: the `appearance=` argument of Detector's tracked frame methods -- the tracker matches by what an object looks
like as well as by where it is.  One launch on the call's frames gives every detection a 128-bin colour descriptor
(ops.appear_records; include/mydet.h: mydet_appear_boxes_rgb_u8 has the rule), and the tracker launch keeps a template per
track, gates its IoU matches by it and re-identifies lost tracks (mydet_track_frames_appear_f32).  With `weight` the optimal
assignment solves one fused IoU-and-appearance cost instead (mydet_track_frames_appear_optimal_f32).  The reference project has
no tracker loop and nothing like it; the step is the appearance branch of DeepSORT / BoT-SORT with a colour histogram in place
of a ReID network: the package ships no weights."""
import math

from .. import ops
from .bound import Bound


class Appearance(Bound):
    """The appearance settings and the templates of every track slot of the tracker it is used with.

    gate: None (off) or a fraction in (0, 1] of the largest similarity -- an IoU match of a track that has a template is
    offered only when the histogram intersection of template and detection reaches it; reid: None (off) or such a fraction --
    a detection that would start a track is instead given to the most similar lost track (not matched in the previous frame)
    of its class within `reach` times the larger box side of its predicted centre, when the similarity reaches it; momentum:
    the share of its old template a matched track keeps; update_thres: the detection score from which a match moves the
    template (None: the tracker's birth threshold, so a low-band match never does).  The defaults are starting points, not
    tuned values: there is no dataset behind them.  weight: None -- the greedy walk with the gate, and a Tracker with
    assign='optimal' is a ValueError; or a fraction in [0, 1] -- the share of the appearance in the cost of the optimal
    assignment, floor(weight * 256 + 0.5) of 256: each stage is then ONE minimum-cost assignment on
    m = ((256 - w) * IoU + w * similarity) >> 8 (both on a scale of 65536; a track without a template keeps its IoU; the gate
    still removes pairs), which a Tracker with assign='optimal' runs and a greedy one refuses with a ValueError.  `workspace`
    is then the int32 [streams, 512 * max_tracks] device buffer the similarities of a frame are computed into, allocated
    beside the state.
    The first call binds the object to the tracker's streams and max_tracks, the frame size and the device; a later call with
    another is a ValueError.  `state` is then the int32 [streams, words] device buffer (ops.appear_state_views names its
    fields) and `last` the latest call's outputs on the device: 'desc' uint16 [B,512,128] (row = record slot of the call's
    final records), 'sim' and 'how' int32 [streams, F, max_tracks].
    reset() clears every template; Tracker.reset() does NOT touch this object, and need not: a slot's template is read only
    while its `has` flag is set, and a birth into a slot overwrites both."""
    what = 'appearance'

    def __init__(self, gate=0.3, reid=0.6, momentum=0.9, reach=2.0, update_thres=None, weight=None):
        super().__init__()
        self.weight, self.weight256, self.workspace = None, None, None
        if weight is not None:
            w = float(weight)
            if not 0 <= w <= 1:                                            # false for a NaN
                raise ValueError(f'appearance: weight is None (the greedy walk) or a fraction in [0, 1], got {weight!r}')
            self.weight, self.weight256 = w, int(math.floor(w * 256 + 0.5))
        ops.appear_set(gate, reid, momentum, reach, 0.0 if update_thres is None else update_thres)     # the range checks, before any device
        self.gate, self.reid, self.momentum, self.reach = gate, reid, float(momentum), float(reach)
        self.update_thres = None if update_thres is None else float(update_thres)

    def __repr__(self):
        return (f'Appearance(gate={self.gate}, reid={self.reid}, momentum={self.momentum}, reach={self.reach}, '
                f'update_thres={self.update_thres}' + ('' if self.weight is None else f', weight={self.weight}') + ')')

    def set(self, birth_thres):
        """The kernel's settings struct for a call whose tracker starts tracks at `birth_thres`."""
        return ops.appear_set(self.gate, self.reid, self.momentum, self.reach, birth_thres if self.update_thres is None else self.update_thres)

    def check_tracker(self, tracker):
        """Without a weight the greedy rule: the optimal assignment forms its costs on the fly and has no place for the gate.
        With one the reverse: the fused cost is the optimal assignment's, the walk keeps its IoU-major key."""
        if self.weight is None:
            if tracker.assign != 'greedy':
                raise ValueError(f"appearance: runs with a Tracker of assign='greedy' only, got assign={tracker.assign!r}")
        elif tracker.assign != 'optimal':
            raise ValueError(f"appearance: weight= is the fused cost of a Tracker of assign='optimal', got assign={tracker.assign!r}")

    def check_call(self, tracker, img_hw):
        """The argument rules of a call that need no device: a tracker of the assignment this object runs with, and the
        tracker's streams and max_tracks and the frame size are those of the first call."""
        self.check_tracker(tracker)
        self._key(tracker, img_hw)

    def _allocate(self, device):
        self.state = ops.appear_state(self.streams, self.max_tracks, device)
        if self.weight is not None:
            self.workspace = ops.appear_workspace(self.streams, self.max_tracks, device)

    def _reset_state(self):
        ops.appear_reset_(self.state, self.max_tracks)

    def run(self, image, yuv, rec, tracker, img_hw, birth_thres):
        """The descriptor launch on the frames of a call (image, yuv: what a frame source's image() returns) and its final
        records; no host synchronisation.  Returns what ops.track_frames takes as appear= and keeps the descriptors in `last`;
        launch_args() has the rest of a call with a weight."""
        self.check_call(tracker, img_hw)
        state = self.bind(tracker, img_hw, self._image_device(image))
        desc = ops.appear_records(image, rec, **yuv)
        self.last = {'desc': desc}
        return self.set(birth_thres), desc, state

    def launch_args(self):
        """The keyword arguments of ops.track_frames beside appear=: the weight and the workspace of the fused cost, or none."""
        return {} if self.weight is None else {'appear_weight': self.weight256, 'appear_ws': self.workspace}

    def took(self, track_out):
        """Keep the tracker launch's sim and how beside the descriptors."""
        self.last.update(sim=track_out['sim'], how=track_out['how'])
