"""`Tracker`: the `tracker=` argument of Detector.predict_frames and its YUV forms -- identities that persist from frame to
frame and Kalman-filtered boxes, computed on the device from the call's own detection records (ops.track_frames;
include/mydet.h: mydet_track_frames_f32 has the rules).  The state model is the reference's KFTracklet
(utils/structures.py:445-529); the reference has no loop around it, the association is this package's."""
from .. import ops
from .bound import Bound


class Tracker(Bound):
    """State and parameters of `streams` independent video streams, at most `max_tracks` (<= 512) live tracks each.

    match: the pair test of the association, 'iou' (axis-aligned, on cx, cy, w, h) or 'rotated' (the exact rotated IoU;
    'cxcywhd' models only); None = 'rotated' for a 'cxcywhd' model, 'iou' otherwise.  A detection continues a track of its
    class when their IoU is > match_thres; an unmatched detection with score >= new_thres (None: the call's conf_thres) starts
    one; a track is dropped after max_missed frames without a match, when its score (momentum) falls below min_score, or when
    its box leaves the frame.  p0, q, r: the filter's standard deviations (KFTracklet's constants by default).
    assign: 'greedy' (detections in score order, each takes the free track of largest IoU) or 'optimal' (the one-to-one
    assignment of largest total IoU).  low_thres: None, or the score from which a detection below the call's conf_thres may
    still CONTINUE a track that was matched or born in the previous frame (ByteTrack's second stage; it never starts one): the
    call's post-process then runs at min(conf_thres, low_thres).  high_thres: where the high band begins (None: the call's
    conf_thres); low_match_thres: the IoU threshold of the second stage (None: match_thres).  low_thres must be below
    high_thres: a call whose conf_thres is not above it is a ValueError.  include/mydet.h (mydet_track_assoc) has the rules.
    The first call binds the tracker to that call's frame size (H, W), box format and device; `state` is then the int32
    [streams, words] device buffer (ops.track_state_views names its fields) and reset() empties it (ids start at 1 again).
    A batch of B frames is `streams` runs of B / streams consecutive frames: frame f of stream s is frame s * (B / streams) + f."""
    what = 'tracker'
    extra = ('box_width', 'box width')
    hint = ' (one frame size per tracker)'

    def __init__(self, streams=1, max_tracks=256, match=None, match_thres=0.3, new_thres=None, max_missed=30, momentum=0.8,
                 min_score=0.1, p0=ops.TRACK_P0, q=ops.TRACK_Q, r=ops.TRACK_R, assign='greedy', low_thres=None, high_thres=None,
                 low_match_thres=None):
        super().__init__()
        self.streams, self.max_tracks = ops.check_streams('Tracker', streams), int(max_tracks)
        ops.track_state_words(self.max_tracks)
        if match is not None:
            ops.track_match_id(match)
        self.match = match
        self.match_thres, self.new_thres = float(match_thres), None if new_thres is None else float(new_thres)
        self.max_missed, self.momentum, self.min_score = int(max_missed), float(momentum), float(min_score)
        self.p0, self.q, self.r = tuple(p0), tuple(q), tuple(r)
        self.assign = assign
        self.low_thres, self.high_thres, self.low_match_thres = (None if v is None else float(v) for v in (low_thres, high_thres, low_match_thres))
        self.params((1, 1), 'iou', 0.0)                              # the range checks, before any device is touched
        self.assoc(float('nan') if self.low_thres is None else self.low_thres + 1.0)       # a conf_thres above low_thres
        self.box_width = None

    def __repr__(self):
        return (f'Tracker(streams={self.streams}, max_tracks={self.max_tracks}, match={self.match!r}, match_thres={self.match_thres}, '
                f'new_thres={self.new_thres}, max_missed={self.max_missed}, momentum={self.momentum}, min_score={self.min_score}, '
                f'assign={self.assign!r}, low_thres={self.low_thres}, high_thres={self.high_thres}, low_match_thres={self.low_match_thres})')

    def params(self, img_hw, match, conf_thres):
        """The kernel's parameter struct for a frame size, a resolved pair test and the call's conf_thres."""
        return ops.track_params(img_hw, match, self.match_thres, conf_thres if self.new_thres is None else self.new_thres,
                                self.max_missed, self.momentum, self.min_score, self.p0, self.q, self.r)

    def assoc(self, conf_thres):
        """The association mode for a call's conf_thres: None for the default (greedy, one band: the entry point of old), else
        the struct of ops.track_assoc.  A ValueError when the call's conf_thres is not above low_thres."""
        if self.low_thres is None:
            if self.assign == 'greedy' and self.high_thres is None and self.low_match_thres is None:
                return None
            return ops.track_assoc(self.assign, None, self.high_thres, self.low_match_thres)
        return ops.track_assoc(self.assign, self.low_thres, conf_thres if self.high_thres is None else self.high_thres,
                               self.match_thres if self.low_match_thres is None else self.low_match_thres)

    def resolve_match(self, bb_format):
        """The pair test for a model's box format; a ValueError for 'rotated' on a model without angles."""
        if self.match is None:
            return 'rotated' if bb_format == 'cxcywhd' else 'iou'
        if self.match == 'rotated' and bb_format != 'cxcywhd':
            raise ValueError(f"tracker: match 'rotated' needs a 'cxcywhd' model; this one predicts {bb_format!r}")
        return self.match

    def check_call(self, n_frames, img_hw, bb_format):
        """The argument rules of a tracked call that need no device: the batch is whole runs of every stream, and the frame
        size and box format are those of the first call."""
        self.resolve_match(bb_format)
        if n_frames < 1 or n_frames % self.streams:
            raise ValueError(f'tracker: a batch of {n_frames} frames is not a multiple of streams = {self.streams}')
        self._check_bound(self.streams, self.max_tracks, img_hw, 5 if bb_format == 'cxcywhd' else 4)

    def _allocate(self, device):
        self.state = ops.track_state(self.streams, self.max_tracks, device)

    def _reset_state(self):
        """reset(): forget every track; the next id of every stream is 1 again.  The frame size stays bound.  A CameraMotion used
        with this tracker is not touched: it has its own reset().  Neither is an Appearance: a slot's template is read only while
        its `has` flag is set, a reset tracker matches nothing (so no template moves), and a birth into a slot overwrites both;
        call Appearance.reset() as well to clear them at once."""
        ops.track_reset_(self.state, self.max_tracks)

    def bind(self, img_hw, box_width, device):
        """First call: take the frame size and allocate the state on the records' device."""
        return self._bind_key(self._check_bound(self.streams, self.max_tracks, img_hw, int(box_width)), device)
