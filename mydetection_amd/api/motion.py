"""`CameraMotion`: the `motion=` argument of Detector's tracked frame methods -- one global image shift per frame, estimated
on the device from the frames themselves (ops.motion_frames; include/mydet.h: mydet_motion_frames_rgb_u8 has the rules) and
handed to the tracker, whose predictions move with the camera before they are associated (mydet_track_frames_motion_f32).
The reference project has no tracker loop and nothing like it; the step is BoT-SORT's camera-motion compensation with a pure
translation (model='shift') or with a four-parameter similarity -- shift, rotation, isotropic zoom -- fitted to the same block
vectors (model='similarity'; mydet_motion_warp_frames_rgb_u8, mydet_track_frames_warp_f32)."""
from .. import ops
from .bound import Bound


class CameraMotion(Bound):
    """The estimator's settings and its state for every stream of the tracker it is used with.

    reduce: None (by frame size) or 2, 4, 8 -- the luma is reduced by k x k box means before the coarse search; search: the
    coarse search range, 4 .. 16 reduced pixels, so motion up to search * reduce pixels per frame is found; min_texture: the
    SAD range below which a 16 x 16 block is flat and does not vote; min_blocks: None (an eighth of the blocks, at least 2) or
    the number of voting blocks below which a frame reports no motion (valid = 0: a scene cut, a flat frame).  Both stages
    take the median over the blocks, so moving objects that cover less than half of the voting blocks do not disturb it.
    The first call binds the object to the tracker's streams, the frame size and the device; a later call with another is a
    ValueError.  `state` is then the int32 [streams, words] device buffer (ops.motion_state_views names its fields) and `last`
    the output dict of the latest call on the device: 'shift' int32 [streams, F, 4] = (dx, dy, valid, n_valid), 'blocks'.
    model: 'shift', or 'similarity' for a camera that also yaws, rolls, zooms, climbs or descends: every block is refined around
    its own vector and a similarity about the frame centre is fitted to the block vectors (medians over block pairs, then two
    rounds of least squares over the blocks within `tolerance` pixels of the model).  `last` then also holds 'warp' int32
    [streams, F, 8] = (a, b, tx, ty, s_q, deg_q, valid, n_inliers) in Q16, which the tracker's launch takes in the place of the
    shift: predictions are moved, turned and scaled; 'shift' stays the motion of the frame centre in whole pixels, which is what
    the key-frame carry reads.  max_zoom (None: 1/8) and max_rotation (None: 7 degrees) are the largest |zoom - 1| and rotation of
    a valid frame: a fit beyond them reports no motion.  Foreign motion on up to a quarter of the voting blocks does not disturb
    the fit (its start pairs the blocks, and a pair is lost with either of its blocks).
    reset() forgets the last frame of every stream, so that the next frame reports (0, 0, 0, 0); Tracker.reset() does NOT
    touch this object, and reset() does not touch the tracker.
    Zones, trails and the heat map stay in frame pixels: they assume a fixed camera."""
    what = 'motion'

    def __init__(self, reduce=None, search=8, min_texture=1024, min_blocks=None, model='shift', max_zoom=None, max_rotation=None,
                 tolerance=2.0):
        super().__init__()
        # the range checks, before any device is touched
        self.set = ops.motion_set(reduce, search, min_texture, min_blocks, model, max_zoom, max_rotation, tolerance)
        self.reduce, self.search, self.min_texture, self.min_blocks = reduce, int(search), int(min_texture), min_blocks
        self.model, self.max_zoom, self.max_rotation, self.tolerance = model, max_zoom, max_rotation, float(tolerance)

    def __repr__(self):
        base = f'CameraMotion(reduce={self.reduce}, search={self.search}, min_texture={self.min_texture}, min_blocks={self.min_blocks}'
        if self.model == 'shift':                                    # the text it always had
            return base + ')'
        return base + f', model={self.model!r}, max_zoom={self.max_zoom}, max_rotation={self.max_rotation}, tolerance={self.tolerance})'

    def track_args(self):
        """The camera-motion keywords of ops.track_frames for the latest call: warp= under the similarity model, else shift=."""
        return {'warp': self.last['warp']} if self.model == 'similarity' else {'shift': self.last['shift']}

    def check_call(self, tracker, img_hw):
        """The argument rules of a call that need no device: the frame is large enough for a block and its search window, and
        the tracker's streams and the frame size are those of the first call."""
        if self.img_hw is None:
            ops.motion_geometry((int(img_hw[0]), int(img_hw[1])), self.set)      # the frame-size rule
        self._key(tracker, img_hw)

    def _key(self, tracker, img_hw):
        return self._check_bound(tracker.streams, None, img_hw)      # no track slots in this state: max_tracks is not bound

    def _allocate(self, device):
        self.state = ops.motion_state(self.streams, self.img_hw, self.set, device)

    def _reset_state(self):
        ops.motion_reset_(self.state, self.img_hw, self.set)

    def run(self, image, yuv, tracker, img_hw):
        """The estimator's launches on the frames of a call (image, yuv: what a frame source's image() returns); no host
        synchronisation.  Returns (and keeps in `last`) the dict of ops.motion_frames."""
        self.check_call(tracker, img_hw)
        state = self.bind(tracker, img_hw, self._image_device(image))
        self.last = ops.motion_frames(image, state, self.set, layout=yuv.get('layout') if yuv else None)
        return self.last
