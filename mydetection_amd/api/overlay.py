"""`Overlay`: the `overlay=` argument of Detector.annotate_frames and its YUV forms -- the zones and lines of the call's `Zones`,
their running counters and the trails of the tracks, painted into the frames on the device before the boxes (ops.draw_overlay;
include/mydet.h: mydet_draw_overlay_rgb_u8 has the raster rules, mydet_trails_frames those of the trails).  The reference prints
`Count: N` into its frame (utils/visualization.py: draw_bboxes_on_np); everything else here is this package's."""
from .. import _lib, ops
from .bound import Bound


class Overlay(Bound):
    """What the counting overlay paints.  zones: the polygons of the call's Zones, filled (zone_alpha while nobody is inside,
    occupied_alpha otherwise; 0..255) and outlined; lines: its directed lines, each with a tick on its positive side;
    counters: the parts of a zone's label, any of 'occupancy' (`N`), 'entries' (`+E`), 'visits' (`-V`, the finished visits) -- a
    line's label is `name +pos -neg`; empty: no labels.  trails: 0, or 2 .. 32 points kept per track, joined by segments in the
    track's id colour; the trail follows the anchor of the call's Zones ('center' without zones=) and, with classes, only tracks
    of those class indices.  thickness (outlines, lines, ticks), trail_thickness: 1..64 pixels, None = max(1, round(H / 360)) for
    frames of H rows, as Draw's; label_height: 8..64, None = as Draw's.
    Like Zones, the first call binds the object to the tracker's streams and max_tracks, the frame size and the device; it then
    holds the trail state (`state`, ops.trails_state_views names its fields; `last`: the output dict of the latest call,
    ops.trails_frames).  A later call with another shape is a ValueError.  reset() forgets the trails; the binding stays."""
    what = 'overlay'
    extra = ('_anchor', 'anchor')

    def __init__(self, zones=True, lines=True, counters=('occupancy', 'entries'), trails=0, zone_alpha=48, occupied_alpha=96,
                 thickness=None, trail_thickness=None, label_height=None, classes=None):
        super().__init__()
        self.zones, self.lines = bool(zones), bool(lines)
        self.counters = (counters,) if isinstance(counters, str) else tuple(counters or ())
        ops.overlay_counter_flags(self.counters)
        if isinstance(trails, bool) or not isinstance(trails, int) or not (trails == 0 or 2 <= trails <= _lib.TRAIL_MAX_POINTS):
            raise ValueError(f'Overlay: trails is 0 or 2 .. {_lib.TRAIL_MAX_POINTS} points per track, got {trails!r}')
        self.trails = trails
        if not (self.zones or self.lines or self.trails):
            raise ValueError('Overlay: nothing to paint: zones=False, lines=False and trails=0')
        for name, v in (('zone_alpha', zone_alpha), ('occupied_alpha', occupied_alpha)):
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 255:
                raise ValueError(f'Overlay: an integer {name} in 0..255 expected, got {v!r}')
        self.zone_alpha, self.occupied_alpha = zone_alpha, occupied_alpha
        # ops.draw_style has the rules of the sizes; None entries are checked with a stand-in and resolved per frame size
        ops.draw_style(2 if thickness is None else thickness, label_height=16 if label_height is None else label_height)
        ops.draw_style(2 if trail_thickness is None else trail_thickness)
        self.thickness, self.trail_thickness, self.label_height = thickness, trail_thickness, label_height
        self.classes = None if classes is None else tuple(int(c) for c in classes)
        ops.trail_set(2, 'center', self.classes)
        self._anchor = self._trail_set = self._track_out = None
        self._styles, self._geometry = {}, None

    def __repr__(self):
        return (f'Overlay(zones={self.zones}, lines={self.lines}, counters={self.counters}, trails={self.trails}, zone_alpha={self.zone_alpha}, '
                f'occupied_alpha={self.occupied_alpha}, thickness={self.thickness}, trail_thickness={self.trail_thickness}, '
                f'label_height={self.label_height}, classes={self.classes})')

    @property
    def zone_parts(self):
        """The call needs zones=: the geometry and the counters come from there."""
        return self.zones or self.lines

    def sizes(self, frame_hw):
        """(thickness, trail_thickness, label_height) for frames of size frame_hw: None entries resolved as Draw's."""
        from ..utils.visualization import default_label_height
        h = int(frame_hw[0])
        auto = min(max(1, round(h / 360)), _lib.DRAW_MAX_THICKNESS)
        return (auto if self.thickness is None else self.thickness, auto if self.trail_thickness is None else self.trail_thickness,
                default_label_height(h) if self.label_height is None else self.label_height)

    def style(self, frame_hw):
        """The ops.DrawStyle whose palette and glyph atlas the overlay uses for frames of size frame_hw (cached)."""
        height = self.sizes(frame_hw)[2]
        if height not in self._styles:
            self._styles[height] = ops.draw_style(label_height=height)
        return self._styles[height]

    def check_call(self, tracker, zones, img_hw):
        """The argument rules of a call that need no device."""
        if tracker is None:
            raise ValueError('overlay: overlay= paints what the tracker and the zones counted and needs tracker= in the same call')
        if self.zone_parts and zones is None:
            raise ValueError('overlay: zones=True or lines=True paint the polygons, lines and counters of a Zones and need zones= in the same call '
                             '(trails alone: Overlay(zones=False, lines=False, trails=N))')
        if not (self.trails or (self.zones and zones.polygons) or (self.lines and zones.lines)):
            raise ValueError(f'overlay: nothing to paint: {self!r} with {zones!r}')
        hw = self._call_key(tracker, zones, img_hw)[2]
        if max(hw) > _lib.ZONE_MAX_FRAME:
            raise ValueError(f'overlay: frames of at most {_lib.ZONE_MAX_FRAME} on a side, got {hw[0]}x{hw[1]}')

    def _call_key(self, tracker, zones, img_hw):
        return self._check_bound(tracker.streams, tracker.max_tracks, img_hw, 'center' if zones is None else zones.anchor)

    def _allocate(self, device):
        if self.trails:
            self._trail_set = ops.trail_set(self.trails, self._anchor, self.classes)
            self.state = ops.trails_state(self.streams, self.max_tracks, self.trails, device)

    def _reset_state(self):
        ops.trails_reset_(self.state, self.max_tracks, self.trails)

    def bind(self, tracker, zones, img_hw, device):
        """First call: take the tracker's shape, the frame size and the zones' anchor; allocate the trail state on the device."""
        self._bind_key(self._call_key(tracker, zones, img_hw), device)

    def run_trails(self, track_out, tracker, zones, img_hw):
        """The trails launch on a tracker launch's outputs (right behind it: no host synchronisation); keeps the result as `last`."""
        self.check_call(tracker, zones, img_hw)
        self.bind(tracker, zones, img_hw, track_out['box'].device)
        self.last = ops.trails_frames(track_out, self.state, self._trail_set) if self.trails else None
        self._track_out = track_out
        return self.last

    def geometry(self, zones, img_hw):
        """The ops.OverlayGeometry of the call's Zones (made once: the binding keeps frame size and Zones' shape)."""
        if self._geometry is None or self._geometry[0] is not zones:
            self._geometry = (zones, ops.overlay_geometry(zones.zone_set(img_hw), zones.names, self.sizes(img_hw)[0]))
        return self._geometry[1]

    def paint(self, image, yuv, zones, img_hw, coasting):
        """The overlay launch into the frames or planes of a call (ops.draw_overlay / ops.draw_overlay_yuv420)."""
        kwargs = dict(zones=self.zones, lines=self.lines, counters=self.counters, zone_alpha=self.zone_alpha, occupied_alpha=self.occupied_alpha,
                      trail_thickness=self.sizes(img_hw)[1], coasting=coasting)
        if self.zone_parts:
            kwargs.update(geometry=self.geometry(zones, img_hw), zones_out=zones.last)
        if self.trails:
            kwargs.update(trails_out=self.last, track_out=self._track_out)
        if yuv:
            ops.draw_overlay_yuv420(image, style=self.style(img_hw), **yuv, **kwargs)
        else:
            ops.draw_overlay(image, self.style(img_hw), **kwargs)
