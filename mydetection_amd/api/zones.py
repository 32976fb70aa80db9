"""`Zones`: the `zones=` argument of Detector's tracked frame methods -- how many tracks are inside each polygon, how many went
through each directed line, and for how long they stayed, counted on the device by one launch behind the tracker launch
(ops.zones_frames; include/mydet.h: mydet_zones_frames has the rules).  The reference project counts the people of one frame
(utils/visualization.py: draw_bboxes_on_np prints `Count: N`); the bookkeeping across frames is this package's."""
from .. import _lib, ops
from .bound import Bound


class Zones(Bound):
    """Polygons and directed lines in frame pixels, and the counters of every stream of the tracker they are used with.

    polygons: at most 16 sequences of 3 .. 16 points (x, y); lines: at most 16 pairs ((ax, ay), (bx, by)), A -> B: a crossing
    is counted as `pos` when the track arrives on the side where (B - A) x (p - A) > 0, as `neg` on the other side.
    Coordinates are quantised to 1/16 pixel and every decision is an integer comparison, so a point on a shared edge of
    two polygons is inside exactly one of them.  anchor: the point of a track's box
    that is tested, 'center' or 'bottom' (cx, cy + h/2; 'cxcywh' models only).  classes: None, or up to 16 class indices to
    count.  coasting: also follow live tracks through frames without a detection, at their predicted boxes (a crossing is then
    counted where the prediction crosses, not at the re-match).  heat: None, or (gh, gw) <= 1024 each: an int32 [streams,gh,gw]
    map that counts the anchors of matched tracks per cell across calls.  names: None, or one name per polygon followed by
    one per line, used by counts().
    The first call binds the object to the tracker's streams and max_tracks, the frame size and the device; a later call with
    another is a ValueError.  `state` is then the int32 [streams, words] device buffer (ops.zones_state_views names its fields),
    `last` the output dict of the latest call on the device (ops.zones_frames), `heat` the heat map (None without heat=).
    reset() zeroes the counters, the frame counter, the heat map and forgets who is inside; the binding stays."""
    what = 'zones'

    def __init__(self, polygons=(), lines=(), anchor='center', classes=None, coasting=False, heat=None, names=None):
        super().__init__()
        self.polygons = [[(float(x), float(y)) for x, y in poly] for poly in self._rows(polygons, 'polygons')]
        self.lines = [[(float(x), float(y)) for x, y in line] for line in self._rows(lines, 'lines')]
        self.anchor, self.coasting = anchor, bool(coasting)
        self.classes = None if classes is None else tuple(int(c) for c in classes)
        self.heat_hw = None if heat is None else tuple(heat)
        self.zone_set((_lib.ZONE_MAX_FRAME, _lib.ZONE_MAX_FRAME))    # the range checks, before any device is touched
        n = len(self.polygons) + len(self.lines)
        if names is None:
            names = [f'zone{z}' for z in range(len(self.polygons))] + [f'line{l}' for l in range(len(self.lines))]
        names = [str(v) for v in names]
        if len(names) != n:
            raise ValueError(f'Zones: names is one name per polygon followed by one per line ({n}), got {len(names)}')
        self.names = names
        self.heat = self._set = None

    @staticmethod
    def _rows(rows, what):
        try:
            return [[tuple(pt) for pt in row] for row in rows]
        except TypeError:
            raise ValueError(f'Zones: {what} is a sequence of sequences of points (x, y), got {rows!r}') from None

    def __repr__(self):
        return (f'Zones({len(self.polygons)} polygons, {len(self.lines)} lines, anchor={self.anchor!r}, classes={self.classes}, '
                f'coasting={self.coasting}, heat={self.heat_hw})')

    def zone_set(self, img_hw):
        """The kernel's parameter struct for a frame size (ops.zone_set)."""
        return ops.zone_set(img_hw, self.polygons, self.lines, self.anchor, self.classes, self.coasting, self.heat_hw)

    def check_call(self, tracker, img_hw, bb_format):
        """The argument rules of a call that need no device: the box format suits the anchor, and the tracker's shape and the
        frame size are those of the first call."""
        if self.anchor == 'bottom' and bb_format != 'cxcywh':
            raise ValueError(f"zones: anchor 'bottom' is for 'cxcywh' models; this one predicts {bb_format!r}")
        if self.img_hw is None:
            self.zone_set(img_hw)                                    # the frame-size rule
        self._key(tracker, img_hw)

    def _allocate(self, device):
        self._set = self.zone_set(self.img_hw)
        self.state = ops.zones_state(self.streams, self.max_tracks, device)
        if self.heat_hw is not None:
            self.heat = ops.zones_heat(self.streams, self._set, device)

    def _reset_state(self):
        ops.zones_reset_(self.state, self.max_tracks)
        if self.heat is not None:
            self.heat.zero_()

    def run(self, track_out, tracker, img_hw):
        """The zone launch on a tracker launch's outputs; no host synchronisation.  Returns (and keeps as `last`) the dict of
        ops.zones_frames.  The caller has checked the model's box format (check_call)."""
        self.check_call(tracker, img_hw, 'cxcywh')
        state = self.bind(tracker, img_hw, track_out['box'].device)
        self.last = ops.zones_frames(track_out, state, self._set, heat=self.heat)
        return self.last

    def counts(self):
        """The cumulative numbers, one host synchronisation (the state crosses once): a list with one dict per stream --
        'frames' (frames seen), 'zones': name -> {'occupancy', 'entries', 'exits', 'lost', 'visits', 'mean_dwell' (frames per
        finished visit, None without one), 'max_dwell'}, 'lines': name -> {'pos', 'neg'}.  A visit ends by an exit or by the
        track's end inside ('lost').  Before the first call: an empty list."""
        if self.state is None:
            return []
        v = ops.zones_state_views(self.state.cpu(), self.max_tracks)
        nz, out = len(self.polygons), []
        for s in range(self.streams):
            inside = v['inside'][s]
            zones, lines = {}, {}
            for z in range(nz):
                entries, exits, lost, visits = v['zone_counts'][s, z].tolist()
                zones[self.names[z]] = {'occupancy': int(((inside >> z) & 1).sum()), 'entries': entries, 'exits': exits, 'lost': lost,
                                        'visits': visits, 'mean_dwell': int(v['dwell_sum'][s, z]) / visits if visits else None,
                                        'max_dwell': int(v['dwell_max'][s, z])}
            for l in range(len(self.lines)):
                pos, neg = v['line_counts'][s, l].tolist()
                lines[self.names[nz + l]] = {'pos': pos, 'neg': neg}
            out.append({'frames': int(v['now'][s]), 'zones': zones, 'lines': lines})
        return out
