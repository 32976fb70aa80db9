"""Plain-Python restatement of the zone and line counting rules of include/mydet.h (mydet_zones_frames), written from the rule
text: Python integers everywhere (no overflow to think about), float32 only where the rules say float32 (the anchor and its
quantisation).  tests/test_zones_host.py holds its geometry to exact fractions; tests/test_gpu_zones.py holds the kernel to it
with ==."""
import numpy as np

ZMAX = 16
COORD_MAX = 1 << 20
BAD_CLASS = -1                      # MYDET_COUNT_BAD_CLASS


def q(v):
    """q(v) = (int32) floorf(min(max(v * 16.0f, -1048576.0f), 1048576.0f)) on a float32."""
    with np.errstate(over='ignore'):
        v = np.float32(v) * np.float32(16.0)
    v = min(max(v, np.float32(-COORD_MAX)), np.float32(COORD_MAX))
    return int(np.floor(v))


def quantise(points):
    return [(q(x), q(y)) for x, y in points]


def sign(v):
    return (v > 0) - (v < 0)


def cross(u, v):
    return u[0] * v[1] - u[1] * v[0]


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1])


def inside(poly, p):
    """Even-odd, half-open, on integer points."""
    hit = False
    n = len(poly)
    for i in range(n):
        a, b = poly[i], poly[(i + 1) % n]
        if (a[1] > p[1]) != (b[1] > p[1]):
            d = b[1] - a[1]
            lhs, rhs = (p[0] - a[0]) * d, (b[0] - a[0]) * (p[1] - a[1])
            if (lhs < rhs) if d > 0 else (lhs > rhs):
                hit = not hit
    return hit


def side(line, p):
    a, b = line
    return sign((b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]))


def segment_test(line, p_prev, p):
    """A and B not strictly on the same side of the line through p' and p."""
    a, b = line
    u = sub(p, p_prev)
    return sign(cross(u, sub(a, p_prev))) * sign(cross(u, sub(b, p_prev))) <= 0


class ZoneSet:
    """Quantised polygons and lines and the settings, from frame pixels."""

    def __init__(self, img_hw, polygons=(), lines=(), anchor='center', classes=None, coasting=False, heat=None):
        self.img_hw = (int(img_hw[0]), int(img_hw[1]))
        self.polygons = [quantise(poly) for poly in polygons]
        self.lines = [tuple(quantise(line)) for line in lines]
        self.anchor, self.coasting, self.heat = anchor, bool(coasting), heat
        self.classes = None if classes is None else set(int(c) for c in classes)

    def anchor_of(self, box):
        """The float32 anchor of a box row (cx, cy, w, h, angle), or None when a coordinate is not finite."""
        box = np.asarray(box, dtype=np.float32)
        x = box[0]
        with np.errstate(all='ignore'):
            y = box[1] + box[3] / np.float32(2.0) if self.anchor == 'bottom' else box[1]
        if not (np.isfinite(x) and np.isfinite(y)):
            return None
        return (q(x), q(y))


class Slot:
    def __init__(self):
        self.clear()

    def clear(self):
        self.id = 0
        self.inside = [False] * ZMAX
        self.entered = [0] * ZMAX
        self.side = [0] * ZMAX          # the remembered side of every line: 0 = none
        self.p = (0, 0)                 # the previously observed anchor (meaningful once a side is remembered)


class Stream:
    """The state of one stream."""

    def __init__(self, max_tracks):
        self.now = 0
        self.slots = [Slot() for _ in range(max_tracks)]
        self.entries, self.exits, self.lost, self.visits = ([0] * ZMAX for _ in range(4))
        self.pos, self.neg = [0] * ZMAX, [0] * ZMAX
        self.dwell_sum, self.dwell_max = [0] * ZMAX, [0] * ZMAX

    def _leave(self, slot, z):
        d = self.now - slot.entered[z]
        self.visits[z] += 1
        self.dwell_sum[z] += d
        self.dwell_max[z] = max(self.dwell_max[z], d)
        slot.inside[z] = False
        slot.entered[z] = 0

    def frame(self, zs, box, ids, cls, missed, count, heat=None):
        """One frame: box [MT,5], ids, cls, missed [MT], count a number.  Returns the frame's outputs (inside [MT], crossed [MT],
        dwell [MT][Z], occupancy [Z], zone_counts [Z][4], line_counts [L][2]) as lists."""
        Z, L, MT = len(zs.polygons), len(zs.lines), len(self.slots)
        o_inside, o_crossed = [0] * MT, [0] * MT
        o_dwell = [[-1] * Z for _ in range(MT)]
        if count >= 0:                                               # 1. a bad-class frame leaves all of it alone
            for t, slot in enumerate(self.slots):
                tid = int(ids[t])
                if slot.id != 0 and slot.id != tid:                  # 2. close
                    for z in range(ZMAX):
                        if slot.inside[z]:
                            self.lost[z] += 1
                            self._leave(slot, z)
                    slot.clear()
                p = None                                             # 3. observe
                if tid != 0 and (zs.classes is None or int(cls[t]) in zs.classes) and \
                        (missed[t] == 0 or (zs.coasting and missed[t] > 0)):
                    p = zs.anchor_of(box[t])
                if p is not None:
                    if slot.id == 0:
                        slot.id = tid
                    for z, poly in enumerate(zs.polygons):
                        now_in = inside(poly, p)
                        if now_in and not slot.inside[z]:
                            self.entries[z] += 1
                            slot.entered[z] = self.now
                            slot.inside[z] = True
                        elif slot.inside[z] and not now_in:
                            self.exits[z] += 1
                            self._leave(slot, z)
                    for l, line in enumerate(zs.lines):
                        s = side(line, p)
                        if s != 0:
                            if slot.side[l] != 0 and slot.side[l] != s and segment_test(line, slot.p, p):
                                if s > 0:
                                    self.pos[l] += 1
                                    o_crossed[t] |= 1 << (2 * l)
                                else:
                                    self.neg[l] += 1
                                    o_crossed[t] |= 1 << (2 * l + 1)
                            slot.side[l] = s
                    slot.p = p
                    if heat is not None and missed[t] == 0:          # 5. heat
                        H, W = zs.img_hw
                        gh, gw = heat.shape
                        if 0 <= p[0] < 16 * W and 0 <= p[1] < 16 * H:
                            heat[p[1] * gh // (16 * H), p[0] * gw // (16 * W)] += 1
                if slot.id == tid:                                   # 4. the slot's outputs
                    o_inside[t] = sum(1 << z for z in range(Z) if slot.inside[z])
                    for z in range(Z):
                        if slot.inside[z]:
                            o_dwell[t][z] = self.now - slot.entered[z]
        occupancy = [sum(1 for slot in self.slots if slot.inside[z]) for z in range(Z)]
        zone_counts = [[self.entries[z], self.exits[z], self.lost[z], self.visits[z]] for z in range(Z)]
        line_counts = [[self.pos[l], self.neg[l]] for l in range(L)]
        self.now += 1                                                # 6.
        return o_inside, o_crossed, o_dwell, occupancy, zone_counts, line_counts

    def arrays(self):
        """The state as ops.zones_state_views names it (one stream)."""
        mt = len(self.slots)
        code = {0: 0, 1: 1, -1: 2}
        return {
            'now': np.int32(self.now),
            'zone_counts': np.array([[self.entries[z], self.exits[z], self.lost[z], self.visits[z]] for z in range(ZMAX)], np.int32),
            'line_counts': np.array([[self.pos[l], self.neg[l]] for l in range(ZMAX)], np.int32),
            'dwell_max': np.array(self.dwell_max, np.int32),
            'dwell_sum': np.array(self.dwell_sum, np.int64),
            'id': np.array([s.id for s in self.slots], np.int64),
            'inside': np.array([sum(1 << z for z in range(ZMAX) if s.inside[z]) for s in self.slots], np.int32),
            'sides': np.array([sum(code[s.side[l]] << (2 * l) for l in range(ZMAX)) for s in self.slots], np.uint32).view(np.int32),
            'px': np.array([s.p[0] for s in self.slots], np.int32),
            'py': np.array([s.p[1] for s in self.slots], np.int32),
            'entered': np.array([[s.entered[z] for s in self.slots] for z in range(ZMAX)], np.int32).reshape(ZMAX, mt),
        }


def run(zs, streams, track_out, heat=None):
    """F frames of every stream: track_out a dict of numpy arrays box [S,F,MT,5], id, cls, missed [S,F,MT], count [S,F]; streams
    a list of Stream, advanced in place; heat None or int [S,gh,gw], added to in place.  Returns the outputs as int32 arrays
    shaped like ops.zones_frames' (crossed through uint32: bit 31 is line 15's negative direction)."""
    S, F, MT = track_out['id'].shape
    Z, L = len(zs.polygons), len(zs.lines)
    out = {'inside': np.zeros((S, F, MT), np.int32), 'crossed': np.zeros((S, F, MT), np.uint32), 'dwell': np.zeros((S, F, MT, Z), np.int32),
           'occupancy': np.zeros((S, F, Z), np.int32), 'zone_counts': np.zeros((S, F, Z, 4), np.int32),
           'line_counts': np.zeros((S, F, L, 2), np.int32)}
    for s in range(S):
        for f in range(F):
            r = streams[s].frame(zs, track_out['box'][s, f], track_out['id'][s, f], track_out['cls'][s, f], track_out['missed'][s, f],
                                 int(track_out['count'][s, f]), None if heat is None else heat[s])
            out['inside'][s, f], out['crossed'][s, f] = r[0], r[1]
            out['dwell'][s, f] = np.array(r[2], np.int32).reshape(MT, Z)
            out['occupancy'][s, f] = np.array(r[3], np.int32).reshape(Z)
            out['zone_counts'][s, f] = np.array(r[4], np.int32).reshape(Z, 4)
            out['line_counts'][s, f] = np.array(r[5], np.int32).reshape(L, 2)
    out['crossed'] = out['crossed'].view(np.int32)
    return out
