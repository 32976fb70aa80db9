"""Case tables of tests/test_warp_host.py and tests/test_gpu_warp.py: warped scenes as host arrays and what the restatement
(tests/_warp_ref.py) makes of each, computed once per process.  Test code; no device.

A case is a dict: hw, set (the keywords of ops.motion_set beside model='similarity'), source ('rgb' or a 4:2:0 layout), and
`truths`, per stream the true models (degrees, zoom, shift) of frames 1, 2, ... -- each the warp of the stream's FIRST frame, so
frame 1 against frame 0 shows truths[0] and later pairs show the composition.  A bilinear warp is fine: the kernel is held to the
restatement, and only the host test holds the restatement to the truth.

Measured corner errors of the restatement (pixels; seeds 1, 2, 3 of the texture), from which BOUND below is the largest doubled:
    320 x 448, k 2, R 8, 117 blocks,  1.5 deg, zoom 1.02, shift (5.3, -3.6):   0.043  0.060  0.094
    320 x 448, k 2, R 8, 117 blocks, -2.5 deg, zoom 0.97, shift (-4, 2):       0.182  0.069  0.200
    262 x 382, k 4, R 7,  15 blocks,  3 deg, no zoom, no shift:                0.289  0.437  0.334
    320 x 448, pure shift (7, -9):                                             exact"""
import functools

import numpy as np

import _motion_ref as mref
import _warp_ref as ref

# twice the largest measured error of each geometry (the texture seed moves it)
BOUND = {(320, 448): 0.40, (262, 382): 0.88}
SEED = 1

SCENES = {'turn_zoom_in': dict(hw=(320, 448), set=dict(reduce=2, search=8), truths=(((1.5, 1.02, (5.3, -3.6)),),)),
          'turn_zoom_out': dict(hw=(320, 448), set=dict(reduce=2, search=8), truths=(((-2.5, 0.97, (-4, 2)),),)),
          'turn_k4': dict(hw=(262, 382), set=dict(reduce=4, search=7), truths=(((3.0, 1.0, (0, 0)),),)),
          'pure_shift': dict(hw=(320, 448), set=dict(reduce=2, search=8), truths=(((0.0, 1.0, (7, -9)),),))}
for _c in SCENES.values():
    _c.update(source='rgb')

# every reduction at the smallest shapes of _motion_cases.SHAPES, per source; the turns are small: few blocks, short arms
_SMALL = {2: ((83, 119), 4, (((1.0, 1.01, (2, -3)), (-1.5, 0.99, (-3, 1))), ((-1.0, 1.02, (-2, 2)), (0.8, 1.0, (3, 3))))),
          4: ((131, 191), 7, (((1.5, 1.02, (5, -6)), (-1.0, 0.98, (-9, 4))), ((-2.0, 1.0, (7, 3)), (1.0, 1.03, (-4, -8))))),
          8: ((197, 459), 4, (((0.5, 1.01, (9, -11)), (-0.5, 0.99, (-13, 6))), ((0.8, 1.0, (-7, 10)), (-0.3, 1.02, (12, -5)))))}
REDUCTIONS = {}
for _k, (_hw, _R, _tr) in _SMALL.items():
    for _src in ('rgb', 'nv12', 'p010'):
        REDUCTIONS[f'{_src}-k{_k}'] = dict(hw=_hw, set=dict(reduce=_k, search=_R), source=_src, truths=_tr[:1])
REDUCTIONS['rgb-k4-two-streams'] = dict(hw=_SMALL[4][0], set=dict(reduce=4, search=7), source='rgb', truths=_SMALL[4][2])
REDUCTIONS['nv12-k2-two-streams'] = dict(hw=_SMALL[2][0], set=dict(reduce=2, search=4), source='nv12', truths=_SMALL[2][2])

# k = 4 once more on the 4:2:0 sources at a shape with six blocks: the smallest k = 4 shape has two, too few for any fit
for _src in ('nv12', 'p010'):
    REDUCTIONS[f'{_src}-k4-six-blocks'] = dict(hw=(197, 251), set=dict(reduce=4, search=7), source=_src, truths=_SMALL[4][2][:1])

MANY = {'272': dict(hw=(560, 528), set=dict(reduce=2, search=4), source='rgb', truths=(((0.4, 1.005, (3, -2)),),))}

# a call of three frames, for the 1 + 2 split
SPLIT = {'split': dict(hw=_SMALL[2][0], set=dict(reduce=2, search=4), source='rgb', truths=_SMALL[2][2])}

# the invalid exits of the fit that pixels can reach (the others are guards: tests/test_warp_host.py holds them on the fit alone)
INVALID = {'rotation_cap': dict(hw=(320, 448), set=dict(reduce=2, search=8, max_rotation=1.0), truths=(((3.0, 1.0, (0, 0)),),)),
           'zoom_cap': dict(hw=(320, 448), set=dict(reduce=2, search=8, max_zoom=0.01), truths=(((0.0, 1.03, (1, 1)),),)),
           'few_inliers': dict(hw=(320, 448), set=dict(reduce=2, search=8, tolerance=0.0005), truths=(((2.0, 1.02, (0.5, 0.5)),),)),
           'one_pair': dict(hw=(96, 128), set=dict(reduce=2, search=8, min_blocks=2), truths=(((0.0, 1.0, (3, -2)),),), keep_blocks=2),
           'no_pair': dict(hw=(96, 128), set=dict(reduce=2, search=8, min_blocks=1), truths=(((0.0, 1.0, (3, -2)),),), keep_blocks=1)}
for _c in INVALID.values():
    _c.update(source='rgb')

# a quarter of the blocks shows another motion: the left 3 of 13 block columns, 27 of 117 blocks
OUTLIERS = {'quarter': dict(hw=(320, 448), set=dict(reduce=2, search=8), source='rgb', truths=(((1.5, 1.02, (5.3, -3.6)),),),
                            foreign=(0.0, 1.0, (-6, 7)), foreign_x=16 + 32 * 3)}

GROUPS = {'scene': SCENES, 'reduction': REDUCTIONS, 'many': MANY, 'split': SPLIT, 'invalid': INVALID, 'outliers': OUTLIERS}


def case(group, name):
    return GROUPS[group][name]


def _stream_frames(c, s):
    truths = [ref.true_model(*t) for t in c['truths'][s]]
    fr = ref.scene(c['hw'], SEED + 10 * s, truths)
    if 'foreign' in c:                                               # the region keeps its place; its content moves otherwise
        other = ref.scene(c['hw'], SEED + 5, [ref.true_model(*c['foreign'])])
        fr[:, :, :c['foreign_x']] = other[:, :, :c['foreign_x']]
    if 'keep_blocks' in c:                                           # flat but for the first blocks of the upper block row:
        g = geometry(c)                                              # the texture ends where the next block's window begins
        keep = np.zeros(c['hw'], bool)
        keep[:16 * g.k, :16 * c['keep_blocks'] * g.k] = True
        fr = np.where(keep[None], fr, 90).astype(np.uint8)
    return fr


def geometry(c):
    s = c['set']
    return mref.Geometry(c['hw'], s.get('reduce'), s.get('search', 8), s.get('min_texture', 1024), s.get('min_blocks'))


def fit_of(c):
    s = c['set']
    return ref.Fit(s.get('tolerance', 2.0), s.get('max_zoom'), s.get('max_rotation'))


@functools.lru_cache(maxsize=None)
def scene(group, name):
    """(y8 uint8 [S, F, H, W], lumas int64 [S, F, H, W]) of a case: grey frames; an RGB source shows them as R = G = B, whose luma
    is the grey value, a 4:2:0 source as its Y plane.  Never written to."""
    c = case(group, name)
    y8 = np.stack([_stream_frames(c, s) for s in range(len(c['truths']))])
    lumas = y8.astype(np.int64)
    for a in (y8, lumas):
        a.setflags(write=False)
    return y8, lumas


@functools.lru_cache(maxsize=None)
def want(group, name):
    """(geometry, the restatement's output dict, the streams after the last frame), computed once."""
    c = case(group, name)
    _, lumas = scene(group, name)
    g = geometry(c)
    streams = [ref.Stream(g, fit_of(c)) for _ in range(lumas.shape[0])]
    out = ref.run(streams, lumas)
    for a in out.values():
        a.setflags(write=False)
    return g, out, streams
