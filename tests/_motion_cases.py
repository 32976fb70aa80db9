"""Case tables of tests/test_gpu_motion_branches.py: the scenes that send the camera-motion kernels (csrc/motion.hip) down every
branch they compile, as host arrays, and what the restatement (tests/_motion_ref.py) makes of each, computed once per process.
tests/test_motion_cases_host.py proves on the restatement alone that each case is what it claims to be.  Test code; no device.

A case is a dict: hw, set (the keywords of ops.motion_set), source ('rgb' or a 4:2:0 layout), form (how the frames lie in
memory: 'packed', 'wide', 'narrow' -- test_gpu_motion_branches.py builds them) and what its scene builder needs."""
import functools

import numpy as np

import _motion_ref as ref

MARGIN = 160
LAYOUTS = ('nv12', 'nv21', 'i420', 'p010', 'i010')


@functools.lru_cache(maxsize=None)
def coarse(seed):
    """Coarse textures for every reduction; about one cell in sixteen is saturated (255), for the 10-bit clamp."""
    return ref.coarse_texture(600, 800, seed, saturate=16)


@functools.lru_cache(maxsize=None)
def fine(seed, hw=(512, 640)):
    return ref.texture(hw[0], hw[1], seed)


# ---- A. every instance ----
# k -> frame size (neither side a multiple of k, both odd, wr % 4 != 0), R, and per stream the true shifts: none a multiple of
# k in both components, one component at +-R k
SHAPES = {2: ((83, 119), 4, (((3, -5), (-8, 7), (1, 8)), ((-3, 2), (8, -7), (5, 5)))),
          4: ((131, 191), 7, (((5, -11), (-28, 27), (3, 28)), ((-9, 6), (28, -25), (-13, -28)))),
          8: ((197, 459), 4, (((13, -29), (-32, 31), (-1, 32)), ((-7, 10), (32, -31), (29, -32))))}
TWO_STREAMS = ('nv12-k4-wide', 'i010-k4-narrow', 'p010-k8-wide', 'i420-k8-narrow')


def _instances():
    out = {}
    for k in (4, 8):
        for source in ('rgb',) + LAYOUTS:
            for form in ('wide', 'narrow'):
                out[f'{source}-k{k}-{form}'] = dict(k=k, source=source, form=form)
    for source in LAYOUTS:                                           # k = 2: the only reduction whose rows end inside a quad
        out[f'{source}-k2-wide'] = dict(k=2, source=source, form='wide')
    for name, c in out.items():
        hw, R, shifts = SHAPES[c['k']]
        c.update(hw=hw, set=dict(reduce=c['k'], search=R), shifts=shifts[:2 if name in TWO_STREAMS else 1])
    return out


INSTANCES = _instances()


def _instance_scene(c):
    """RGB: one texture per channel; 4:2:0: one texture as the luma.  uint8 [S, F, H, W(, 3)]."""
    seeds = ((0, 1, 2), (2, 3, 0))
    frames = []
    for s, shifts in enumerate(c['shifts']):
        off = ref.offsets_of_shifts(shifts, MARGIN)
        if c['source'] == 'rgb':
            frames.append(np.stack([ref.crops(coarse(seed), c['hw'], off) for seed in seeds[s]], axis=-1))
        else:
            frames.append(ref.crops(coarse(seeds[s][0]), c['hw'], off))
    return np.stack(frames)


# ---- C. medians that decide; G. thresholds at equality ----
# Six blocks (2 x 3).  Both textures are flat from column flat_x of the first frame on, which covers the right block column and
# its whole search window in both frames: two invalid blocks (SAD 0 everywhere), and the edge moves with the content of the
# middle column, which stays valid.  The upper block row shows texture b moving by `b`, the lower one texture a moving by `a`:
# the lower medians take x from the `a` blocks and y from the `b` blocks, and both motions are inside the refine window round
# the coarse median.
MEDIANS = {'96x128-k2': dict(hw=(96, 128), set=dict(reduce=2, search=8), a=(-4, 0), b=(-2, -2), cut_y=48, flat_x=64),
           '160x224-k4': dict(hw=(160, 224), set=dict(reduce=4, search=4), a=(-7, -1), b=(-5, -5), cut_y=80, flat_x=128)}
for _c in MEDIANS.values():
    _c.update(source='rgb', form='packed')


def _medians_scene(c):
    H, W = c['hw']
    flat = np.mgrid[:512, :640][1] >= MARGIN + c['flat_x']           # painted on the textures: its edge moves with them
    tex_a, tex_b = (ref.partly_flat(fine(seed), flat) for seed in (7, 8))
    return ref.two_motions(tex_a, tex_b, c['hw'], [c['a']], [c['b']], np.mgrid[:H, :W][0] < c['cut_y'], MARGIN)[None]


THRESHOLDS = ('texture_equal', 'texture_above', 'blocks_equal', 'blocks_above')
THRESHOLD_BASE = '96x128-k2'


def threshold_case(which):
    """The median scene under a min_texture or a min_blocks at, or one above, what the restatement's block rows hold."""
    base = MEDIANS[THRESHOLD_BASE]
    g, _, blocks, _ = want('medians', THRESHOLD_BASE)
    rows = [r for r in blocks[0, 1] if ref.block_valid(r, g)]
    least = min(int(r[3] - r[2]) for r in rows)
    extra = {'texture_equal': dict(min_texture=least), 'texture_above': dict(min_texture=least + 1),
             'blocks_equal': dict(min_blocks=len(rows)), 'blocks_above': dict(min_blocks=len(rows) + 1)}[which]
    return dict(base, set=dict(base['set'], **extra))


# ---- D. more blocks than threads ----
MANY = {'272': dict(hw=(560, 528), nb=272), '1024': dict(hw=(1040, 1040), nb=1024)}
for _c in MANY.values():
    _c.update(set=dict(reduce=2, search=4), source='rgb', form='packed', a=(-6, 0), b=(-4, -2))


def _many_scene(c):
    H, W = c['hw']
    big = (1120, 1120)
    return ref.two_motions(fine(7, big), fine(8, big), c['hw'], [c['a']], [c['b']], np.mgrid[:H, :W][1] >= W // 2, 40)[None]


# ---- E. equal minima ----
# k = 2, R = 8.  x, y: period 8 reduced pixels, moved by 4: candidates -4 and +4 tie at the same distance and the smaller dx (dy)
# wins.  both: period 4 along both axes, moved by 2: -6, -2, 2, 6 tie along each axis, and the distance decides first.
# diagonal: the texture repeats under (dx, dy) = (4, -4) only, moved by (2, -2): (2, -2) and (-2, 2) tie at one distance, and dy
# is compared before dx.
PERIODIC = {'x': dict(period=(None, 16), shift=(8, 0)), 'y': dict(period=(16, None), shift=(0, 8)),
            'both': dict(period=(8, 8), shift=(4, 4)), 'diagonal': dict(period=16, shift=(4, -4))}
for _c in PERIODIC.values():
    _c.update(hw=(96, 128), set=dict(reduce=2, search=8), source='rgb', form='packed')


def _periodic_scene(c):
    build = ref.diagonal if isinstance(c['period'], int) else ref.periodic
    return build(c['hw'], c['period'], c['shift'], seed=5)[None]


# ---- F. odd radii ----
ODD = {'R5-k2': dict(hw=(83, 117), set=dict(reduce=2, search=5), shifts=((3, -10), (-10, 9), (9, 10))),
       'R15-k2': dict(hw=(99, 141), set=dict(reduce=2, search=15), shifts=((-30, 29), (30, -13), (7, 30))),
       'R7-k4': dict(hw=(131, 190), set=dict(reduce=4, search=7), shifts=((5, -11), (-28, 27), (3, 28))),
       'R5-k8': dict(hw=(213, 339), set=dict(reduce=8, search=5), shifts=((13, -37), (-40, 39), (-1, 40)))}
for _c in ODD.values():
    _c.update(source='rgb', form='packed', shifts=(_c['shifts'],))

GROUPS = {'instance': (INSTANCES, _instance_scene), 'medians': (MEDIANS, _medians_scene), 'many': (MANY, _many_scene),
          'periodic': (PERIODIC, _periodic_scene), 'odd': (ODD, _instance_scene)}


def case(group, name):
    return threshold_case(name) if group == 'threshold' else GROUPS[group][0][name]


@functools.lru_cache(maxsize=None)
def scene(group, name):
    """(pixels, lumas int64 [S, F, H, W]) of a case.  pixels: uint8 [S, F, H, W, 3] for 'rgb' (a grey scene has R = G = B, whose
    luma is the grey value), else the Y plane as the layout stores it [S, F, H, W] (uint8, or int16 words).  Never written to."""
    c = case(group, name)
    px = (_medians_scene(c) if group == 'threshold' else GROUPS[group][1](c))
    if c['source'] == 'rgb':
        if px.ndim == 4:
            px = np.repeat(px[..., None], 3, axis=-1)
        lumas = ref.luma_rgb(px)
    else:
        y8 = px
        px = ref.store_y(y8, c['source'], np.random.default_rng(11))
        lumas = ref.luma_y(px, c['source'])
        assert np.array_equal(lumas, y8), 'the 10-bit rule gives back y'
    for a in (px, lumas):
        a.setflags(write=False)
    return px, lumas


@functools.lru_cache(maxsize=None)
def want(group, name):
    """(geometry, shift [S, F, 4], blocks [S, F, nb, 6], the streams after the last frame) of the restatement, computed once."""
    c = case(group, name)
    _, lumas = scene(group, name)
    g = ref.Geometry(c['hw'], c['set'].get('reduce'), c['set'].get('search', 8), c['set'].get('min_texture', 1024), c['set'].get('min_blocks'))
    streams = [ref.Stream(g) for _ in range(lumas.shape[0])]
    shift, blocks = ref.run(streams, lumas)
    for a in (shift, blocks):
        a.setflags(write=False)
    return g, shift, blocks, streams
