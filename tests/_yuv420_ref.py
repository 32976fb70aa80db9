"""The 4:2:0 layouts restated in numpy, independent of the library: any layout is repacked to NV12 planes (interleave, swap,
10-bit reduction), which _nv12_ref.nv12_to_rgb turns into RGB.  Plane order is the storage order of the layout:

    nv12, p010: (y, uv) with (U, V) pairs        nv21: (y, vu) with (V, U) pairs
    i420, i010: (y, u, v)                        yv12: (y, v, u)
    p010: 16-bit words, v10 = word >> 6          i010: 16-bit words, v10 = word & 1023
    s8 = min(255, (v10 + 2) >> 2)"""
import numpy as np

import _nv12_ref

LAYOUTS = ('nv12', 'nv21', 'i420', 'yv12', 'p010', 'i010')
PLANAR = ('i420', 'yv12', 'i010')
WORDS = ('p010', 'i010')


def reduce10(v10):
    """10-bit sample values -> uint8 by the rule of include/mydet.h."""
    v = np.asarray(v10).astype(np.int64)
    assert v.min() >= 0 and v.max() <= 1023
    return np.minimum(255, (v + 2) >> 2).astype(np.uint8)


def samples8(plane, layout):
    """A stored plane as uint8 samples."""
    if layout not in WORDS:
        assert plane.dtype == np.uint8
        return plane
    assert plane.dtype == np.uint16
    return reduce10(plane >> 6 if layout == 'p010' else plane & 1023)


def to_nv12(planes, layout):
    """The planes of `layout` (storage order) as NV12 planes (y uint8 [..., H, W], uv uint8 [..., ceil(H/2), ceil(W/2), 2])."""
    s = [samples8(p, layout) for p in planes]
    if layout in ('nv12', 'p010'):
        y, uv = s
    elif layout == 'nv21':
        y, uv = s[0], s[1][..., ::-1]
    elif layout in ('i420', 'i010'):
        y, uv = s[0], np.stack([s[1], s[2]], axis=-1)
    else:
        assert layout == 'yv12'
        y, uv = s[0], np.stack([s[2], s[1]], axis=-1)
    return np.ascontiguousarray(y), np.ascontiguousarray(uv)


def to_rgb(planes, layout, matrix='bt601', full_range=False):
    return _nv12_ref.nv12_to_rgb(*to_nv12(planes, layout), matrix, full_range)


def words10(v10, layout, rng):
    """10-bit values as the 16-bit words of `layout`, the six ignored bits random (low for p010, high for i010)."""
    v = np.asarray(v10).astype(np.uint16)
    junk = rng.integers(0, 64, size=v.shape, dtype=np.uint16)
    return (v << 6 | junk) if layout == 'p010' else (v | junk << 10)


def expand10(s8, rng):
    """10-bit values that reduce to the uint8 samples s8: 4 * s + (-2 .. 1), and all of 1018 .. 1023 for s = 255."""
    s = np.asarray(s8).astype(np.int64)
    v = np.clip(4 * s + rng.integers(-2, 2, size=s.shape), 0, 1023)
    v = np.where(s == 255, rng.integers(1018, 1024, size=s.shape), v)
    assert np.array_equal(reduce10(v), s8)
    return v


def _arrange(y, u, v, layout):
    if layout in ('nv12', 'p010'):
        return y, np.stack([u, v], axis=-1)
    if layout == 'nv21':
        return y, np.stack([v, u], axis=-1)
    return (y, v, u) if layout == 'yv12' else (y, u, v)


def from_values10(y, u, v, layout, rng):
    """Planes of a 16-bit layout from 10-bit values."""
    assert layout in WORDS
    return _arrange(*(words10(p, layout, rng) for p in (y, u, v)), layout)


def from_samples(y, u, v, layout, rng=None):
    """Planes of `layout` whose 8-bit samples are the uint8 planes y, u, v (for the 16-bit layouts: expand10, random ignored bits)."""
    if layout in WORDS:
        return from_values10(*(expand10(p, rng) for p in (y, u, v)), layout, rng)
    return _arrange(y, u, v, layout)


def from_nv12(y, uv, layout, seed=0):
    """from_samples of NV12 planes; to_nv12 of the result is (y, uv) again."""
    planes = from_samples(y, np.ascontiguousarray(uv[..., 0]), np.ascontiguousarray(uv[..., 1]), layout, np.random.Generator(np.random.PCG64(seed)))
    planes = tuple(np.ascontiguousarray(p) for p in planes)
    back = to_nv12(planes, layout)
    assert np.array_equal(back[0], y) and np.array_equal(back[1], uv)
    return planes


def random_planes(layout, b, h, w, seed):
    """Random planes: every byte value for the 8-bit layouts, every 16-bit word (so every ignored bit too) for the others."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ch, cw = (h + 1) // 2, (w + 1) // 2
    dt, hi = (np.uint16, 65536) if layout in WORDS else (np.uint8, 256)
    shapes = [(b, h, w)] + ([(b, ch, cw)] * 2 if layout in PLANAR else [(b, ch, cw, 2)])
    return tuple(rng.integers(0, hi, size=s, dtype=dt) for s in shapes)


def clip_frame(layout):
    """_nv12_ref.clip_frame() in `layout`.  For the 16-bit layouts a sample s < 255 is the 10-bit value 4 * s, and the samples
    of value 255 cycle through 1020, 1021, 1022, 1023 (all reduce to 255: the rounding and the clamp); ignored bits random."""
    y, uv = _nv12_ref.clip_frame()
    u, v = uv[..., 0], uv[..., 1]
    if layout not in WORDS:
        return tuple(np.ascontiguousarray(p) for p in _arrange(y, u, v, layout))

    def ten(p):
        q = p.astype(np.uint16) * 4
        top = np.flatnonzero(p == 255)
        q.reshape(-1)[top] = 1020 + np.arange(top.size) % 4
        return q
    return tuple(np.ascontiguousarray(p) for p in from_values10(ten(y), ten(u), ten(v), layout, np.random.Generator(np.random.PCG64(10))))
