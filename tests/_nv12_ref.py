"""The NV12 -> RGB conversion restated in numpy, independent of the library (int32 arithmetic, >> 8, np.clip), and the frames
the NV12 tests share.

    D = U - 128, E = V - 128, C = Y - 16 (limited range) or Y (full range)
    R = clip8((cy*C         + crv*E + 128) >> 8)
    G = clip8((cy*C - cgu*D - cgv*E + 128) >> 8)
    B = clip8((cy*C + cbu*D         + 128) >> 8)
Chroma is nearest-neighbour: pixel (y, x) uses the (U, V) pair at (y >> 1, x >> 1)."""
import numpy as np

# (matrix, full_range) -> cy, crv, cgu, cgv, cbu
TABLE = {
    ('bt601', False): (298, 409, 100, 208, 516),
    ('bt709', False): (298, 459, 55, 136, 541),
    ('bt601', True): (256, 359, 88, 183, 454),
    ('bt709', True): (256, 403, 48, 120, 475),
}


def table_from_matrices():
    """The same table from its definition: round(256 * x) of the BT.601 / BT.709 matrices."""
    out = {}
    for name, (kr, kb) in (('bt601', (0.299, 0.114)), ('bt709', (0.2126, 0.0722))):
        kg = 1.0 - kr - kb
        for full in (False, True):
            sy, sc = (1.0, 1.0) if full else (255.0 / 219.0, 255.0 / 224.0)
            out[(name, full)] = tuple(int(round(256 * v)) for v in (
                sy, 2 * (1 - kr) * sc, 2 * kb * (1 - kb) / kg * sc, 2 * kr * (1 - kr) / kg * sc, 2 * (1 - kb) * sc))
    return out


def nv12_to_rgb(y, uv, matrix='bt601', full_range=False):
    """y: uint8 [..., H, W]; uv: uint8 [..., ceil(H/2), ceil(W/2), 2] -> uint8 [..., H, W, 3]."""
    cy, crv, cgu, cgv, cbu = TABLE[(matrix, bool(full_range))]
    H, W = y.shape[-2:]
    assert uv.shape[-3:] == ((H + 1) // 2, (W + 1) // 2, 2) and y.dtype == uv.dtype == np.uint8
    rows, cols = np.arange(H) >> 1, np.arange(W) >> 1
    near = uv[..., rows, :, :][..., cols, :].astype(np.int32)
    C = y.astype(np.int32) - (0 if full_range else 16)
    D, E = near[..., 0] - 128, near[..., 1] - 128
    r = np.clip((cy * C + crv * E + 128) >> 8, 0, 255)
    g = np.clip((cy * C - cgu * D - cgv * E + 128) >> 8, 0, 255)
    b = np.clip((cy * C + cbu * D + 128) >> 8, 0, 255)
    return np.stack([r, g, b], axis=-1).astype(np.uint8)


def random_nv12(b, h, w, seed):
    """(y [b,h,w], uv [b,ceil(h/2),ceil(w/2),2]) of random bytes: every value of every plane, so clipped pixels too."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.integers(0, 256, size=(b, h, w), dtype=np.uint8),
            rng.integers(0, 256, size=(b, (h + 1) // 2, (w + 1) // 2, 2), dtype=np.uint8))


def clip_frame():
    """Y is a 0..255 ramp across W = 256; each pair of rows carries one (U, V) of {0, 16, 128, 240, 255}^2: H = 50.  Every clip
    branch of every channel and negative values under the shift occur."""
    levels = (0, 16, 128, 240, 255)
    y = np.broadcast_to(np.arange(256, dtype=np.uint8), (50, 256)).copy()
    uv = np.zeros((25, 128, 2), np.uint8)
    for i, (u, v) in enumerate((u, v) for u in levels for v in levels):
        uv[i] = (u, v)
    return y[None], uv[None]
