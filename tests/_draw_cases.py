"""Case generator shared by tests/test_draw_host.py and tests/test_gpu_draw.py.  Every box has cx, cy, w, h at multiples of
1/8, so every threshold of the raster rules and every label anchor is exact in float32; only the angle is arbitrary."""
import numpy as np

SIZES = ((96, 160), (95, 157))           # neither a tile multiple; the second odd in both directions


def eighths(rng, lo, hi, n):
    return rng.integers(int(lo * 8), int(hi * 8) + 1, size=n).astype(np.float64) / 8.0


def random_boxes(seed, H, W, K, rotated):
    """float32 [K, 5] rows (cx, cy, w, h, deg): centres inside the frame, sizes 4 .. half the frame."""
    rng = np.random.default_rng(seed)
    b = np.zeros((K, 5), dtype=np.float64)
    b[:, 0], b[:, 1] = eighths(rng, 0, W, K), eighths(rng, 0, H, K)
    b[:, 2], b[:, 3] = eighths(rng, 4, W / 2, K), eighths(rng, 4, H / 2, K)
    if rotated:
        b[:, 4] = rng.uniform(-180.0, 180.0, size=K)
    return b.astype(np.float32)


def rotated_cases():
    """[(name, H, W, thickness, fill_alpha, boxes [B][K,5])]: the rotated cases of the GPU test, B = 2 with different K."""
    out = []
    for n, (H, W) in enumerate(SIZES):
        for t, alpha, seed in ((2, 0, 11), (3, 96, 12), (6, 0, 13)):
            out.append((f'rot_{H}x{W}_t{t}_a{alpha}', H, W, t, alpha,
                        [random_boxes(100 * n + seed, H, W, 9, True), random_boxes(100 * n + seed + 50, H, W, 5, True)]))
    return out


def axis_boxes(H, W):
    """Axis-aligned rows with pixel centres exactly on thresholds: integer and half-integer edges, eighths, thin boxes."""
    return np.array([[40.5, 30.5, 21.0, 11.0, 0], [80.0, 48.0, 40.0, 24.0, 0], [20.125, 60.375, 17.25, 9.5, 0],
                     [120.0, 20.0, 3.0, 30.0, 0], [W - 10.0, H - 8.0, 30.0, 30.0, 0], [60.5, 70.0, 1.0, 1.0, 0],
                     [100.0, 64.5, 0.125, 12.0, 0]], dtype=np.float32)


def clip_skip_boxes(H, W):
    """Half and fully outside, larger than the frame, w = 0, NaN and inf rows, a negative height."""
    nan, inf = float('nan'), float('inf')
    return np.array([[0.0, 20.0, 30.0, 16.0, 0], [W + 0.0, H + 0.0, 24.0, 24.0, 30.0], [-100.0, -100.0, 20.0, 20.0, 0],
                     [W / 2, H / 2, 3.0 * W, 3.0 * H, 0], [W / 2, H / 2, 2.0 * W + 2, 2.0 * H + 2, 12.5],
                     [50.0, 50.0, 0.0, 10.0, 0], [nan, 50.0, 10.0, 10.0, 0], [50.0, 50.0, inf, 10.0, 0],
                     [50.0, 50.0, 10.0, 10.0, nan], [50.0, 40.0, 10.0, -4.0, 0], [3e9, 10.0, 20.0, 20.0, 0],
                     [70.0, 40.0, 12.0, 18.0, 0]], dtype=np.float32)


def label_boxes(H, W):
    """Boxes whose labels meet all four frame-edge clamps (left, top, right, bottom) and one in the open."""
    return np.array([[-20.0, 50.0, 30.0, 20.0, 0], [60.0, 4.0, 30.0, 20.0, 0], [W + 10.0, 60.0, 40.0, 20.0, 0],
                     [50.0, H + 60.0, 30.0, 20.0, 0], [70.5, 60.25, 30.0, 24.0, 0], [100.0, 40.0, 16.0, 16.0, 33.0]], dtype=np.float32)
