"""Writes tests/golden/kf_tracklet.npz: the Kalman-tracklet fixture (build container only -- it imports the reference).

A few seeded measurement sequences run through the reference's KFTracklet (utils/structures.py:445-529, over
RotBBoxKalmanFilter, utils/kalman_filter.py:77-142) in float64.  A step is predict(), then update(z, score) when the frame
has a measurement.  Stored per sequence and step, padded to the longest sequence:
  z [N,T,5] float32 (NaN: no measurement), z_score [N,T] float32, has_z [N,T] bool       the inputs
  x [N,T,10], P [N,T,10,10] float64      the filter state after the step (P whole: its off-block entries must be 0)
  score [N,T] float64, pred_count [N,T], feasible [N,T] bool, box [N,T,5] float64 (the box the call returned)
and init_box [N,5] float32, init_score [N] float32, length [N], names [N], img_hw.  The sequences: plain motion; the angle
crossing 179 -> 1 degrees and back; runs of missed frames, the last long enough for the score to fall through 0.1; a box that
leaves the image; raw angles of -30 and of 400 degrees.  Measurements are float32 values, which is what a record holds.
Only these arrays are stored; nothing of the reference's program text is.

    python tools/gen_golden_track.py
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMG_HW = (480, 640)


def sequences(seed=0):
    """name -> (init box [5], init score, [(z [5], score) or None per step]), all float32."""
    rng = np.random.Generator(np.random.PCG64(seed))
    f32 = np.float32

    def run(start, vel, steps, missing=(), noise=(1.0, 1.0, 1.0, 1.0, 1.0), raw_angle=None):
        box = np.array(start, np.float64)
        out = []
        for t in range(1, steps + 1):
            true = box + np.array(vel, np.float64) * t
            if t in missing:
                out.append(None)
                continue
            z = true + rng.uniform(-1, 1, 5) * np.array(noise)
            z[4] = z[4] % 180 if raw_angle is None else raw_angle + (z[4] - true[4])
            out.append((z.astype(f32), f32(rng.uniform(0.5, 0.95))))
        return np.array(start, f32), f32(0.9), out

    seqs = {
        'plain': run((500, 300, 80, 40, 30), (3, 1.5, 0.4, -0.2, 0.5), 40),
        'wrap_up': run((300, 200, 90, 50, 170), (1, 2, 0, 0, 1.5), 30),
        'wrap_down': run((300, 200, 90, 50, 10), (-2, 1, 0, 0, -1.5), 30),
        'missed': run((200, 240, 60, 120, 80), (2, -1, 0.2, 0.3, 0.3), 40, missing=set(range(8, 11)) | set(range(22, 41))),
        'leaving': run((560, 100, 60, 50, 45), (12, 0.5, 0, 0, 0), 14),
        'raw_m30': run((320, 240, 100, 40, -30), (1, 1, 0, 0, 0), 12, raw_angle=-30.0),
        'raw_400': run((320, 240, 100, 40, 400), (-1, 2, 0, 0, 0), 12, raw_angle=400.0),
    }
    return seqs


def main():
    try:
        import scipy.linalg  # noqa: F401
    except ImportError:                                              # imported by the reference's kalman_filter.py, never called
        sys.modules['scipy'] = types.ModuleType('scipy')
        sys.modules['scipy.linalg'] = sys.modules['scipy'].linalg = types.ModuleType('scipy.linalg')
    from oracle import _refimport
    _refimport.install()
    from utils.structures import KFTracklet
    np.bool = bool                                                   # the reference predates numpy 1.24; set after every import

    seqs = sequences()
    names = list(seqs)
    N, T = len(names), max(len(s[2]) for s in seqs.values())
    z = np.full((N, T, 5), np.nan, np.float32)
    z_score = np.zeros((N, T), np.float32)
    has_z = np.zeros((N, T), bool)
    x = np.zeros((N, T, 10))
    P = np.zeros((N, T, 10, 10))
    score = np.zeros((N, T))
    pred_count = np.zeros((N, T), np.int64)
    feasible = np.zeros((N, T), bool)
    box = np.zeros((N, T, 5))
    init_box = np.zeros((N, 5), np.float32)
    init_score = np.zeros(N, np.float32)
    length = np.zeros(N, np.int64)
    for i, name in enumerate(names):
        b0, s0, steps = seqs[name]
        init_box[i], init_score[i], length[i] = b0, s0, len(steps)
        trk = KFTracklet(b0.astype(np.float64), float(s0), object_id=1, img_hw=IMG_HW)
        for t, m in enumerate(steps):
            ret = trk.predict()
            if m is not None:
                z[i, t], z_score[i, t], has_z[i, t] = m[0], m[1], True
                ret = trk.update(m[0].astype(np.float64), float(m[1]))
            x[i, t], P[i, t], score[i, t], pred_count[i, t] = trk.kf.x, trk.kf.P, trk.score, trk._pred_count
            feasible[i, t], box[i, t] = trk.is_feasible(), ret
        print(f'{name:10s} {len(steps):3d} steps, {int(has_z[i].sum()):3d} measured, feasible until '
              f'{int(np.argmin(feasible[i, :len(steps)])) if not feasible[i, :len(steps)].all() else len(steps)}, final score {score[i, len(steps) - 1]:.4f}')
    out = os.path.join(ROOT, 'tests', 'golden', 'kf_tracklet.npz')
    np.savez_compressed(out, names=np.array(names), img_hw=np.array(IMG_HW, np.int64), init_box=init_box, init_score=init_score,
                        length=length, z=z, z_score=z_score, has_z=has_z, x=x, P=P, score=score, pred_count=pred_count,
                        feasible=feasible, box=box)
    size = os.path.getsize(out)
    print(out, size, 'bytes')
    assert size < 256 * 1024


if __name__ == '__main__':
    main()
