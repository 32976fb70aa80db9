"""Time mydet_decode_levels_f32 / mydet_decode_uv5_levels_f32 alone on the head layouts at bench sizes (HBM roofline check).

    python tools/bench_decode.py [--batch 32] [--size 640] [--iters 200] [--only yolo]
    python tools/bench_decode.py --ab uv5,yolo [--runs 5]

Prints one line per layout: average launch time (HIP events on the launch stream), algorithmic bytes, GB/s and the
fraction of the 8 TB/s HBM peak.  `uv5` is the Ultralytics decode on the very tensors of `yolo`.  --ab A,B times two
layouts in one process, their runs of --iters launches interleaved (A B A B ...), and prints every run, the two medians
and median(A) / median(B).
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mydetection_amd import ops  # noqa: E402


def layouts(B, S):
    dev = 'cuda'
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    out = {}
    # YOLOv3: one [B,H,W,255] tensor per level, anchor-major channels (85 per anchor)
    lv, n = [], 0
    for st in (8, 16, 32):
        H = S // st
        t = rnd(B, H, H, 256)[..., :255]          # ld 256 keeps rows 16-byte aligned like the product's head conv
        lv.append(dict(box=t, ldbox=256, cls=t, ldcls=256, anchors_wh=[[10, 13], [16, 30], [33, 23]], H=H, W=H,
                       stride=st, n_off=n))
        n += 3 * H * H
    out['yolo'] = (ops.DECODE_YOLO, lv, dict(box_astride=85, box_c0=0, cls_astride=85, cls_c0=5, conf_c0=4, A=3, C=80), n)
    out['uv5'] = ('uv5', lv, out['yolo'][2], n)       # the same tensors through mydet_decode_uv5_levels_f32
    # RetinaNet head: box [B,H,W,36] and cls [B,H,W,720] per level, 9 anchors
    lv, n = [], 0
    for st in (8, 16, 32, 64, 128):
        H = (S + st - 1) // st
        bx, cl = rnd(B, H, H, 36), rnd(B, H, H, 720)
        lv.append(dict(box=bx, ldbox=36, cls=cl, ldcls=720, anchors_wh=[[32 * st / 8, 32 * st / 8]] * 9, H=H, W=H,
                       stride=st, n_off=n))
        n += 9 * H * H
    out['retina'] = (ops.DECODE_RETINA, lv, dict(box_astride=4, box_c0=0, cls_astride=80, cls_c0=0, conf_c0=0, A=9, C=80), n)
    # FCOS/ATSS head: box [B,H,W,4], cls [B,H,W,84] (80 classes + centerness at 80), 1 anchor
    lv, n = [], 0
    for st in (8, 16, 32, 64, 128):
        H = (S + st - 1) // st
        bx, cl = rnd(B, H, H, 4), rnd(B, H, H, 84)
        lv.append(dict(box=bx, ldbox=4, cls=cl, ldcls=84, anchors_wh=None, H=H, W=H, stride=st, n_off=n))
        n += H * H
    out['fcos'] = (ops.DECODE_FCOS, lv, dict(box_astride=4, box_c0=0, cls_astride=84, cls_c0=0, conf_c0=80, A=1, C=80), n)
    return out


class Timed:
    """One layout: a hipGraph of `reps` back-to-back launches (the host side of a launch -- ctypes marshalling of the level
    table -- costs more than the kernel, so the events must see device time only)."""
    reps = 20

    def __init__(self, name, mode, lv, kw, N, B, S):
        self.name, self.mode, self.lv, self.kw, self.N, self.B, self.S = name, mode, lv, kw, N, B, S
        bbox = torch.empty(B, N, 4, device='cuda')
        ci = torch.empty(B, N, dtype=torch.int64, device='cuda')
        sc = torch.empty(B, N, device='cuda')
        layout = (kw['box_astride'], kw['box_c0'], kw['cls_astride'], kw['cls_c0'], kw['conf_c0'], kw['A'], kw['C'])
        if mode == 'uv5':
            run = lambda: ops.decode_uv5_levels(lv, *layout, B, (S, S), bbox, ci, sc)
        else:
            run = lambda: ops.decode_levels(mode, lv, *layout, B, (S, S), bbox, ci, sc)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(3):
                run()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            for _ in range(self.reps):
                run()
        self.graph.replay()
        torch.cuda.synchronize()

    def ms(self, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = max(1, iters // self.reps)
        e0.record()
        for _ in range(n):
            self.graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (n * self.reps)

    def line(self, ms):
        kw = self.kw
        per_pix = kw['A'] * (kw['C'] + 4 + (0 if self.mode == ops.DECODE_RETINA else 1))
        nbytes = sum(4.0 * self.B * l['H'] * l['W'] * per_pix + 28.0 * self.B * kw['A'] * l['H'] * l['W'] for l in self.lv)
        gbs = nbytes / ms / 1e6
        return (f'{self.name:7s} B={self.B} S={self.S} N={self.N} {ms * 1e3:8.1f} us  {nbytes / 1e6:8.1f} MB  {gbs:7.0f} GB/s  '
                f'{gbs / 8000:.3f} of HBM peak')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--only', default='')
    ap.add_argument('--ab', default='', help='two layouts, e.g. uv5,yolo: interleaved runs, medians and their ratio')
    ap.add_argument('--runs', type=int, default=5)
    a = ap.parse_args()
    B, S = a.batch, a.size
    table = layouts(B, S)
    if a.ab:
        na, nb = a.ab.split(',')
        ta, tb = Timed(na, *table[na], B, S), Timed(nb, *table[nb], B, S)
        ra, rb = [], []
        for r in range(a.runs):
            ra.append(ta.ms(a.iters))
            rb.append(tb.ms(a.iters))
            print(f'run {r}: {na} {ra[-1] * 1e3:.1f} us  {nb} {rb[-1] * 1e3:.1f} us', flush=True)
        ma, mb = statistics.median(ra), statistics.median(rb)
        print(ta.line(ma))
        print(tb.line(mb))
        print(f'median of {a.runs} runs of {a.iters} launches: {na} / {nb} = {ma / mb:.3f}', flush=True)
        return
    for name, entry in table.items():
        if a.only and name != a.only:
            continue
        t = Timed(name, *entry, B, S)
        print(t.line(t.ms(a.iters)), flush=True)


if __name__ == '__main__':
    main()
