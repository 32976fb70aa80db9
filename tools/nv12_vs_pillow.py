"""What "full range" means here, for the reader of profiles/nv12.md (CPU only, nothing is asserted): the library's full-range
BT.601 row (cy, crv, cgu, cgv, cbu = 256, 359, 88, 183, 454, >> 8) against Pillow's own 'YCbCr' -> 'RGB' conversion (the JPEG
matrix) over every (Y, U, V) triple.  Prints the largest absolute difference per channel and how many triples differ.

    python tools/nv12_vs_pillow.py
"""
import json

import numpy as np
import PIL
import PIL.Image


def main():
    u, v = np.meshgrid(np.arange(256, dtype=np.int32), np.arange(256, dtype=np.int32), indexing='ij')
    d, e = u - 128, v - 128
    worst, differ = np.zeros(3, np.int64), np.zeros(3, np.int64)
    for y in range(256):
        c = 256 * y + 128
        ours = np.stack([np.clip((c + 359 * e) >> 8, 0, 255), np.clip((c - 88 * d - 183 * e) >> 8, 0, 255),
                         np.clip((c + 454 * d) >> 8, 0, 255)], axis=-1)
        ycc = np.stack([np.full_like(u, y), u, v], axis=-1).astype(np.uint8)
        pil = np.asarray(PIL.Image.fromarray(ycc, 'YCbCr').convert('RGB')).astype(np.int32)
        diff = np.abs(ours - pil).reshape(-1, 3)
        worst = np.maximum(worst, diff.max(axis=0))
        differ += (diff != 0).sum(axis=0)
    print(json.dumps({'pillow': PIL.__version__, 'triples': 256 ** 3, 'max_abs_diff_rgb': worst.tolist(),
                      'triples_that_differ_rgb': differ.tolist()}))


if __name__ == '__main__':
    main()
