"""Numpy restatement of the overlay renderer's raster rules (include/mydet.h: mydet_draw_boxes_*), written from
the rules and not from the kernel: float64 geometry, integer blending.  Colours and label texts come from the documented host
functions (ops.draw_palette, ops.rgb_to_yuv, ops.draw_label_text), which tests/test_draw_host.py checks on their own."""
import math

import numpy as np

from mydetection_amd import ops

EPS = 1e-3          # a pixel whose (a, b) lies within EPS of a threshold that decides it is "unsettled" for float32


def _ab(H, W, row):
    cx, cy, w, h, ang = (float(v) for v in row)
    c, s = (1.0, 0.0) if ang == 0 else (math.cos(math.radians(ang)), math.sin(math.radians(ang)))
    dx = (np.arange(W, dtype=np.float64) + 0.5 - cx)[None, :]
    dy = (np.arange(H, dtype=np.float64) + 0.5 - cy)[:, None]
    return np.abs(dx * c + dy * s), np.abs(-dx * s + dy * c)


def _fill(a, b, w, h):
    return (a <= w / 2) & (b <= h / 2)


def _outline(a, b, w, h, t):
    return (a <= w / 2 + t / 2) & (b <= h / 2 + t / 2) & ~((a < w / 2 - t / 2) & (b < h / 2 - t / 2))


def valid_row(row):
    return bool(np.all(np.isfinite(np.asarray(row, dtype=np.float64))) and row[2] > 0 and row[3] > 0)


def box_masks(H, W, row, t, alpha):
    """(fill mask, outline mask, unsettled mask) of one valid row (cx, cy, w, h, angle)."""
    a, b = _ab(H, W, row)
    w, h = float(row[2]), float(row[3])
    fill, outline = _fill(a, b, w, h), _outline(a, b, w, h, t)
    unsettled = np.zeros((H, W), dtype=bool)
    if float(row[4]) == 0:                                         # c = 1, s = 0 and box values at multiples of 1/8: float32 is exact
        return fill, outline, unsettled
    for da in (-EPS, EPS):
        for db in (-EPS, EPS):
            unsettled |= _outline(a + da, b + db, w, h, t) != outline
            if alpha:
                unsettled |= _fill(a + da, b + db, w, h) != fill
    return fill, outline, unsettled


def label_bitmap(text, atlas):
    """(rows x n*cw) 0 / 1 bitmap of a label text from the atlas [96, ch, cw]; a byte outside 32..127 shows '?'."""
    codes = [ord(c) if 32 <= ord(c) <= 127 else ord('?') for c in text[:33]]
    return np.concatenate([atlas[c - 32] for c in codes], axis=1)


def label_rect(H, W, row, t, n, ch, cw):
    cx, cy, w, h = (float(v) for v in row[:4])
    left = min(max(math.floor(cx - w / 2 - t / 2), 0), max(0, W - n * cw))
    top = min(max(math.floor(cy - h / 2 - t / 2) - ch, 0), max(0, H - ch))
    return int(left), int(top)


def label_masks(H, W, row, t, text, atlas):
    """(label mask, text mask) [H, W] of a row's label, clipped to the frame."""
    lab, txt = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
    if not text:
        return lab, txt
    bm = label_bitmap(text, atlas) != 0
    ch, lw = bm.shape
    left, top = label_rect(H, W, row, t, lw // atlas.shape[2], ch, atlas.shape[2])
    hh, ww = min(ch, H - top), min(lw, W - left)
    lab[top:top + hh, left:left + ww] = True
    txt[top:top + hh, left:left + ww] = bm[:hh, :ww]
    return lab, txt


def text_color(rgb):
    r, g, b = (int(v) for v in rgb)
    return (255, 255, 255) if 299 * r + 587 * g + 114 * b < 150000 else (0, 0, 0)


def blend(old, col, alpha):
    return ((int(col) * alpha + old.astype(np.int64) * (255 - alpha) + 127) // 255).astype(np.uint8)


def row_colors(style, classes, ids, K):
    """uint8 [K, 3]: the colour of each row under an ops.DrawStyle."""
    if style.color_mode == ops.DRAW_COLOR_MODES['fixed']:
        return np.tile(np.asarray(style.color, dtype=np.uint8), (K, 1))
    keys = classes if style.color_mode == ops.DRAW_COLOR_MODES['class'] else ids
    pal = ops.draw_palette(style.n_palette)
    if keys is None:
        return np.tile(pal[0], (K, 1))
    return pal[np.asarray(keys, dtype=np.int64) % style.n_palette]


def row_texts(style, scores, classes, ids, K):
    return [ops.draw_label_text(None if classes is None else classes[k], None if scores is None else scores[k],
                                None if ids is None else ids[k], style.names, style.label_flags) if style.label_flags else ''
            for k in range(K)]


def _rows(boxes):
    boxes = np.asarray(boxes, dtype=np.float64)
    if boxes.shape[1] == 4:
        boxes = np.concatenate([boxes, np.zeros((boxes.shape[0], 1))], axis=1)
    return boxes


def draw_rgb(img, boxes, count, style, scores=None, classes=None, ids=None):
    """Paint one frame [H, W, 3] uint8 in place; returns the unsettled-pixel mask [H, W]."""
    H, W, _ = img.shape
    boxes = _rows(boxes)
    K = boxes.shape[0]
    unsettled = np.zeros((H, W), dtype=bool)
    count = K if count is None else min(int(count), K)
    if count <= 0:
        return unsettled
    colors, texts = row_colors(style, classes, ids, K), row_texts(style, scores, classes, ids, K)
    atlas = ops.glyph_atlas(style.label_height).numpy() if style.label_flags else None
    t, alpha = style.thickness, style.fill_alpha
    for k in range(count - 1, -1, -1):
        row = boxes[k]
        if not valid_row(row):
            continue
        fill, outline, uns = box_masks(H, W, row, t, alpha)
        unsettled |= uns
        col = colors[k]
        if alpha:
            for c in range(3):
                img[..., c][fill] = blend(img[..., c][fill], col[c], alpha)
        img[outline] = col
        lab, txt = label_masks(H, W, row, t, texts[k], atlas)
        img[lab] = col
        img[txt] = text_color(col)
    return unsettled


def draw_yuv(Y, U, V, boxes, count, style, matrix='bt601', full_range=False, scores=None, classes=None, ids=None):
    """Paint one 4:2:0 frame in place: Y [H, W], U and V [ceil(H/2), ceil(W/2)] uint8; returns the unsettled luma mask."""
    H, W = Y.shape
    H2, W2 = U.shape
    boxes = _rows(boxes)
    K = boxes.shape[0]
    unsettled = np.zeros((H, W), dtype=bool)
    count = K if count is None else min(int(count), K)
    if count <= 0:
        return unsettled
    colors, texts = row_colors(style, classes, ids, K), row_texts(style, scores, classes, ids, K)
    atlas = ops.glyph_atlas(style.label_height).numpy() if style.label_flags else None
    t, alpha = style.thickness, style.fill_alpha

    def quads(mask):                                               # [H2, 2, W2, 2] with the frame's odd edge padded by False
        m = np.zeros((2 * H2, 2 * W2), dtype=bool)
        m[:H, :W] = mask
        return m.reshape(H2, 2, W2, 2)

    for k in range(count - 1, -1, -1):
        row = boxes[k]
        if not valid_row(row):
            continue
        fill, outline, uns = box_masks(H, W, row, t, alpha)
        unsettled |= uns
        cy, cu, cv = (int(v) for v in ops.rgb_to_yuv(colors[k], matrix, full_range))
        ty, tu, tv = (int(v) for v in ops.rgb_to_yuv(np.asarray(text_color(colors[k]), dtype=np.uint8), matrix, full_range))
        if alpha:
            Y[fill] = blend(Y[fill], cy, alpha)
            q = quads(fill).any(axis=(1, 3))
            U[q], V[q] = blend(U[q], cu, alpha), blend(V[q], cv, alpha)
        Y[outline] = cy
        q = quads(outline).any(axis=(1, 3))
        U[q], V[q] = cu, cv
        lab, txt = label_masks(H, W, row, t, texts[k], atlas)
        Y[lab] = cy
        Y[txt] = ty
        ql, qt = quads(lab), quads(txt)
        done = np.zeros((H2, W2), dtype=bool)
        for r in range(2):                                         # the colour at the first pixel of the quad the label hits
            for c in range(2):
                first = ql[:, r, :, c] & ~done
                is_text = first & qt[:, r, :, c]
                U[first], V[first] = cu, cv
                U[is_text], V[is_text] = tu, tv
                done |= first
    return unsettled
