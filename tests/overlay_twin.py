"""numpy twin of the demo's detection overlay (mega/pytorch_amd/demo.py defines the picture; csrc/overlay.hip is the
kernel).  A painter: selection, stable sort, f32 rescale and truncation, label text by Python formatting, placement, then
every outline in draw order and every label in draw order, each painted over what is there."""
import numpy as np

COORD_MAX = 2 ** 30


def label_text(name, score):
    """"<name>: D.DD" -- Python's own formatting of the f32 score (scores above 9.99 print as 9.99)"""
    return "%s: %s" % (name, "%.2f" % min(float(np.float32(score)), 9.99))


def ratios(hw, resized_hw):
    """BoxList.resize: the ratio is an f64 quotient, the multiply an f32 op with the ratio rounded to f32 -> (sx, sy)"""
    return np.float32(hw[1] / resized_hw[1]), np.float32(hw[0] / resized_hw[0])


def rescale(box, sx, sy):
    """[n,4] f32 xyxy -> [n,4] i64: one f32 multiply, truncation toward zero, clamp to +-2^30 (NaN -> -2^30)"""
    box = np.asarray(box, np.float32).reshape(-1, 4)
    v = box * np.asarray([sx, sy, sx, sy], np.float32)
    assert v.dtype == np.float32
    with np.errstate(invalid="ignore"):
        t = np.clip(np.trunc(v.astype(np.float64)), -COORD_MAX, COORD_MAX)
    return np.where(np.isnan(t), -COORD_MAX, t).astype(np.int64)


def draw_list(box, score, label, count, hw, resized_hw, thr, num_classes):
    """the rows that are drawn, in draw order -> [(row, (x0, y0, x1, y1), class, f32 score)]"""
    H, W = hw
    n = int(min(max(count, 0), len(score)))
    score = np.asarray(score, np.float32)[:n]
    thr = np.float32(thr)
    ib = rescale(np.asarray(box)[:n], *ratios(hw, resized_hw))
    rows = [i for i in range(n) if score[i] > thr]
    rows.sort(key=lambda i: (-float(score[i]), i))
    out = []
    for i in rows:
        x0, y0, x1, y1 = (int(v) for v in ib[i])
        c = int(label[i])
        if x1 < x0 or y1 < y0 or x1 < 0 or y1 < 0 or x0 >= W or y0 >= H or not 0 <= c < num_classes:
            continue
        out.append((i, (x0, y0, x1, y1), c, score[i]))
    return out


def outline_rects(hw, b, thickness):
    """The pixels whose Chebyshev distance to the 1-pixel rectangle of b is <= h = (thickness - 1) / 2: the rectangle is
    four segments, and the square dilation of a segment is a filled rectangle -> those four, clipped to the image, as
    inclusive (xs0, ys0, xs1, ys1)."""
    H, W = hw
    x0, y0, x1, y1 = b
    h = (thickness - 1) // 2
    for ax0, ay0, ax1, ay1 in ((x0, y0, x0, y1), (x1, y0, x1, y1), (x0, y0, x1, y0), (x0, y1, x1, y1)):
        xs0, xs1 = max(ax0 - h, 0), min(ax1 + h, W - 1)
        ys0, ys1 = max(ay0 - h, 0), min(ay1 + h, H - 1)
        if xs1 >= xs0 and ys1 >= ys0:
            yield xs0, ys0, xs1, ys1


def outline_mask(hw, b, thickness):
    out = np.zeros(hw, bool)
    for xs0, ys0, xs1, ys1 in outline_rects(hw, b, thickness):
        out[ys0:ys1 + 1, xs0:xs1 + 1] = True
    return out


def draw(frame, box, score, label, count, resized_hw, thr, thickness, palette, atlas, names):
    """-> the annotated copy of frame [H,W,3] u8.  atlas: cells [G,gh,gw] u8, advances [G], chars (demo.LabelAtlas over
    numpy arrays); names[c] the class names; palette [NC,3] u8."""
    assert thickness >= 1 and thickness % 2 == 1
    out = np.array(frame, np.uint8, copy=True)
    H, W = out.shape[:2]
    palette = np.asarray(palette, np.uint8)
    dl = draw_list(box, score, label, count, (H, W), resized_hw, thr, len(palette))
    for _, b, c, _ in dl:
        for xs0, ys0, xs1, ys1 in outline_rects((H, W), b, thickness):
            out[ys0:ys1 + 1, xs0:xs1 + 1] = palette[c]
    cells, adv = np.asarray(atlas.cells), np.asarray(atlas.advances)
    gh, gw = cells.shape[1:]
    index = {ch: i for i, ch in enumerate(atlas.chars)}
    for _, (x0, y0, x1, y1), c, s in dl:
        text = label_text(names[c], s)
        tw = int(sum(adv[index[ch]] for ch in text))
        ly = y0 - gh
        if ly < 0:
            ly = max(y0, 0)
        lx = max(min(x0, W - tw), 0)
        a = np.zeros((gh, tw), np.int64)           # coverage of the whole rectangle
        col = 0
        for ch in text:
            g, w = index[ch], int(adv[index[ch]])
            shown = min(w, gw)
            a[:, col:col + shown] = cells[g][:, :shown]
            col += w
        colour = palette[c].astype(np.int64)
        patch = (colour[None, None, :] * (255 - a[:, :, None]) + 255 * a[:, :, None] + 127) // 255
        ys0, ys1, xs0, xs1 = max(ly, 0), min(ly + gh, H), max(lx, 0), min(lx + tw, W)
        if ys1 > ys0 and xs1 > xs0:
            out[ys0:ys1, xs0:xs1] = patch[ys0 - ly:ys1 - ly, xs0 - lx:xs1 - lx].astype(np.uint8)
    return out


def draw_batch(frames, boxes, scores, labels, counts, resized_hw, thr, thickness, palette, atlas, names):
    return np.stack([draw(frames[f], boxes[f], scores[f], labels[f], counts[f], resized_hw, thr, thickness, palette, atlas,
                          names) for f in range(len(frames))]) if len(frames) else np.array(frames, copy=True)


def as_op(names):
    """the twin behind the signature of ops.overlay_detections, over CPU torch tensors (VIDDemo(overlay=...))"""
    import torch

    def op(frames, boxes, scores, labels, counts, resized_hw, thr, thickness, palette, atlas, select_only=False):
        host = type("A", (), {"cells": atlas.cells.numpy(), "advances": atlas.advances.numpy(), "chars": atlas.chars})
        out = draw_batch(frames.numpy(), boxes.numpy(), scores.numpy(), labels.numpy(), counts.numpy(), resized_hw, thr,
                         thickness, palette.numpy(), host, names)
        frames.copy_(torch.from_numpy(out))
        return frames
    return op


def kernel_digits(score):
    """the kernel's arithmetic for D.DD: rint (round half to even) of the exact f64 product f32 score * 100"""
    iv = int(min(np.rint(np.float64(np.float32(score)) * np.float64(100.0)), 999.0))
    return "%d.%d%d" % (iv // 100, iv // 10 % 10, iv % 10)


def random_detections(seed, F, R, resized_hw, num_classes=31, grid=64):
    """Seeded [F,R,...] detections in the resized frame: boxes crossing each of the four edges, boxes wholly outside,
    degenerate boxes, scores on a coarse grid (ties; 0.7 and 1.0 as f32 among them), a few classes outside the palette,
    counts from 0 to R."""
    rng = np.random.default_rng(seed)
    rh, rw = resized_hw
    ctr = rng.uniform([-0.1 * rw, -0.1 * rh], [1.1 * rw, 1.1 * rh], (F, R, 2))
    wh = rng.uniform(2, [0.5 * rw + 3, 0.5 * rh + 3], (F, R, 2))
    box = np.concatenate([ctr - wh / 2, ctr + wh / 2], 2)
    kind = rng.integers(0, 40, (F, R))
    box[kind == 0] = box[kind == 0][:, [2, 1, 0, 3]]                   # x1 < x0
    box[kind == 1] += np.asarray([2.0 * rw, 0, 2.0 * rw, 0])           # wholly outside
    box[kind == 2] = box[kind == 2] * 0 + np.asarray([-30.0, -20.0, rw + 30.0, rh + 20.0])      # crosses all four edges
    score = (rng.integers(0, grid + 1, (F, R)) / float(grid)).astype(np.float32)
    score[kind == 3] = np.float32(0.7)
    score[kind == 4] = np.float32(1.0)
    label = rng.integers(1, num_classes, (F, R)).astype(np.int64)
    label[kind == 5] = num_classes
    label[kind == 6] = -1
    counts = rng.integers(0, R + 1, F).astype(np.int32)
    if F > 1:
        counts[0] = R
    return box.astype(np.float32), score, label, counts
