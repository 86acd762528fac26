"""A numpy restatement of the test-time box augmentation of mega_core/engine/bbox_aug.py + box_head/inference.py, in f32
as the reference's torch ops round it:
  candidates()     prepare_boxlist + clip_to_image(remove_empty=False) + the score threshold, class-major, no background
  transpose()      BoxList.transpose(FLIP_LEFT_RIGHT): x' = (W - x_max) - 1, x'_max = (W - x_min) - 1
  resize()         BoxList.resize: f32 box times the f32 of float(s) / float(s_orig), per axis
  filter_results() score > thresh, per-class greedy NMS (nms.cu IoU, +1 areas), keep ascending, k-th value cut
  merge()          the views of one frame -> its detections (boxes, scores, labels) in view 0's image
Ties are ordered by (score desc, index asc), the rule of the package's NMS."""
import numpy as np

f32 = np.float32


def candidates(logits, deltas, props, im_w, im_h, weights=(10.0, 10.0, 5.0, 5.0), score_thresh=0.001, nprop=None):
    """logits [R,NC], deltas [R,NC*4], props [R,4] -> (boxes [NC-1,R,4], scores [NC-1,R]; -1 = not > thresh)."""
    logits, deltas, props = (np.asarray(a, f32) for a in (logits, deltas, props))
    R, NC = logits.shape
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    prob = (e / e.sum(axis=1, keepdims=True, dtype=f32)).astype(f32)
    wx, wy, ww, wh = (f32(w) for w in weights)
    clip = f32(np.log(f32(1000.0 / 16)))
    widths = props[:, 2] - props[:, 0] + f32(1)
    heights = props[:, 3] - props[:, 1] + f32(1)
    cx = props[:, 0] + f32(0.5) * widths
    cy = props[:, 1] + f32(0.5) * heights
    d = deltas.reshape(R, NC, 4)
    dx, dy = d[..., 0] / wx, d[..., 1] / wy
    dw, dh = np.minimum(d[..., 2] / ww, clip), np.minimum(d[..., 3] / wh, clip)
    pcx, pcy = dx * widths[:, None] + cx[:, None], dy * heights[:, None] + cy[:, None]
    pw, ph = np.exp(dw) * widths[:, None], np.exp(dh) * heights[:, None]
    b = np.stack([pcx - f32(0.5) * pw, pcy - f32(0.5) * ph, pcx + f32(0.5) * pw - f32(1), pcy + f32(0.5) * ph - f32(1)], -1)
    b[..., 0::2] = np.clip(b[..., 0::2], f32(0), f32(im_w - 1))
    b[..., 1::2] = np.clip(b[..., 1::2], f32(0), f32(im_h - 1))
    s = np.where(prob > f32(score_thresh), prob, f32(-1)).astype(f32)
    if nprop is not None:
        s[int(nprop):] = -1
    return np.ascontiguousarray(b[:, 1:].transpose(1, 0, 2)).astype(f32), np.ascontiguousarray(s[:, 1:].T)


def transpose(boxes, w):
    b = np.array(boxes, f32, copy=True)
    b[:, 0] = (f32(w) - boxes[:, 2]) - f32(1)
    b[:, 2] = (f32(w) - boxes[:, 0]) - f32(1)
    return b


def resize(boxes, size, size_orig):
    rw = f32(float(size[0]) / float(size_orig[0]))
    rh = f32(float(size[1]) / float(size_orig[1]))
    b = np.array(boxes, f32, copy=True)
    b[:, 0::2] = b[:, 0::2] * rw
    b[:, 1::2] = b[:, 1::2] * rh
    return b


def _suppresses(a, b, thr, strict_gt):
    """box a [4] against boxes b [n,4]: nms.cu devIoU term by term in f32 (elementwise numpy f32 ops round as scalar ones)"""
    one, zero = f32(1), f32(0)
    left, right = np.maximum(a[0], b[:, 0]), np.minimum(a[2], b[:, 2])
    top, bottom = np.maximum(a[1], b[:, 1]), np.minimum(a[3], b[:, 3])
    width = np.maximum(right - left + one, zero)
    height = np.maximum(bottom - top + one, zero)
    inter = width * height
    sa = (a[2] - a[0] + one) * (a[3] - a[1] + one)
    sb = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    iou = inter / (sa + sb - inter)
    return iou > f32(thr) if strict_gt else iou >= f32(thr)


def nms(boxes, scores, thr, strict_gt=True):
    """greedy NMS; kept indices ascending"""
    n = len(scores)
    order = np.lexsort((np.arange(n), -np.asarray(scores, np.float64)))
    sb = np.asarray(boxes, f32)[order]
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(order[i])
        if i + 1 < n:
            removed[i + 1:] |= _suppresses(sb[i], sb[i + 1:], thr, strict_gt)
    return np.sort(np.asarray(keep, np.int64))


def filter_results(boxes, scores, score_thresh=0.001, nms_thresh=0.5, max_det=300, strict_gt=True):
    """boxes [C1,N,4], scores [C1,N] (class j + 1) -> (boxes [D,4], scores [D], labels [D])"""
    ob, os_, ol = [], [], []
    for c in range(scores.shape[0]):
        inds = np.nonzero(scores[c] > f32(score_thresh))[0]
        b, s = boxes[c][inds], scores[c][inds]
        k = nms(b, s, nms_thresh, strict_gt)
        ob.append(b[k]); os_.append(s[k]); ol.append(np.full(len(k), c + 1, np.int64))
    ob = np.concatenate(ob).reshape(-1, 4).astype(f32)
    os_ = np.concatenate(os_).astype(f32)
    ol = np.concatenate(ol)
    n = len(os_)
    if n > max_det > 0:
        t = np.sort(os_)[n - max_det]            # torch.kthvalue(scores, n - max_det + 1)
        m = os_ >= t
        ob, os_, ol = ob[m], os_[m], ol[m]
    return ob, os_, ol


def merge(views, sizes, flips, **kw):
    """views[k] = (boxes [C1,R_k,4], scores [C1,R_k]) of one frame in view k's image of sizes[k] = (w, h); flips[k]."""
    bs, ss = [], []
    for k, (b, s) in enumerate(views):
        C1, R = s.shape
        b = np.asarray(b, f32).reshape(-1, 4)
        if flips[k]:
            b = transpose(b, sizes[k][0])
        if k > 0:
            b = resize(b, sizes[0], sizes[k])
        bs.append(b.reshape(C1, R, 4))
        ss.append(np.asarray(s, f32))
    return filter_results(np.concatenate(bs, axis=1), np.concatenate(ss, axis=1), **kw)


def random_views(seed, K, R, C1=30, sizes=None, p_live=0.3, grid=None, empty=False):
    """Seeded candidates of one frame for K views: boxes inside each view's image, scores on a coarse grid when `grid`
    (exact ties), -1 for rows below the threshold.  A few objects repeat across views and rows so NMS has work."""
    rng = np.random.RandomState(seed)
    sizes = sizes or [(160 + 16 * k, 96 + 8 * k) for k in range(K)]
    out = []
    for k in range(K):
        w, h = sizes[k]
        ctr = rng.rand(C1, R, 2) * [w, h]
        ctr[:, ::3] = rng.rand(C1, 1, 2) * [w, h] + rng.randn(C1, (R + 2) // 3, 2) * 3   # clustered rows
        half = rng.rand(C1, R, 2) * [w / 4, h / 4] + 2
        b = np.concatenate([ctr - half, ctr + half], -1)
        b[..., 0::2] = np.clip(b[..., 0::2], 0, w - 1)
        b[..., 1::2] = np.clip(b[..., 1::2], 0, h - 1)
        s = rng.rand(C1, R)
        if grid:
            s = np.round(s * grid) / grid
        s = np.where((rng.rand(C1, R) < p_live) & (s > 0.001) & (not empty), s, -1)
        out.append((b.astype(f32), s.astype(f32)))
    return out, sizes
