"""A numpy restatement of mega/pytorch_amd/soft_nms.py (soft-NMS + box voting as the final filter of the candidate
merge): f32 as defined there, f64 where stated.  Built on tests/bbox_aug_twin.py for the candidates, the flip, the resize,
the IoU and the greedy NMS.
  iou()            box a against boxes b: nms.cu devIoU term by term in f32
  soft_nms()       step 1 on one (frame, class): kept rows in selection order with their final scores
  vote()           step 2 for the kept rows of one (frame, class)
  merge()          the views of one frame -> (boxes, scores, labels) in view 0's image
  clustered_views()/ tie_views()   the seeded fixtures of the tests
`stats` (a dict) collects what the fixture preconditions need: "gap" = the smallest relative gap between the winner and
the runner-up over all selection steps, "thresh" = the smallest relative distance of a decayed score to SCORE_THRESH,
"steps" = the longest selection chain."""
import numpy as np

import bbox_aug_twin as bt

f32 = np.float32


def iou(a, b):
    one, zero = f32(1), f32(0)
    a, b = np.asarray(a, f32), np.asarray(b, f32).reshape(-1, 4)
    left, right = np.maximum(a[0], b[:, 0]), np.minimum(a[2], b[:, 2])
    top, bottom = np.maximum(a[1], b[:, 1]), np.minimum(a[3], b[:, 3])
    width = np.maximum(right - left + one, zero)
    height = np.maximum(bottom - top + one, zero)
    inter = width * height
    sa = (a[2] - a[0] + one) * (a[3] - a[1] + one)
    sb = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (inter / (sa + sb - inter)).astype(f32)


def _note(stats, key, value, smallest=True):
    if stats is not None:
        old = stats.get(key)
        stats[key] = value if old is None else (min(old, value) if smallest else max(old, value))


def soft_nms(boxes, scores, method, nms_thresh=0.5, strict_gt=True, sigma=0.5, score_thresh=0.001, stats=None):
    """boxes [N,4], scores [N] (every row of the class, -1 = dead) -> (kept rows in selection order, their scores)"""
    boxes = np.asarray(boxes, f32)
    s = np.array(scores, f32, copy=True)
    thr, sth = f32(nms_thresh), f32(score_thresh)
    alive = s > sth
    kept, ks = [], []
    for _ in range(len(s)):                      # every pass removes at least m
        idx = np.nonzero(alive)[0]
        if len(idx) == 0:
            break
        m = idx[np.argmax(s[idx])]               # the first of equal maxima: the smallest row
        if len(idx) > 1:
            second = np.sort(s[idx])[-2]
            _note(stats, "gap", float((np.float64(s[m]) - np.float64(second)) / np.float64(s[m])))
        kept.append(int(m))
        ks.append(s[m])
        alive[m] = False
        j = np.nonzero(alive)[0]
        if len(j) == 0:
            break
        o = iou(boxes[m], boxes[j])
        if method == "gaussian":
            with np.errstate(invalid="ignore"):
                w = np.exp(-(o * o) / f32(sigma)).astype(f32)
        elif method == "linear":
            with np.errstate(invalid="ignore"):
                hit = (o > thr) if strict_gt else (o >= thr)
            w = np.where(hit, f32(1) - o, f32(1)).astype(f32)
        else:
            raise ValueError(method)
        w = np.where(np.isnan(o), f32(1), w).astype(f32)
        s[j] = s[j] * w
        _note(stats, "thresh", float(np.min(np.abs(s[j].astype(np.float64) - np.float64(sth))) / np.float64(sth)))
        alive[j] = s[j] > sth
    _note(stats, "steps", len(kept), smallest=False)
    return np.asarray(kept, np.int64), np.asarray(ks, f32)


def vote(boxes, scores, kept, vote_thresh=0.8, scoring="ID", score_thresh=0.001, kept_scores=None):
    """boxes [N,4] / scores [N]: the class's ORIGINAL rows; kept [M] rows -> (voted boxes [M,4] f32, scores [M] f32)"""
    boxes, scores = np.asarray(boxes, f32), np.asarray(scores, f32)
    live = np.nonzero(scores > f32(score_thresh))[0]
    ob = np.zeros((len(kept), 4), f32)
    os_ = np.array(scores[kept] if kept_scores is None else kept_scores, f32, copy=True)
    for n, k in enumerate(kept):
        with np.errstate(invalid="ignore"):
            v = iou(boxes[k], boxes[live]) >= f32(vote_thresh)
        v |= live == k
        sj = scores[live][v].astype(np.float64)
        bj = boxes[live][v].astype(np.float64)
        ob[n] = ((sj[:, None] * bj).sum(0) / sj.sum()).astype(f32)
        if scoring == "AVG":
            os_[n] = f32(sj.sum() / len(sj))
        elif scoring != "ID":
            raise ValueError(scoring)
    return ob, os_


def map_views(views, sizes, flips):
    """views[k] = (boxes [C1,R_k,4], scores [C1,R_k]) -> (boxes [C1,sum R_k,4] in view 0's image, scores), (view, row) order"""
    bs, ss = [], []
    for k, (b, s) in enumerate(views):
        C1, R = np.asarray(s).shape
        b = np.asarray(b, f32).reshape(-1, 4)
        if flips[k]:
            b = bt.transpose(b, sizes[k][0])
        if k > 0:
            b = bt.resize(b, sizes[0], sizes[k])
        bs.append(b.reshape(C1, R, 4))
        ss.append(np.asarray(s, f32))
    return np.concatenate(bs, axis=1), np.concatenate(ss, axis=1)


def merge(views, sizes, flips, score_thresh=0.001, nms_thresh=0.5, max_det=300, strict_gt=True, soft_method=None,
          sigma=0.5, vote_on=False, vote_thresh=0.8, vote_scoring="ID", stats=None):
    """One frame -> (boxes [D,4], scores [D], labels [D]) as ops.soft_merge returns its first counts[f] rows."""
    boxes, scores = map_views(views, sizes, flips)
    ob, os_, ol = [], [], []
    for c in range(scores.shape[0]):
        b, s = boxes[c], scores[c]
        if soft_method is None:
            live = np.nonzero(s > f32(score_thresh))[0]
            kept = live[bt.nms(b[live], s[live], nms_thresh, strict_gt)]
            ks = s[kept]
        else:
            kept, ks = soft_nms(b, s, soft_method, nms_thresh, strict_gt, sigma, score_thresh, stats)
            o = np.argsort(kept, kind="stable")
            kept, ks = kept[o], ks[o]
        if vote_on:
            kb, ks = vote(b, s, kept, vote_thresh, vote_scoring, score_thresh, kept_scores=ks)
        else:
            kb = b[kept]
        ob.append(kb.reshape(-1, 4)); os_.append(ks); ol.append(np.full(len(kept), c + 1, np.int64))
    ob = np.concatenate(ob).reshape(-1, 4).astype(f32)
    os_ = np.concatenate(os_).astype(f32)
    ol = np.concatenate(ol)
    n = len(os_)
    if n > max_det > 0:
        t = np.sort(os_)[n - max_det]
        m = os_ >= t
        ob, os_, ol = ob[m], os_[m], ol[m]
    return ob, os_, ol


def _to_view(b0, k, sizes, flips):
    """view-0 boxes -> view k's own image (the inverse of the merge's mapping, up to rounding), clipped to the view"""
    w0, h0 = sizes[0]
    w, h = sizes[k]
    b = np.array(b0, np.float64, copy=True)
    if k > 0:
        b[..., 0::2] *= w / w0
        b[..., 1::2] *= h / h0
    if flips[k]:
        x1 = w - b[..., 2] - 1
        x2 = w - b[..., 0] - 1
        b[..., 0], b[..., 2] = x1, x2
    b[..., 0::2] = np.clip(b[..., 0::2], 0, w - 1)
    b[..., 1::2] = np.clip(b[..., 1::2], 0, h - 1)
    return b


def clustered_class(seed, K, R, sizes, flips, p_live=0.37, centres=6, max_live=111):
    """One class of clustered_views from its own seed -> [(boxes [R,4], scores [R])] x K"""
    rng = np.random.RandomState(seed)
    w0, h0 = sizes[0]
    ctr = rng.rand(centres, 2) * [w0 * 0.7, h0 * 0.7] + [w0 * 0.15, h0 * 0.15]
    half = rng.rand(centres, 2) * [w0 * 0.10, h0 * 0.10] + [w0 * 0.04, h0 * 0.04]
    out = []
    budget = max_live if max_live else K * R
    for k in range(K):
        which = rng.randint(0, centres, R)
        c = ctr[which] + rng.randn(R, 2) * half[which] * 0.18
        hf = half[which] * (1 + rng.randn(R, 2) * 0.10)
        b0 = np.concatenate([c - hf, c + hf], -1)
        b0[..., 0::2] = np.clip(b0[..., 0::2], 0, w0 - 1)
        b0[..., 1::2] = np.clip(b0[..., 1::2], 0, h0 - 1)
        s = rng.rand(R) * 0.98 + 0.01
        s = np.where(rng.rand(R) < p_live, s, -1)
        live = np.nonzero(s >= 0)[0]
        s[live[budget:]] = -1
        budget -= min(budget, len(live))
        out.append((_to_view(b0, k, sizes, flips).astype(f32), s.astype(f32)))
    return out


VIEW_SIZES = [(1000, 600), (1000, 600), (1203, 717)]      # identity, its flip, a rescaled view (unequal w / h ratios)
VIEW_FLIPS = [False, True, False]


def clustered_views(seeds, K, R, sizes=None, flips=None, p_live=0.37, centres=6, empty_classes=(), max_live=111):
    """Seeded candidates of one frame, one seed per class: every class has `centres` objects in view 0's image; a row is
    one of them, jittered (so IoUs fall on both sides of 0.5 and 0.8), seen in its view's own image; dead rows (-1) are
    interleaved with live ones, at most max_live live rows per class over all views (the surplus of the later views is
    dead too); scores are continuous (no exact ties).  -> (views, sizes, flips)"""
    sizes = sizes or VIEW_SIZES[:K]
    flips = flips or VIEW_FLIPS[:K]
    per_class = [clustered_class(sd, K, R, sizes, flips, p_live, centres, max_live) for sd in seeds]
    out = []
    for k in range(K):
        b = np.stack([pc[k][0] for pc in per_class])
        s = np.stack([pc[k][1] for pc in per_class])
        for c_ in empty_classes:
            s[c_] = -1
        out.append((b, s))
    return out, sizes, flips


def tie_views(seed, K, R, C1=3, sizes=None, flips=None, p_live=0.6):
    """Integer boxes from a few templates at integer offsets and scores from a small set: exact score ties, identical
    boxes (IoU 1) and pairs whose IoU is exactly 0.5 (10x10 inside 10x20: 100 / 200) in every view."""
    rng = np.random.RandomState(seed)
    sizes = sizes or [(320, 200), (320, 200), (160, 100)][:K]
    flips = flips or [False, True, False][:K]
    tmpl = np.asarray([[0, 0, 9, 9], [0, 0, 9, 19], [0, 0, 19, 9], [5, 0, 14, 9], [0, 5, 9, 14], [2, 2, 11, 11]], np.float64)
    out = []
    for k in range(K):
        w, h = sizes[k]
        off = np.stack([rng.randint(0, 3, (C1, R)) * 40 + 10, rng.randint(0, 2, (C1, R)) * 40 + 10], -1)
        b = tmpl[rng.randint(0, len(tmpl), (C1, R))] + np.concatenate([off, off], -1)
        s = rng.randint(1, 8, (C1, R)) / 8.0
        s = np.where(rng.rand(C1, R) < p_live, s, -1)
        assert b[..., 2].max() <= w - 1 and b[..., 3].max() <= h - 1
        out.append((b.astype(f32), s.astype(f32)))
    return out, sizes, flips


# The GPU fixtures: F = 2 frames x NC - 1 = 3 classes, one seed per (frame, class), chosen so that under gaussian
# soft-NMS (SIGMA 0.5) the twin's "gap" and "thresh" are >= 1e-3 (tests/test_soft_nms.py asserts it on the CPU).
FIXTURE_P_LIVE = {(1, 1): 1.0, (1, 37): 0.6, (1, 300): 0.37, (3, 1): 1.0, (3, 37): 0.6, (3, 300): 0.11}
FIXTURE_SEEDS = {(1, 1): (1008, 1009, 1010, 1011, 1012, 1013), (1, 37): (1260, 1261, 1262, 1263, 1265, 1266),
                 (1, 300): (3104, 3118, 3122, 3134, 3140, 3146), (3, 1): (3008, 3009, 3010, 3011, 3012, 3013),
                 (3, 37): (3263, 3269, 3270, 3271, 3274, 3282), (3, 300): (5104, 5114, 5118, 5124, 5127, 5133)}
FIXTURE_SIGMA = 0.5


def fixture(K, R):
    """-> (frames, sizes, flips): frames[f] = the K views of frame f, as merge() takes them"""
    seeds = FIXTURE_SEEDS[(K, R)]
    frames = []
    for f in range(2):
        v, sizes, flips = clustered_views(seeds[3 * f:3 * f + 3], K, R, p_live=FIXTURE_P_LIVE[(K, R)])
        frames.append(v)
    return frames, sizes, flips
