"""Test helper: a numpy twin of Seq-NMS as mega/pytorch_amd/seq_nms.py defines it, written literally: a full DP
recompute every iteration, the f32 IoU in the stated order (vid_twin.iou_f32: boxlist_iou's +1 convention), f64 sums,
vectorised per frame step.

Frames are dicts {"box": [n,4] f32, "score": [n] f32, "label": [n] int} (the shape vid_twin uses, "size" optional);
videos are (start, length) pairs.
"""
import numpy as np

import vid_twin


def _task(boxes, scores, link, nms, rescore):
    """One (video, class) task: boxes / scores per frame (lists) -> (keep list of bool arrays, new score list)."""
    L = len(boxes)
    alive = [np.ones(len(s), bool) for s in scores]
    keep = [np.zeros(len(s), bool) for s in scores]
    new = [np.zeros(len(s), np.float32) for s in scores]
    s64 = [np.asarray(s, np.float32).astype(np.float64) for s in scores]
    ious = [None] + [vid_twin.iou_f32(boxes[t - 1], boxes[t]) if len(boxes[t - 1]) and len(boxes[t]) else None
                     for t in range(1, L)]                    # [n_{t-1}, n_t]: iou(j, i)
    iters = 0
    while any(a.any() for a in alive):
        iters += 1
        # 1. forward DP (full recompute)
        S, P = [], []
        for t in range(L):
            if t == 0 or ious[t] is None or not alive[t - 1].any():
                S.append(s64[t].copy())
                P.append(np.full(len(s64[t]), -1, np.int64))
                continue
            with np.errstate(invalid="ignore"):
                link_m = (ious[t] > link) & alive[t - 1][:, None]
            cand = np.where(link_m, S[t - 1][:, None], -np.inf)
            has = link_m.any(0)
            best = cand.max(0)
            arg = cand.argmax(0)                 # the first (smallest) j on equal S
            S.append(np.where(has, s64[t] + best, s64[t]))
            P.append(np.where(has, arg, -1))
        # 2. the best end box: largest S, then the earliest frame, then the smallest position
        bs, bt, bi = -np.inf, -1, -1
        for t in range(L):
            if not alive[t].any():
                continue
            m = np.where(alive[t], S[t], -np.inf)
            i = int(m.argmax())
            if m[i] > bs:
                bs, bt, bi = m[i], t, i
        path = []
        t, i = bt, bi
        while True:
            path.append((t, i))
            j = int(P[t][i])
            if j < 0:
                break
            t, i = t - 1, j
        # 3. rescore
        if rescore == "avg":
            val = np.float32(bs / len(path))
        else:
            val = np.float32(max(np.float32(scores[t][i]) for t, i in path))
        # 4. suppress
        for t, i in path:
            with np.errstate(invalid="ignore"):
                sup = vid_twin.iou_f32(boxes[t], boxes[t][i:i + 1])[:, 0] > nms
            alive[t] &= ~sup
            alive[t][i] = False
            keep[t][i] = True
            new[t][i] = val
    return keep, new, iters


def seq_nms(frames, videos, link_iou=0.5, nms_iou=0.3, rescore="avg"):
    """-> (keep per frame [n] bool, new score per frame [n] f32 (0 where not kept), iterations per (video, class))."""
    link, nms = np.float32(link_iou), np.float32(nms_iou)
    keep = [np.zeros(len(f["score"]), bool) for f in frames]
    new = [np.zeros(len(f["score"]), np.float32) for f in frames]
    iters = {}
    for vi, (s0, n) in enumerate(videos):
        labels = set()
        for f in frames[s0:s0 + n]:
            labels.update(np.asarray(f["label"]).astype(int).tolist())
        for c in sorted(labels):
            sel = [np.nonzero(np.asarray(f["label"]).astype(int) == c)[0] for f in frames[s0:s0 + n]]
            boxes = [np.asarray(f["box"], np.float32).reshape(-1, 4)[s] for f, s in zip(frames[s0:s0 + n], sel)]
            scores = [np.asarray(f["score"], np.float32)[s] + np.float32(0) for f, s in zip(frames[s0:s0 + n], sel)]
            k, v, it = _task(boxes, scores, link, nms, rescore)
            iters[(vi, c)] = it
            for t, s in enumerate(sel):
                keep[s0 + t][s] = k[t]
                new[s0 + t][s] = v[t]
    return keep, new, iters


def _track(rng, L, W=640, H=480):
    """A jittered box moving across L frames."""
    x1, y1 = rng.uniform(0, W * 0.6), rng.uniform(0, H * 0.6)
    w, h = rng.uniform(30, W * 0.35), rng.uniform(30, H * 0.35)
    vx, vy = rng.normal(0, 2), rng.normal(0, 2)
    out = []
    for t in range(L):
        b = np.array([x1 + vx * t, y1 + vy * t, x1 + vx * t + w, y1 + vy * t + h]) + rng.normal(0, 1.5, 4)
        out.append(np.clip(b, 0, [W - 1, H - 1, W - 1, H - 1]))
    return np.asarray(out, np.float32)


def make_videos(seed, n_videos=6, max_len=40, classes=30, tracks=4, clutter=6, tie_scores=True, special=True,
                lengths=None):
    """Seeded synthetic videos: temporally coherent jittered tracks (scores with dips), clutter, scores on a coarse grid
    (ties) with tie_scores; with special=True also exact-threshold IoU pairs (0.5 link, f32(0.3) suppression), equal boxes
    of different classes, empty frames and an empty video.  -> (frames, videos)"""
    rng = np.random.default_rng(seed)
    frames, videos = [], []
    lens = list(lengths) if lengths is not None else [int(rng.integers(1, max_len + 1)) for _ in range(n_videos)]
    if special and lengths is None:
        lens[min(1, len(lens) - 1)] = 0          # an empty video
    for L in lens:
        start = len(frames)
        videos.append((start, L))
        trk = [(_track(rng, L), int(rng.integers(1, classes + 1)), int(rng.integers(0, max(L, 1))),
                int(rng.integers(1, L + 1)) if L else 0) for _ in range(tracks)]
        for t in range(L):
            boxes, scores, labels = [], [], []
            if special and t % 7 == 3:
                frames.append({"box": np.zeros((0, 4), np.float32), "score": np.zeros(0, np.float32),
                               "label": np.zeros(0, np.int64)})
                continue
            for tb, c, t0, n in trk:
                if t0 <= t < t0 + n:
                    boxes.append(tb[t])
                    s = rng.uniform(0.5, 1.0) if rng.random() > 0.2 else rng.uniform(0.0, 0.2)   # dips
                    scores.append(s)
                    labels.append(c)
            for _ in range(int(rng.integers(0, clutter + 1))):
                cx, cy = rng.uniform(0, 640), rng.uniform(0, 480)
                w, h = rng.uniform(8, 200), rng.uniform(8, 200)
                boxes.append([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])
                scores.append(rng.uniform(0, 0.3))
                labels.append(int(rng.integers(1, classes + 1)))
            if special and t % 5 == 1:
                c = int(rng.integers(1, classes + 1))
                # exact IoU 0.5 with [0,0,9,9] (50 / 100) and exact f32(0.3) ([0,0,9,2]: 30 / 100); equal boxes, 2 classes
                boxes += [[0, 0, 9, 9], [0, 0, 9, 4], [0, 0, 9, 2], [100, 100, 140, 150], [100, 100, 140, 150]]
                scores += [0.5, 0.5, 0.25, 0.75, 0.75]
                labels += [c, c, c, c, c % classes + 1]
            score = np.asarray(scores, np.float64)
            if tie_scores:
                score = np.round(score * 8) / 8
            frames.append({"box": np.asarray(boxes, np.float32).reshape(-1, 4), "score": score.astype(np.float32),
                           "label": np.asarray(labels, np.int64)})
    return frames, videos


def to_boxlists(frames, size=(640, 480)):
    import torch
    from mega.pytorch_amd.structures import BoxList
    out = []
    for f in frames:
        b = BoxList(torch.from_numpy(np.asarray(f["box"], np.float32).reshape(-1, 4).copy()), tuple(f.get("size", size)))
        b.add_field("scores", torch.from_numpy(np.asarray(f["score"], np.float32).copy()))
        b.add_field("labels", torch.from_numpy(np.asarray(f["label"], np.int64).copy()))
        out.append(b)
    return out


def from_boxlists(predictions):
    return [{"box": p.bbox.cpu().numpy().reshape(-1, 4), "score": p.get_field("scores").cpu().numpy(),
             "label": p.get_field("labels").cpu().numpy(), "size": tuple(p.size)} for p in predictions]
