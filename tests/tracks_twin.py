"""Test helper: a numpy twin of the track linking as mega/pytorch_amd/tracks.py defines it, written as the definition's
loops: frames ascending, candidates in descending score (equal scores by position), per candidate the f32 IoU
(vid_twin.iou_f32, as seq_nms_twin) to the last boxes of the available tracks, the smallest-root tie rule, f64 sums in
frame order.  Plus two seeded generators of GT tracks with detections for the AP tests.

Frames are dicts {"box": [n,4] f32, "score": [n] f32, "label": [n] int} (the shape vid_twin uses, "size" optional);
videos are (start, length) pairs.
"""
import numpy as np

import vid_twin
from seq_nms_twin import from_boxlists, to_boxlists  # noqa: F401  (the same frame dicts <-> list[BoxList])


def _task(boxes, scores, flat, thr, link, max_gap):
    """One (video, class) task: per frame the boxes [n,4], scores [n] and flat indices [n] -> the tracks, each a dict
    {"root": flat index, "members": [(t, i)], "sum": f64, "max": f32}."""
    open_, closed = [], []
    for t in range(len(boxes)):
        keep = []
        for tr in open_:                                           # 1. close
            (closed if tr["last_t"] < t - max_gap - 1 else keep).append(tr)
        open_ = keep
        sc = np.asarray(scores[t], np.float32) + np.float32(0)     # (-0.0 counts as +0.0)
        order = [int(i) for i in np.argsort(-sc, kind="stable") if sc[i] >= thr]      # 2. candidates
        avail = list(open_)                                        # every open track's last frame is < t here
        for i in order:                                            # 3.
            best = None
            if avail:
                last = np.stack([tr["box"] for tr in avail]).astype(np.float32)
                iou = vid_twin.iou_f32(last, boxes[t][i][None])[:, 0]
                with np.errstate(invalid="ignore"):
                    ok = iou > link                                # a NaN IoU never links
                if ok.any():
                    top = iou[ok].max()
                    ties = [k for k in range(len(avail)) if ok[k] and iou[k] == top]
                    best = min(ties, key=lambda k: avail[k]["root"])
            if best is not None:
                tr = avail.pop(best)                               # extended in t: not available any more
                tr["box"], tr["last_t"] = boxes[t][i], t
                tr["members"].append((t, i))
                tr["sum"] = tr["sum"] + np.float64(sc[i])
                tr["max"] = max(tr["max"], sc[i])
            else:
                open_.append({"root": int(flat[t][i]), "box": boxes[t][i], "last_t": t, "members": [(t, i)],
                              "sum": np.float64(sc[i]), "max": sc[i]})
    return closed + open_


def link(frames, videos, score_thresh=0.05, link_iou=0.5, max_gap=1, min_len=1, rescore=None):
    """-> (track ids per frame [n] i64, scores per frame [n] f32, table: a list of (video, id, label, first frame, last
    frame, count, mean f64) rows by video then id)."""
    thr, lnk = np.float32(score_thresh), np.float32(link_iou)
    ids = [np.full(len(f["score"]), -1, np.int64) for f in frames]
    new = [np.asarray(f["score"], np.float32).copy() for f in frames]
    off = np.cumsum([0] + [len(f["score"]) for f in frames])
    table = []
    for vi, (s0, n) in enumerate(videos):
        vf = frames[s0:s0 + n]
        labels = set()
        for f in vf:
            labels.update(np.asarray(f["label"]).astype(int).tolist())
        tracks = []
        for c in sorted(labels):
            sel = [np.nonzero(np.asarray(f["label"]).astype(int) == c)[0] for f in vf]
            boxes = [np.asarray(f["box"], np.float32).reshape(-1, 4)[s] for f, s in zip(vf, sel)]
            scores = [np.asarray(f["score"], np.float32)[s] for f, s in zip(vf, sel)]
            flat = [off[s0 + t] + s for t, s in enumerate(sel)]
            for tr in _task(boxes, scores, flat, thr, lnk, max_gap):
                tr["label"] = c
                tr["members"] = [(t, int(sel[t][i])) for t, i in tr["members"]]
                tracks.append(tr)
        tracks = sorted([tr for tr in tracks if len(tr["members"]) >= min_len], key=lambda tr: tr["root"])
        for k, tr in enumerate(tracks):
            cnt = len(tr["members"])
            mean = tr["sum"] / cnt
            for t, i in tr["members"]:
                ids[s0 + t][i] = k
                if rescore == "avg":
                    new[s0 + t][i] = np.float32(mean)
                elif rescore == "max":
                    new[s0 + t][i] = np.float32(tr["max"])
            table.append((vi, k, tr["label"], tr["members"][0][0], tr["members"][-1][0], cnt, float(mean)))
    return ids, new, table


def rescored(frames, new):
    """The frames with their scores replaced (for vid_twin.evaluate)."""
    return [dict(f, score=s) for f, s in zip(frames, new)]


def ap_set(seed=12, n_videos=8, L=30, distinct_classes=False, p_absent=0.0):
    """GT tracks (3 per video); predictions: the tracks jittered, with score dips, plus two temporally isolated false
    positives per frame whose scores lie between the dips and the track scores.  The defaults restate the dips set of the
    Seq-NMS AP test.  distinct_classes: the three tracks of a video get pairwise distinct classes; p_absent: each track's
    detection is absent with this probability, never in two consecutive frames and never in the first or last frame.
    -> (preds, gts, videos)"""
    rng = np.random.default_rng(seed)
    preds, gts, videos = [], [], []
    for v in range(n_videos):
        videos.append((len(preds), L))
        K = 3
        xy = rng.uniform(0, 300, (K, 2))
        wh = rng.uniform(40, 120, (K, 2))
        cls = rng.choice(np.arange(1, 31), K, replace=False) if distinct_classes else rng.integers(1, 31, K)
        prev_absent = np.zeros(K, bool)
        for t in range(L):
            gb = np.round(np.concatenate([xy + t, xy + t + wh], 1)).astype(np.float32)
            box = gb + rng.normal(0, 1.0, gb.shape).astype(np.float32)
            sc = np.where(rng.random(K) < 0.3, rng.uniform(0.05, 0.15, K), rng.uniform(0.7, 0.95, K))
            present = np.ones(K, bool)
            if p_absent > 0:
                absent = (rng.random(K) < p_absent) & ~prev_absent & (0 < t < L - 1)
                present, prev_absent = ~absent, absent
            nfp = 2
            fxy = rng.uniform(0, 500, (nfp, 2))
            fb = np.concatenate([fxy, fxy + rng.uniform(20, 60, (nfp, 2))], 1)
            preds.append({"box": np.concatenate([box[present], fb]).astype(np.float32),
                          "score": np.concatenate([sc[present], rng.uniform(0.3, 0.5, nfp)]).astype(np.float32),
                          "label": np.concatenate([cls[present], rng.integers(1, 31, nfp)]), "size": (640, 480)})
            gts.append({"box": gb, "label": cls.astype(np.int64), "im_info": (480, 640)})
    return preds, gts, videos


GAP_SEED = 12      # ap_gap_set's seed: the relations the gap test asserts hold for it in this twin


def ap_gap_set(seed=GAP_SEED, n_videos=8, L=30):
    return ap_set(seed, n_videos, L, distinct_classes=True, p_absent=0.2)
