"""Test helper: a numpy twin of the VID evaluation the HIP kernels implement (mega/pytorch_amd/vid_eval.py), written as
the reference's loops (vid_eval.py:156-343) with the tie order this package defines (equal scores by descending
position: a stable ascending argsort reversed) and BoxList.resize's f32 rescale.

Frames are dicts:  predictions {"box": [n,4] f32, "score": [n] f32, "label": [n] int, "size": (width, height)},
                   GT          {"box": [g,4] f32, "label": [g] int, "im_info": (height, width)}.
"""
from collections import defaultdict

import numpy as np

MOTION_RANGES = [[0.0, 1.0], [0.0, 0.7], [0.7, 0.9], [0.9, 1.0]]


def desc_order(score):
    return np.argsort(score, kind="stable")[::-1]


def rescale(box, size, im_info):
    """BoxList.resize((width, height)) of the annotation: Python-float ratios applied in f32."""
    rw = np.float32(float(im_info[1]) / float(size[0]))
    rh = np.float32(float(im_info[0]) / float(size[1]))
    box = np.asarray(box, np.float32).reshape(-1, 4)
    return np.stack([box[:, 0] * rw, box[:, 1] * rh, box[:, 2] * rw, box[:, 3] * rh], axis=1).astype(np.float32)


def iou_f32(a, b):
    """boxlist_iou (TO_REMOVE = 1) in f32, the reference's operation order."""
    one = np.float32(1)
    area1 = (a[:, 2] - a[:, 0] + one) * (a[:, 3] - a[:, 1] + one)
    area2 = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    lt = np.maximum(a[:, None, :2], b[:, :2])
    rb = np.minimum(a[:, None, 2:], b[:, 2:])
    wh = np.clip(rb - lt + one, np.float32(0), None)
    inter = wh[:, :, 0] * wh[:, :, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / ((area1[:, None] + area2) - inter)


def empty_weight(motion, lo, hi):
    if motion is None:
        return 0
    allm = np.concatenate([np.asarray(m, np.float64).reshape(-1) for m in motion])
    w = sum([(allm[i] >= lo) & (allm[i] <= hi) for i in range(len(allm))]) / float(len(allm))
    return 0 if w == 1 else w


def prec_rec(preds, gts, motion=None, motion_range=(0.0, 1.0), iou_thresh=0.5):
    """calc_detection_vid_prec_rec.  Also returns per-detection match / pred_ignore (flat, original prediction order)."""
    n_pos = defaultdict(int)
    score = defaultdict(list)
    match = defaultdict(list)
    pred_ignore = defaultdict(list)
    flat = defaultdict(list)
    offs = np.concatenate([[0], np.cumsum([len(p["score"]) for p in preds])]).astype(np.int64)
    N = int(offs[-1])
    m_det = np.zeros(N, np.uint8)
    pi_det = np.zeros(N, np.float64)
    ew = empty_weight(motion, *motion_range)
    for fi, (p, g) in enumerate(zip(preds, gts)):
        mi = None if motion is None else list(motion[fi])
        pred_bbox = rescale(p["box"], p["size"], g["im_info"])
        pred_label = np.asarray(p["label"]).astype(int).reshape(-1)
        pred_score = np.asarray(p["score"], np.float32).reshape(-1)
        gt_bbox = np.asarray(g["box"], np.float32).reshape(-1, 4)
        gt_label = np.asarray(g["label"]).astype(int).reshape(-1)
        gt_ignore = np.zeros(len(gt_bbox))
        for k in range(len(gt_bbox)):
            if mi:
                gt_ignore[k] = 1 if (mi[k] < motion_range[0] or mi[k] > motion_range[1]) else 0
        for l in np.unique(np.concatenate((pred_label, gt_label)).astype(int)):
            sel = np.nonzero(pred_label == l)[0]
            order = desc_order(pred_score[sel])
            sel = sel[order]
            pb = pred_bbox[sel]
            gm = gt_label == l
            gb = gt_bbox[gm]
            gi = gt_ignore[gm]
            n_pos[l] += gb.shape[0] - sum(gi)
            score[l].extend(pred_score[sel])
            flat[l].extend(offs[fi] + sel)
            if len(pb) == 0:
                continue
            if len(gb) == 0:
                match[l].extend((0,) * len(pb))
                pred_ignore[l].extend((ew,) * len(pb))
                continue
            pb = pb.copy()
            pb[:, 2:] += 1
            gb = gb.copy()
            gb[:, 2:] += 1
            iou = iou_f32(pb, gb)
            selec = np.zeros(len(gb), dtype=bool)
            for j in range(len(pb)):
                iou_match, ig, nig, arg = iou_thresh, -1, -1, -1
                for k in range(len(gb)):
                    if (gi[k] == 1) & (iou[j, k] > ig):
                        ig = iou[j, k]
                    if (gi[k] == 0) & (iou[j, k] > nig):
                        nig = iou[j, k]
                    if selec[k] or iou[j, k] < iou_match:
                        continue
                    if iou[j, k] == iou_match:
                        if arg < 0 or gi[arg]:
                            arg = k
                    else:
                        arg = k
                    iou_match = iou[j, k]
                if arg >= 0:
                    match[l].append(1)
                    pred_ignore[l].append(gi[arg])
                    selec[arg] = True
                else:
                    if nig > ig:
                        pred_ignore[l].append(0)
                    elif ig > nig:
                        pred_ignore[l].append(1)
                    else:
                        pred_ignore[l].append(sum(gi) / float(len(gb)))
                    match[l].append(0)
    for l in flat:
        if len(match[l]):
            m_det[np.asarray(flat[l], np.int64)] = match[l]
            pi_det[np.asarray(flat[l], np.int64)] = pred_ignore[l]
    n_fg_class = max(n_pos.keys()) + 1
    prec = [None] * n_fg_class
    rec = [None] * n_fg_class
    for l in n_pos.keys():
        score_l = np.array(score[l])
        match_l = np.array(match[l], dtype=np.int8)
        pi_l = np.array(pred_ignore[l], dtype=np.float64)
        order = desc_order(score_l)
        match_l = match_l[order]
        pi_l = pi_l[order]
        tps = np.logical_and(match_l == 1, np.logical_not(pi_l == 1))
        fps = np.logical_and(match_l == 0, np.logical_not(pi_l == 1))
        pi_l[pi_l == 0] = 1
        fps = fps * pi_l
        tp = np.cumsum(tps)
        fp = np.cumsum(fps)
        prec[l] = tp / (fp + tp + np.spacing(1))
        if n_pos[l] > 0:
            rec[l] = tp / n_pos[l]
    npos = np.zeros(n_fg_class, np.int64)
    for l, v in n_pos.items():
        npos[l] = int(v)
    return {"prec": prec, "rec": rec, "match": m_det, "pred_ignore": pi_det, "n_pos": npos,
            "match_l": {int(l): np.asarray(v, np.int64) for l, v in match.items()},
            "pred_ignore_l": {int(l): np.asarray(v, np.float64) for l, v in pred_ignore.items()}}


def ap_from(prec, rec):
    """calc_detection_vid_ap, use_07_metric=False."""
    ap = np.empty(len(prec))
    for l in range(len(prec)):
        if prec[l] is None or rec[l] is None:
            ap[l] = np.nan
            continue
        mpre = np.concatenate(([0], np.nan_to_num(prec[l]), [0]))
        mrec = np.concatenate(([0], rec[l], [1]))
        mpre = np.maximum.accumulate(mpre[::-1])[::-1]
        i = np.where(mrec[1:] != mrec[:-1])[0]
        ap[l] = np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])
    return ap


def evaluate(preds, gts, motion=None):
    """eval_detection_vid -> list over ranges of the prec_rec dict plus "ap" / "map"."""
    ranges = MOTION_RANGES if motion is not None else MOTION_RANGES[:1]
    out = []
    for r in ranges:
        d = prec_rec(preds, gts, motion, r)
        d["ap"] = ap_from(d["prec"], d["rec"])
        with np.errstate(invalid="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                d["map"] = np.nanmean(d["ap"])
        out.append(d)
    return out


def from_boxlists(predictions, groundtruth):
    """(list[BoxList], VIDGroundTruth) -> the twin's frame dicts."""
    preds = [{"box": p.bbox.cpu().numpy().reshape(-1, 4), "score": p.get_field("scores").cpu().numpy(),
              "label": p.get_field("labels").cpu().numpy(), "size": tuple(p.size)} for p in predictions]
    gts = []
    for i in range(len(groundtruth)):
        s, e = groundtruth.off[i], groundtruth.off[i + 1]
        gts.append({"box": groundtruth.boxes[s:e], "label": groundtruth.labels[s:e],
                    "im_info": (int(groundtruth.height[i]), int(groundtruth.width[i]))})
    return preds, gts


def make_frames(seed, F=80, max_det=40, max_gt=8, min_det=0, min_gt=0, labels=(1, 3, 4, 7, 9, 12), gt_only=(14,), pred_only=(15,),
                sizes=((640, 480), (500, 375), (1280, 720)), tie_scores=False, motion=True, special=True):
    """Seeded synthetic frames: detections jittered around GT boxes plus clutter, unequal rescale ratios, frames without
    predictions / GT, classes present only in predictions or only in GT; with special=True also exact IoU = 0.5 pairs,
    degenerate boxes, an IoU that is 0 / 0, and motion IoUs at exactly 0.7 / 0.9 and frames with an empty motion list.
    tie_scores=False: every score is distinct (no ties within a frame's class or a class); True: scores on a coarse grid.
    -> (preds, gts, motion lists or None)"""
    rng = np.random.default_rng(seed)
    preds, gts, mot = [], [], []
    n_total = F * max_det
    pool = (rng.permutation(n_total * 4)[:n_total] + 1).astype(np.float64) / (n_total * 4 + 1)
    pi = 0
    for f in range(F):
        H, W = [(480, 640), (375, 500), (720, 1280)][f % 3]
        psize = sizes[(f * 7 + 1) % len(sizes)] if f % 4 else (W, H)      # prediction frame (width, height)
        g = 0 if f % 11 == 5 else int(rng.integers(min_gt, max_gt + 1))
        gl = rng.choice(list(labels) + list(gt_only), size=g)
        x1 = rng.uniform(0, W * 0.7, g)
        y1 = rng.uniform(0, H * 0.7, g)
        gb = np.stack([x1, y1, np.minimum(x1 + rng.uniform(8, W * 0.3, g), W - 1),
                       np.minimum(y1 + rng.uniform(8, H * 0.3, g), H - 1)], 1).astype(np.float32).reshape(-1, 4)
        gb = np.round(gb)          # annotations are integral
        n = 0 if f % 9 == 4 else int(rng.integers(min_det, max_det + 1))
        boxes, labs = [], []
        sx, sy = psize[0] / float(W), psize[1] / float(H)
        for i in range(n):
            if g and rng.random() < 0.6:
                k = int(rng.integers(0, g))
                b = gb[k] + rng.normal(0, 6, 4)
                lab = gl[k] if gl[k] not in gt_only else labels[0]
            else:
                cx, cy = rng.uniform(0, W), rng.uniform(0, H)
                w, h = rng.uniform(4, W / 3), rng.uniform(4, H / 3)
                b = np.array([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])
                lab = rng.choice(list(labels) + list(pred_only))
            b = np.array([b[0] * sx, b[1] * sy, b[2] * sx, b[3] * sy])
            b = np.clip(b, 0, [psize[0] - 1, psize[1] - 1] * 2)
            boxes.append(b)
            labs.append(int(lab))
        box = np.asarray(boxes, np.float32).reshape(-1, 4)
        if tie_scores:
            score = (rng.integers(1, 8, n) / 8.0).astype(np.float32)
        else:
            score = pool[pi:pi + n].astype(np.float32)
            pi += n
        label = np.asarray(labs, np.int64)
        if special and f % 13 == 2 and g:
            # exact IoU 0.5 (ratio 1 frame): GT [0,0,8,h] -> width term 10; prediction [0,0,3,h] -> 5, inter 5
            psize = (W, H)
            gb[0] = [0, 0, 8, 20]
            gl[0] = labels[1]
            box = np.concatenate([box, np.asarray([[0, 0, 3, 20], [0, 0, 3, 20]], np.float32)])
            score = np.concatenate([score, np.float32([0.999 - f * 1e-4, 0.998 - f * 1e-4])])
            label = np.concatenate([label, [labels[1], labels[1]]])
        if special and f % 17 == 3:
            # degenerate boxes: zero width (clipped), and an inverted pair whose IoU is 0 / 0 = NaN
            gb = np.concatenate([gb, np.float32([[0, 0, 4, -2]])])
            gl = np.concatenate([gl, [labels[2]]])
            box = np.concatenate([box, np.float32([[30, 30, 30, 50], [10, 10, 5, 8]])])
            score = np.concatenate([score, np.float32([0.997 - f * 1e-4, 0.996 - f * 1e-4])])
            label = np.concatenate([label, [labels[2], labels[2]]])
            psize = (W, H)
        preds.append({"box": box, "score": score, "label": label, "size": tuple(int(v) for v in psize)})
        gts.append({"box": gb.astype(np.float32).reshape(-1, 4), "label": np.asarray(gl, np.int64), "im_info": (H, W)})
        if motion:
            if special and f % 10 == 7:
                mot.append([])
            else:
                m = rng.uniform(0, 1, len(gl))
                if special and len(m) > 1:
                    m[0], m[1] = 0.7, 0.9
                mot.append([float(v) for v in m])
    return preds, gts, (mot if motion else None)


def to_boxlists(preds, gts):
    """the twin's frame dicts -> (list[BoxList], VIDGroundTruth) for mega.pytorch_amd.vid_eval."""
    import torch
    from mega.pytorch_amd import vid_eval
    from mega.pytorch_amd.structures import BoxList
    out = []
    for p in preds:
        b = BoxList(torch.from_numpy(np.asarray(p["box"], np.float32).reshape(-1, 4).copy()), tuple(p["size"]))
        b.add_field("scores", torch.from_numpy(np.asarray(p["score"], np.float32).copy()))
        b.add_field("labels", torch.from_numpy(np.asarray(p["label"], np.int64).copy()))
        out.append(b)
    gt = vid_eval.VIDGroundTruth.from_annotations([{"boxes": g["box"], "labels": g["label"], "im_info": g["im_info"]}
                                                   for g in gts])
    return out, gt
