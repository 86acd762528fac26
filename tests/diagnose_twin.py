"""Test helper: a plain Python / numpy twin of the detection error diagnosis, written as loops from the docstring of
mega/pytorch_amd/diagnose.py (not from the kernel).  The IoU is tests/vid_twin.py's: BoxList.resize's f32 rescale, +1 on
x2 / y2, boxlist_iou in f32 in the reference's operation order.  The fixed rows are built here and their AP computed with
vid_twin.ap_from.

Frames are vid_twin's dicts: predictions {"box" [n,4] f32, "score" [n] f32, "label" [n] int, "size" (width, height)},
GT {"box" [g,4] f32, "label" [g] int, "im_info" (height, width)}.

fault: None, or one planted deviation from the definition (tests/test_diagnose.py shows the cases catch each):
  "cls_first"   CLS / BOTH are tested before DUPE / LOC (swapped precedence)
  "strict"      thresholds compared with > instead of >=
  "tie_high"    an equal IoU goes to the higher GT index
"""
import warnings

import numpy as np

import vid_twin

KINDS = ("TP", "DUPE", "LOC", "CLS", "BOTH", "BKG")
TP, DUPE, LOC, CLS, BOTH, BKG = range(6)
GT_STATES = ("DETECTED", "LOC_COVERED", "CLS_COVERED", "MISSED")
FIXES = ("dupe", "loc", "cls", "both", "bkg", "miss")
MOTION_NAMES = ("fast", "medium", "slow")
MOTION_RANGES = vid_twin.MOTION_RANGES[1:]


def frame_iou(p, g):
    """[n, g] f32: every detection of the frame against every GT box."""
    pb = vid_twin.rescale(p["box"], p["size"], g["im_info"]).copy()
    pb[:, 2:] += np.float32(1)
    gb = np.asarray(g["box"], np.float32).reshape(-1, 4).copy()
    gb[:, 2:] += np.float32(1)
    return vid_twin.iou_f32(pb, gb).astype(np.float32).reshape(len(pb), len(gb))


def classify(preds, gts, bg_thresh=0.1, fault=None):
    """Steps 1 to 3 -> det_kind [N] u8, det_gt [N] i32, det_iou [N] f32, gt_det [3,G] i32."""
    tf, tb = np.float32(0.5), np.float32(bg_thresh)

    def reaches(v, t):          # f32 >=; false on NaN
        return bool(v > t) if fault == "strict" else bool(v >= t)

    def better(v, cur):         # a strictly larger IoU; the planted fault also lets an equal one at a higher index win
        return cur is None or bool(v > cur) or (fault == "tie_high" and bool(v == cur))

    N = sum(len(p["score"]) for p in preds)
    G = sum(len(g["label"]) for g in gts)
    det_kind = np.full(N, 255, np.uint8)
    det_gt = np.full(N, -1, np.int32)
    det_iou = np.zeros(N, np.float32)
    gt_det = np.full((3, G), -1, np.int32)
    d0 = g0 = 0
    for p, g in zip(preds, gts):
        n, m = len(p["score"]), len(g["label"])
        score = np.asarray(p["score"], np.float32).reshape(-1)
        lab = [int(v) for v in np.asarray(p["label"]).reshape(-1)]
        glab = [int(v) for v in np.asarray(g["label"]).reshape(-1)]
        iou = frame_iou(p, g) if n and m else np.zeros((n, m), np.float32)
        # step 1: per label, descending score, equal scores by descending position
        taken = [False] * m
        kind = [None] * n
        for l in sorted(set(lab)):
            sel = sorted((j for j in range(n) if lab[j] == l), key=lambda j: (-float(score[j]), -j))
            for j in sel:
                best, arg = None, -1
                for k in range(m):
                    if glab[k] != l or taken[k] or not reaches(iou[j, k], tf):
                        continue
                    if better(iou[j, k], best):
                        best, arg = iou[j, k], k
                if arg >= 0:
                    taken[arg] = True
                    kind[j] = TP
                    det_gt[d0 + j] = g0 + arg
                    det_iou[d0 + j] = best
        # step 2
        for j in range(n):
            if kind[j] == TP:
                continue
            a = b = None
            ga = gb = -1
            for k in range(m):
                v = iou[j, k]
                if np.isnan(v):
                    continue
                if glab[k] == lab[j]:
                    if better(v, a):
                        a, ga = v, k
                elif better(v, b):
                    b, gb = v, k
            same = [(DUPE, a, ga, lambda v: reaches(v, tf)), (LOC, a, ga, lambda v: reaches(v, tb))]
            other = [(CLS, b, gb, lambda v: reaches(v, tf)), (BOTH, b, gb, lambda v: reaches(v, tb))]
            kind[j] = BKG
            for kd, v, k, rule in (other + same if fault == "cls_first" else same + other):
                if v is not None and rule(v):
                    kind[j] = kd
                    det_gt[d0 + j] = g0 + k
                    det_iou[d0 + j] = v
                    break
        det_kind[d0:d0 + n] = kind
        # step 3: the highest score, equal scores to the higher position
        for k in range(m):
            for row, kd in ((0, TP), (1, LOC), (2, CLS)):
                best = -1
                for j in range(n):
                    if kind[j] != kd or det_gt[d0 + j] != g0 + k:
                        continue
                    if best < 0 or score[j] >= score[best]:
                        best = j
                if best >= 0:
                    gt_det[row, g0 + k] = d0 + best
        d0 += n
        g0 += m
    return det_kind, det_gt, det_iou, gt_det


def gt_states(gt_det):
    out = np.zeros(gt_det.shape[1], np.uint8)
    for g in range(gt_det.shape[1]):
        out[g] = 0 if gt_det[0, g] >= 0 else 1 if gt_det[1, g] >= 0 else 2 if gt_det[2, g] >= 0 else 3
    return out


def class_ap(preds, labels, match, pign, n_pos):
    """AP per class of one row: labels / match / pred_ignore per detection (flat), n_pos [C].  The order is the
    evaluation's: per class the frames' detections, each frame's by descending score (equal scores: descending position),
    concatenated, then by descending score (equal scores: descending position in that concatenation)."""
    C = len(n_pos)
    score = np.concatenate([np.asarray(p["score"], np.float32).reshape(-1) for p in preds]) if preds else np.zeros(0)
    offs = np.concatenate([[0], np.cumsum([len(p["score"]) for p in preds])]).astype(np.int64)
    prec, rec = [None] * C, [None] * C
    for l in range(C):
        idx = []
        for fi in range(len(preds)):
            sel = np.nonzero(labels[offs[fi]:offs[fi + 1]] == l)[0] + offs[fi]
            idx.extend(sel[vid_twin.desc_order(score[sel])])
        idx = np.asarray(idx, np.int64)
        idx = idx[vid_twin.desc_order(score[idx])]
        m_l, pi_l = match[idx].astype(np.int8), pign[idx].astype(np.float64)
        tps = np.logical_and(m_l == 1, np.logical_not(pi_l == 1))
        fps = np.logical_and(m_l == 0, np.logical_not(pi_l == 1))
        pi_l[pi_l == 0] = 1
        fps = fps * pi_l
        tp, fp = np.cumsum(tps), np.cumsum(fps)
        prec[l] = tp / (fp + tp + np.spacing(1))
        if n_pos[l] > 0:
            rec[l] = tp / n_pos[l]
    return vid_twin.ap_from(prec, rec)


def nanmean(a):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return float(np.nanmean(a))


def fixed_rows(preds, gts, det_kind, det_gt, gt_det):
    """Step 4 -> {"base" / fix: (labels, match, pred_ignore, n_pos)}."""
    labels = np.concatenate([np.asarray(p["label"]).astype(np.int64).reshape(-1) for p in preds])
    gl = np.concatenate([np.asarray(g["label"]).astype(np.int64).reshape(-1) for g in gts])
    C = int(max(labels.max() if labels.size else -1, gl.max() if gl.size else -1)) + 1
    N = len(labels)
    n_pos = np.zeros(C, np.int64)
    for l in gl:
        n_pos[l] += 1
    base = (det_kind == TP).astype(np.uint8)
    zero = np.zeros(N, np.float64)
    rows = {"base": (labels, base, zero, n_pos)}
    for name, kd in (("dupe", DUPE), ("both", BOTH), ("bkg", BKG)):
        rows[name] = (labels, base, (det_kind == kd).astype(np.float64), n_pos)
    for name, kd, row in (("loc", LOC, 1), ("cls", CLS, 2)):
        match, pign, lab = base.copy(), zero.copy(), labels.copy()
        for d in range(N):
            if det_kind[d] != kd:
                continue
            g = det_gt[d]
            if gt_det[0, g] < 0 and gt_det[row, g] == d:
                match[d] = 1
            else:
                pign[d] = 1
            if kd == CLS:
                lab[d] = gl[g]
        rows[name] = (lab, match, pign, n_pos)
    low = n_pos.copy()
    for g, s in enumerate(gt_states(gt_det)):
        if s == 3:
            low[gl[g]] -= 1
    rows["miss"] = (labels, base, zero, low)
    return rows


def tables(preds, gts, det_kind, det_gt, gt_det, score_thresh=0.5, motion=None):
    labels = np.concatenate([np.asarray(p["label"]).astype(np.int64).reshape(-1) for p in preds])
    score = np.concatenate([np.asarray(p["score"], np.float32).reshape(-1) for p in preds])
    gl = np.concatenate([np.asarray(g["label"]).astype(np.int64).reshape(-1) for g in gts])
    C = int(max(labels.max() if labels.size else -1, gl.max() if gl.size else -1)) + 1
    t = {"kind_counts": np.zeros(6, np.int64), "kind_counts_thr": np.zeros(6, np.int64),
         "kind_counts_by_label": np.zeros((C, 6), np.int64), "kind_counts_thr_by_label": np.zeros((C, 6), np.int64),
         "gt_state_counts": np.zeros(4, np.int64), "gt_state_counts_by_label": np.zeros((C, 4), np.int64),
         "confusion": np.zeros((C, C), np.int64), "motion": None}
    thr = np.float32(score_thresh)
    for d in range(len(labels)):
        k = int(det_kind[d])
        t["kind_counts"][k] += 1
        t["kind_counts_by_label"][labels[d], k] += 1
        if score[d] >= thr:
            t["kind_counts_thr"][k] += 1
            t["kind_counts_thr_by_label"][labels[d], k] += 1
            if k == CLS:
                t["confusion"][labels[d], gl[det_gt[d]]] += 1
    state = gt_states(gt_det)
    for g in range(len(gl)):
        t["gt_state_counts"][state[g]] += 1
        t["gt_state_counts_by_label"][gl[g], state[g]] += 1
    if motion is not None:
        # a GT box's motion IoU: its frame's list entry; a frame with an empty list has none
        mot = []
        for fi, g in enumerate(gts):
            m = list(motion[fi])
            mot.extend([float(m[k]) if m else None for k in range(len(g["label"]))])
        gs, ks = np.zeros((3, 4), np.int64), np.zeros((3, 4), np.int64)
        for ri, (lo, hi) in enumerate(MOTION_RANGES):
            inr = [v is not None and lo <= v <= hi for v in mot]
            for g in range(len(gl)):
                if inr[g]:
                    gs[ri, state[g]] += 1
            for d in range(len(labels)):
                if det_kind[d] in (DUPE, LOC, CLS, BOTH) and inr[det_gt[d]]:
                    ks[ri, int(det_kind[d]) - 1] += 1
        t["motion"] = {"gt_state_counts": gs, "kind_counts": ks}
    return t


def format_result(res):
    def row(names, counts):
        return " ".join("%s %d" % (n, int(c)) for n, c in zip(names, counts))
    lines = ["mAP = %0.4f" % res["map"]]
    lines += ["dAP %-4s = %0.4f" % (k, res["dap"][k]) for k in FIXES]
    lines.append("kinds | all          : " + row(KINDS, res["kind_counts"]))
    lines.append("kinds | score>=%-5.2f : " % res["score_thresh"] + row(KINDS, res["kind_counts_thr"]))
    lines.append("GT    | all          : " + row(GT_STATES, res["gt_state_counts"]))
    if res["motion"] is not None:
        for ri, name in enumerate(MOTION_NAMES):
            lines.append("GT    | motion=%6s: " % name + row(GT_STATES, res["motion"]["gt_state_counts"][ri]))
            lines.append("kinds | motion=%6s: " % name + row(KINDS[1:5], res["motion"]["kind_counts"][ri]))
    return "\n".join(lines) + "\n"


def run(preds, gts, motion=None, score_thresh=0.5, bg_thresh=0.1, fault=None):
    """The whole diagnosis -> dict with evaluate_errors' keys."""
    det_kind, det_gt, det_iou, gt_det = classify(preds, gts, bg_thresh, fault)
    rows = fixed_rows(preds, gts, det_kind, det_gt, gt_det)
    ap = {k: class_ap(preds, *v) for k, v in rows.items()}
    res = {"det_kind": det_kind, "det_gt": det_gt, "det_iou": det_iou, "gt_det": gt_det, "gt_state": gt_states(gt_det),
           "ap": ap["base"], "map": nanmean(ap["base"]), "score_thresh": float(score_thresh), "bg_thresh": float(bg_thresh)}
    res["dap"] = {k: nanmean(ap[k]) - res["map"] for k in FIXES}
    res["dap_by_class"] = {k: ap[k] - ap["base"] for k in FIXES}
    res["rows"] = rows
    res.update(tables(preds, gts, det_kind, det_gt, gt_det, score_thresh, motion))
    res["text"] = format_result(res)
    return res
