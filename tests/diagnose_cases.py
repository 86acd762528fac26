"""Test helper: the cases of the detection error diagnosis (mega/pytorch_amd/diagnose.py), as tests/vid_twin.py's frame
dicts.  All boxes lie on integer lattices and the prediction frame equals the annotation's (ratio 1), except the rescale
case.

The IoU is vid_iou: +1 on x2 / y2, then the +1 convention, so a box [x1, y1, x2, y2] has the side terms x2 - x1 + 2 and
y2 - y1 + 2.  The hand-built frames rest on the GT box A = [0, 0, 18, 18] (20 x 20 = 400):
  [0, 0, 18, 8]  -> 20 x 10 = 200, IoU exactly 0.5        [0, 0, 17, 8] -> 19 x 10 = 190, IoU 0.475 (one step below)
  [0, 0, 18, 0]  -> 20 x 2  = 40,  IoU exactly 0.1f       [0, 0, 17, 0] -> 19 x 2  = 38,  IoU 0.095 (one step below)
  [0, 0, 18, 7]  -> 20 x 9  = 180, IoU 0.45
(GT [0, 0, 9, 9] with the detection [0, 0, 9, 4] gives 66 / 121 under this IoU, not 0.5: the side terms are 11 and 6.)

hand_cases() -> {name: {"preds", "gts", "kind": expected det_kind, "gt": expected det_gt, "gt_det": expected [3][G],
"state": expected GT states, "dap_nonneg": whether every dAP >= 0 is provable for the case}}.
"""
import numpy as np

A = [0, 0, 18, 18]
HALF, BELOW_HALF = [0, 0, 18, 8], [0, 0, 17, 8]
TENTH, BELOW_TENTH = [0, 0, 18, 0], [0, 0, 17, 0]
NEAR = [0, 0, 18, 7]          # IoU 0.45 with A
FAR = [100, 100, 120, 120]    # IoU 0 with everything near the origin
TP, DUPE, LOC, CLS, BOTH, BKG = range(6)
DETECTED, LOC_COVERED, CLS_COVERED, MISSED = range(4)
MARGIN = 1e-4


def frame(dets, gts, size=(200, 200), im_info=(200, 200)):
    """dets: [(box, score, label)], gts: [(box, label)] -> (prediction dict, GT dict)."""
    p = {"box": np.asarray([d[0] for d in dets], np.float32).reshape(-1, 4),
         "score": np.asarray([d[1] for d in dets], np.float32), "label": np.asarray([d[2] for d in dets], np.int64),
         "size": size}
    g = {"box": np.asarray([b for b, _ in gts], np.float32).reshape(-1, 4),
         "label": np.asarray([l for _, l in gts], np.int64), "im_info": im_info}
    return p, g


def _case(frames, kind, gt, gt_det, state, dap_nonneg=True):
    return {"preds": [f[0] for f in frames], "gts": [f[1] for f in frames], "kind": kind, "gt": gt, "gt_det": gt_det,
            "state": state, "dap_nonneg": dap_nonneg}


def hand_cases():
    c = {}
    # the thresholds, hit exactly and missed by one lattice step; a wrong label turns LOC into BOTH and TP into CLS
    c["thresholds_same_label"] = _case(
        [frame([(HALF, 0.9, 1)], [(A, 1)]), frame([(BELOW_HALF, 0.9, 1)], [(A, 1)]), frame([(TENTH, 0.9, 1)], [(A, 1)]),
         frame([(BELOW_TENTH, 0.9, 1)], [(A, 1)])],
        [TP, LOC, LOC, BKG], [0, 1, 2, -1], [[0, -1, -1, -1], [-1, 1, 2, -1], [-1, -1, -1, -1]],
        [DETECTED, LOC_COVERED, LOC_COVERED, MISSED])
    c["thresholds_other_label"] = _case(
        [frame([(HALF, 0.9, 2)], [(A, 1)]), frame([(BELOW_HALF, 0.9, 2)], [(A, 1)]), frame([(TENTH, 0.9, 2)], [(A, 1)]),
         frame([(BELOW_TENTH, 0.9, 2)], [(A, 1)])],
        [CLS, BOTH, BOTH, BKG], [0, 1, 2, -1], [[-1] * 4, [-1] * 4, [0, -1, -1, -1]],
        [CLS_COVERED, MISSED, MISSED, MISSED])
    # a >= tf and b >= tf: DUPE, attributed to the box of its own label
    c["dupe_before_cls"] = _case(
        [frame([(A, 0.9, 1), (A, 0.8, 1)], [(A, 2), (A, 1)])],
        [TP, DUPE], [1, 1], [[-1, 0], [-1, -1], [-1, -1]], [MISSED, DETECTED])
    # tb <= a < tf and b >= tf: LOC
    c["loc_before_cls"] = _case(
        [frame([(NEAR, 0.9, 1)], [(NEAR, 2), (A, 1)])],
        [LOC], [1], [[-1, -1], [-1, 0], [-1, -1]], [MISSED, LOC_COVERED])
    # equal IoU to two GT boxes: the lower index, in the matching and in both attributions
    c["equal_iou_lower_index"] = _case(
        [frame([(A, 0.9, 1), (A, 0.8, 1), (A, 0.7, 1), (A, 0.6, 2), (NEAR, 0.5, 1)], [(A, 1), (A, 1)])],
        [TP, TP, DUPE, CLS, LOC], [0, 1, 0, 0, 0], [[0, 1], [4, -1], [3, -1]], [DETECTED, DETECTED])
    c["equal_iou_lower_index_loc"] = _case(
        [frame([(NEAR, 0.9, 1), (NEAR, 0.8, 2)], [(A, 1), (A, 1), (A, 3), (A, 3)])],
        [LOC, BOTH], [0, 0], [[-1] * 4, [0, -1, -1, -1], [-1] * 4], [LOC_COVERED, MISSED, MISSED, MISSED])
    # two LOC detections of equal score on one GT box: the higher position is the best one
    c["two_loc_equal_score"] = _case(
        [frame([(NEAR, 0.7, 1), (NEAR, 0.7, 1), (NEAR, 0.6, 1)], [(A, 1)])],
        [LOC, LOC, LOC], [0, 0, 0], [[-1], [1], [-1]], [LOC_COVERED])
    c["two_cls_equal_score"] = _case(
        [frame([(A, 0.7, 2), (A, 0.7, 2), (A, 0.75, 3), (A, 0.75, 3)], [(A, 1)])],
        [CLS, CLS, CLS, CLS], [0, 0, 0, 0], [[-1], [-1], [3]], [CLS_COVERED])
    # a detected GT box that also draws a LOC and a CLS detection; the score order decides who is the TP
    c["detected_with_loc_and_cls"] = _case(
        [frame([(NEAR, 0.95, 1), (A, 0.9, 1), (A, 0.85, 2), (HALF, 0.99, 1)], [(A, 1)])],
        [LOC, DUPE, CLS, TP], [0, 0, 0, 0], [[3], [0], [2]], [DETECTED])
    # a frame without GT (all BKG), a frame without detections (all MISSED), and one ordinary frame
    c["empty_frames"] = _case(
        [frame([(A, 0.9, 1), (NEAR, 0.8, 2), (FAR, 0.7, 1)], []), frame([], [(A, 1), (FAR, 2)]),
         frame([(A, 0.6, 1)], [(A, 1)])],
        [BKG, BKG, BKG, TP], [-1, -1, -1, 2], [[-1, -1, 3], [-1] * 3, [-1] * 3], [MISSED, MISSED, DETECTED])
    # no GT at all: every AP is NaN
    c["no_gt_anywhere"] = _case([frame([(A, 0.9, 1), (FAR, 0.8, 2)], [])], [BKG, BKG], [-1, -1],
                                [[], [], []], [], dap_nonneg=False)
    # the rescale: a (100, 50) prediction frame against a 200 x 200 annotation, ratios 2 and 4
    c["rescale"] = _case(
        [frame([([0, 0, 9, 2], 0.9, 1), ([0, 0, 9, 1.75], 0.8, 1), ([0, 0, 9, 0], 0.7, 2)], [(A, 1)], size=(100, 50))],
        [TP, LOC, BOTH], [0, 0, 0], [[0], [1], [-1]], [DETECTED])
    # a label taken in score order across labels: the lower-scored own-label detection still gets its box
    c["other_label_does_not_take"] = _case(
        [frame([(A, 0.9, 2), (A, 0.5, 1), (FAR, 0.4, 2)], [(A, 1), (FAR, 3)])],
        [CLS, TP, CLS], [0, 0, 1], [[1, -1], [-1, -1], [0, 2]], [DETECTED, CLS_COVERED])
    return c


def exact_ious():
    """(detection, GT, the f32 value the IoU must equal) of the exact cases."""
    return [(HALF, A, np.float32(0.5)), (TENTH, A, np.float32(0.1)), (A, A, np.float32(1))]


def near_threshold(iou, bg_thresh=0.1):
    """True when any IoU of the array lies within MARGIN of a threshold without equalling it."""
    v = np.asarray(iou, np.float32).reshape(-1)
    v = v[~np.isnan(v)]
    for t in (np.float32(0.5), np.float32(bg_thresh)):
        if ((np.abs(v.astype(np.float64) - float(t)) < MARGIN) & (v != t)).any():
            return True
    return False


def _draw(rng, n_det, n_gt, hi, labels, jitter):
    gx1, gy1 = rng.integers(0, hi - 20, n_gt), rng.integers(0, hi - 20, n_gt)
    gb = np.stack([gx1, gy1, np.minimum(gx1 + rng.integers(4, hi // 2, n_gt), hi),
                   np.minimum(gy1 + rng.integers(4, hi // 2, n_gt), hi)], 1).astype(np.float32).reshape(-1, 4)
    gl = rng.choice(labels, n_gt)
    box, lab = [], []
    for _ in range(n_det):
        if n_gt and rng.random() < 0.75:
            k = int(rng.integers(0, n_gt))
            b = gb[k] + rng.integers(-jitter, jitter + 1, 4)
            l = gl[k] if rng.random() < 0.6 else rng.choice(labels)
        else:
            b = rng.integers(0, hi + 1, 4).astype(np.float32)
            l = rng.choice(labels)
        b = np.clip(b, 0, hi)
        box.append([min(b[0], b[2]), min(b[1], b[3]), max(b[0], b[2]), max(b[1], b[3])])
        lab.append(int(l))
    score = (rng.integers(1, 9, n_det) / 8.0).astype(np.float32)          # a coarse grid: ties
    dets = [(box[i], score[i], lab[i]) for i in range(n_det)]
    return frame(dets, [(gb[k], int(gl[k])) for k in range(n_gt)], size=(hi + 1, hi + 1), im_info=(hi + 1, hi + 1))


def _drawn(rng, iou_of, *args):
    """One frame that keeps the margin, and the number of frames drawn for it."""
    drawn = 0
    while True:
        p, g = _draw(rng, *args)
        drawn += 1
        if not (len(p["score"]) and len(g["label"])) or not near_threshold(iou_of(p, g)):
            return (p, g), drawn


def random_frames(iou_of, seed=0, frames=250):
    """Seeded random frames: 12 detections x 4 GT boxes, coordinates in 0 .. 79, 3 labels, scores on a coarse grid.  A
    frame is redrawn when any IoU lies within MARGIN of a threshold without equalling it.  iou_of(p, g): the [n, g] f32
    IoUs of a frame (the twin's).  -> (preds, gts, frames drawn, frames redrawn)"""
    rng = np.random.default_rng(seed)
    out, drawn = [], 0
    for _ in range(frames):
        f, d = _drawn(rng, iou_of, 12, 4, 79, (1, 2, 3), 6)
        out.append(f)
        drawn += d
    return [f[0] for f in out], [f[1] for f in out], drawn, drawn - frames


def size_frames(iou_of, seed=1):
    """A frame with 65 GT boxes and 130 detections (two lane chunks of GT boxes, three strides of detections; its last GT
    box, index 64, is matched by a detection of its own), one with 0 GT boxes and 130 detections, one with 65 GT boxes and
    no detection.  -> (preds, gts)"""
    rng = np.random.default_rng(seed)
    while True:
        (p, g), _ = _drawn(rng, iou_of, 129, 65, 299, (1, 2, 3), 5)
        p = {"box": np.concatenate([p["box"], g["box"][64:65]]), "score": np.concatenate([p["score"], np.float32([1.0])]),
             "label": np.concatenate([p["label"], g["label"][64:65]]), "size": p["size"]}
        if not near_threshold(iou_of(p, g)):
            break
    (p0, g0), _ = _drawn(rng, iou_of, 130, 0, 299, (1, 2, 3), 5)
    (p2, g2), _ = _drawn(rng, iou_of, 0, 65, 299, (1, 2, 3), 5)
    return [p, p0, p2], [g, g0, g2]


def motion_table(gts, seed=2):
    """Per-frame motion IoU lists for `gts`: values on a grid with the boundaries 0.7 and 0.9 hit exactly, and every fifth
    frame with GT boxes without a list."""
    rng = np.random.default_rng(seed)
    grid = np.asarray([0.0, 0.3, 0.65, 0.7, 0.8, 0.9, 0.95, 1.0])
    out, k = [], 0
    for g in gts:
        n = len(g["label"])
        if n and k % 5 == 4:
            out.append([])
        else:
            out.append([float(v) for v in rng.choice(grid, n)] if n else [0.0])
        k += 1 if n else 0
    return out
