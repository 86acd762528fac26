"""Detection error diagnosis: why the AP is what it is.  Every detection of a VID evaluation gets one kind -- a true
positive, a duplicate, a poorly placed box, a right box with a wrong label, both, or background -- every GT box one state
-- detected, nearly found, or missed -- and every error type a cost: the mAP an oracle would gain by repairing that type
alone.  This is TIDE's taxonomy (Bolya et al., ECCV 2020; Hoiem et al.'s analysis before it) with the same-class
explanations taking precedence: TIDE tests CLS before DUPE, here DUPE and LOC are tested before CLS.

The reference has no counterpart; this docstring defines it, and the kernel (csrc/diagnose.hip) and the test twin
(tests/diagnose_twin.py) implement this definition.

Inputs.  Everything vid_eval.evaluate_detections takes: predictions, a list[BoxList] with "scores" and "labels";
groundtruth, a vid_eval.VIDGroundTruth of the same frames; motion_iou, optional (vid_eval.load_motion_iou's or
motion_iou.derive's per-frame lists), used only for the cross-tabulation at the end.  The host checks are
vid_eval._pack's, raised as ValueError with the prefix "diagnose:".

IoU.  csrc/box_math.h's vid_iou throughout, the detection AP's: the prediction is rescaled by the frame's ratio in f32,
+1 is added on x2 / y2 of both boxes, then box_iou1 (the +1 convention in f32, no FMA contraction).  A NaN IoU satisfies
no comparison (so a pair with a NaN IoU never matches; this is where the matching below parts from
mega_vid_eval_match, which keeps the reference's treatment of a NaN).  Thresholds: tf = 0.5f, fixed as the evaluation's
own, and tb = bg_thresh, default 0.1f, 0 < tb < 0.5; both are compared in f32 with >=.

Step 1, matching.  mega_vid_eval_match's for one range and no motion list: per frame and label the detections go by
descending score, equal scores by descending position in the frame's BoxList.  Each takes the not yet taken GT box of its
label with the largest IoU >= tf, the lowest GT index among equals.  A detection that takes one is a TP and that GT box
is detected.

Step 2, every other detection d (label l) gets one kind.  Over the GT boxes of d's frame: a = the largest IoU with a GT
box of label l and ga that box, the lowest index on a tie; b and gb the same over the GT boxes of any other label.  A
frame or label without such a box gives "none", which meets no threshold.  The first rule that holds decides:
  1. DUPE  a >= tf (every such box is already taken)       attributed to ga
  2. LOC   tb <= a < tf                                     attributed to ga
  3. CLS   b >= tf                                          attributed to gb
  4. BOTH  tb <= b < tf                                     attributed to gb
  5. BKG   otherwise                                        attributed to nothing
Per detection: det_kind u8 (0 TP, 1 DUPE, 2 LOC, 3 CLS, 4 BOTH, 5 BKG), det_gt i32 (the index into groundtruth.boxes of
the matched or attributed box, -1 for BKG), det_iou f32 (the IoU with that box, 0 for BKG).

Step 3, per GT box g three detection indices (into the flat frame-by-frame list), gt_det [3][G] i32, -1 for none: row 0
the TP that took it, row 1 the best LOC detection attributed to it, row 2 the best CLS detection attributed to it.
"Best" is the highest f32 score, on equal scores the higher position in the frame's BoxList.  The state of g follows:
DETECTED (row 0 >= 0); LOC_COVERED (not detected, row 1 >= 0); CLS_COVERED (not detected, row 1 < 0, row 2 >= 0); MISSED
(none of these).

Step 4, the cost of each error type.  dAP_k = the mAP after an oracle repairs type k alone - the mAP; mAP is the nanmean of
the AP over the classes 0 .. C-1, as evaluate_detections forms it, and the AP comes from the unchanged ops.vid_eval_ap.
The base row is match = (kind == TP), pred_ignore = 0, n_pos = the GT boxes per label.  The fixed rows differ from it only
as follows:
  dupe / both / bkg   pred_ignore = 1 on the detections of that kind.
  loc                 a LOC detection d with attributed box g becomes match = 1 if g is not detected and gt_det[1][g] == d;
                      every other LOC detection gets pred_ignore = 1.
  miss                n_pos[c] is lowered by the number of MISSED boxes of label c; where it reaches 0 the kernel's NaN
                      stands.
  cls                 a CLS detection takes its attributed box's label; it becomes match = 1 if that box is not detected
                      and gt_det[2][g] == d, otherwise pred_ignore = 1.  The per-class order and seg_off are rebuilt for
                      the changed labels exactly as the evaluation builds them (vid_eval.class_orders).
The base and the five rows that keep the order go through one vid_eval_ap call (R = 6), the cls row through a second.

Tables (host side, integers).  The counts of the six kinds over all detections and over those with score >= score_thresh
(default 0.5, compared in f32 with >=), and the same per label; the counts of the four GT states, overall and per label;
a confusion matrix [C][C] of the CLS detections with score >= score_thresh, row = the predicted label, column = the GT
label.  With motion_iou, for fast / medium / slow (vid_eval.MOTION_RANGES[1:], bounds inclusive as in the evaluation, so a
boundary value counts in both ranges): the GT states of the boxes in the range, and the DUPE / LOC / CLS / BOTH counts,
over all detections, by the attributed box's range.  GT boxes of frames without a motion list fall in no range.

Text (result_diagnosis.txt), in fixed format: the mAP line, one "dAP <kind> = x.xxxx" line per fix, the two count rows,
the GT-state row and, with motion_iou, two rows per motion range.

There is no CPU path: one wave per frame classifies (csrc/diagnose.hip), the rows are segment operations on the device,
the AP is vid_eval's kernel.  A frame holds at most vid_eval.MAX_GT_PER_FRAME GT boxes.
"""
import warnings

import numpy as np
import torch

from . import flat, vid_eval

KINDS = ("TP", "DUPE", "LOC", "CLS", "BOTH", "BKG")
TP, DUPE, LOC, CLS, BOTH, BKG = range(6)
GT_STATES = ("DETECTED", "LOC_COVERED", "CLS_COVERED", "MISSED")
DETECTED, LOC_COVERED, CLS_COVERED, MISSED = range(4)
FIXES = ("dupe", "loc", "cls", "both", "bkg", "miss")
MOTION_KINDS = (DUPE, LOC, CLS, BOTH)
SCORE_THRESH = 0.5
BG_THRESH = 0.1
RESULT_NAME = "result_diagnosis.txt"


def check_params(score_thresh=SCORE_THRESH, bg_thresh=BG_THRESH):
    """-> (score_thresh, bg_thresh) as floats; ValueError for a value that is no number, a NaN score_thresh or a bg_thresh
    that is not inside (0, 0.5) as an f32."""
    out = []
    for name, v in (("score_thresh", score_thresh), ("bg_thresh", bg_thresh)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("diagnose: %s must be a number, got %r" % (name, v))
        out.append(float(v))
    if np.isnan(out[0]):
        raise ValueError("diagnose: score_thresh is NaN")
    if not np.float32(0) < np.float32(out[1]) < np.float32(0.5):
        raise ValueError("diagnose: bg_thresh must be inside (0, 0.5), got %r" % (bg_thresh,))
    return out[0], out[1]


def _pack(predictions, groundtruth, motion_iou):
    """vid_eval._pack's checked host arrays as a dict, its sizes, and the motion IoU of every GT box (or None)."""
    ranges = vid_eval.MOTION_RANGES if motion_iou is not None else vid_eval.MOTION_RANGES[:1]
    try:
        parts, meta = vid_eval._pack(predictions, groundtruth, motion_iou, ranges)
    except ValueError as e:
        msg = str(e)
        if msg.startswith("evaluate_detections: "):
            msg = msg[len("evaluate_detections: "):]
        raise ValueError("diagnose: " + msg)
    host = dict(parts)
    return host, meta, host.pop("gt_motion", None)


def _run(predictions, groundtruth, motion_iou, bg_thresh, device):
    from . import ops
    dev = torch.device(device)
    host, meta, motion = _pack(predictions, groundtruth, motion_iou)
    flat.require_hip(dev, "evaluate_errors", device)
    names = ("det_box", "score", "det_label", "det_off", "ratio", "gt_box", "gt_label", "gt_off")
    t = flat.upload([(k, host[k]) for k in names], dev)
    order, gorder, seg_off = vid_eval.class_orders(t["score"], t["det_label"], meta["counts"], meta["C"], dev)
    with torch.cuda.device(dev):
        out = ops.diagnose_match(t["det_box"], t["det_label"], t["score"], t["det_off"], order, t["ratio"], t["gt_box"],
                                 t["gt_label"], t["gt_off"], meta["C"], meta["max_gt"], bg_thresh)
    return {"host": host, "meta": meta, "motion": motion, "t": t, "order": order, "gorder": gorder, "seg_off": seg_off,
            "out": dict(zip(("det_kind", "det_gt", "det_iou", "gt_det"), out))}


def run(predictions, groundtruth, bg_thresh=BG_THRESH, device="cuda"):
    """Steps 1 to 3 -> {"det_kind" [N] u8, "det_gt" [N] i32, "det_iou" [N] f32, "gt_det" [3,G] i32}, on the device."""
    _, bg_thresh = check_params(bg_thresh=bg_thresh)
    return _run(predictions, groundtruth, None, bg_thresh, device)["out"]


def gt_states(gt_det):
    """gt_det [3,G] (numpy) -> the state of every GT box, [G] u8."""
    return np.where(gt_det[0] >= 0, DETECTED, np.where(gt_det[1] >= 0, LOC_COVERED,
                                                      np.where(gt_det[2] >= 0, CLS_COVERED, MISSED))).astype(np.uint8)


def tables(det_kind, det_gt, det_label, det_score, gt_det, gt_label, C, score_thresh=SCORE_THRESH, gt_motion=None):
    """The integer tables of the docstring from the per-detection and per-GT arrays (numpy) -> dict."""
    kind = det_kind.astype(np.int64)
    label = det_label.astype(np.int64)
    gl = gt_label.astype(np.int64)
    above = det_score.astype(np.float32) >= np.float32(score_thresh)
    state = gt_states(gt_det).astype(np.int64)
    out = {"kind_counts": np.bincount(kind, minlength=6), "kind_counts_thr": np.bincount(kind[above], minlength=6),
           "kind_counts_by_label": np.bincount(label * 6 + kind, minlength=C * 6).reshape(C, 6),
           "kind_counts_thr_by_label": np.bincount((label * 6 + kind)[above], minlength=C * 6).reshape(C, 6),
           "gt_state_counts": np.bincount(state, minlength=4),
           "gt_state_counts_by_label": np.bincount(gl * 4 + state, minlength=C * 4).reshape(C, 4)}
    sel = (kind == CLS) & above
    out["confusion"] = np.bincount(label[sel] * C + gl[det_gt[sel]], minlength=C * C).reshape(C, C)
    out["motion"] = None
    if gt_motion is not None:
        gs, ks = [], []
        for lo, hi in vid_eval.MOTION_RANGES[1:]:
            inr = (gt_motion >= lo) & (gt_motion <= hi)            # (NaN: the frame has no motion list -- in no range)
            gs.append(np.bincount(state[inr], minlength=4))
            ks.append([int(np.count_nonzero(inr[det_gt[kind == k]])) for k in MOTION_KINDS])
        out["motion"] = {"gt_state_counts": np.asarray(gs, np.int64), "kind_counts": np.asarray(ks, np.int64)}
    return out


def _fixed_rows(st):
    """Step 4 on the device -> (ap [6,C] for base, dupe, loc, both, bkg, miss; ap [C] for cls), f64."""
    from . import ops
    t, o, meta = st["t"], st["out"], st["meta"]
    N, C = meta["N"], meta["C"]
    dev = t["score"].device
    G = t["gt_label"].shape[0]
    kind, gtd = o["det_kind"], o["gt_det"]
    gl = t["gt_label"].long()
    n_pos = torch.bincount(gl, minlength=C).int()
    base = kind == TP
    idx = torch.arange(N, device=dev)
    dg = o["det_gt"].long().clamp(min=0)

    def oracle(k, row):     # the best detection of kind k on a box that is not detected becomes a match, the others go
        isk = kind == k
        if G == 0 or N == 0:
            win = torch.zeros(N, dtype=torch.bool, device=dev)
        else:
            win = isk & (gtd[0][dg] < 0) & (gtd[row][dg].long() == idx)
        return (base | win).to(torch.uint8), (isk & ~win).to(torch.float64)

    zero = torch.zeros(N, dtype=torch.float64, device=dev)
    m0 = base.to(torch.uint8)
    m_loc, p_loc = oracle(LOC, 1)
    match = torch.stack([m0, m0, m_loc, m0, m0, m0]).contiguous()
    pign = torch.stack([zero, (kind == DUPE).to(torch.float64), p_loc, (kind == BOTH).to(torch.float64),
                        (kind == BKG).to(torch.float64), zero]).contiguous()
    missed = (gtd[0] < 0) & (gtd[1] < 0) & (gtd[2] < 0)
    npos = n_pos[None, :].repeat(6, 1)
    npos[5] -= torch.bincount(gl[missed], minlength=C).int()
    m_cls, p_cls = oracle(CLS, 2)
    labels2 = t["det_label"].clone()
    iscls = kind == CLS
    if G and N:
        labels2[iscls] = t["gt_label"][dg[iscls]]
    _, gorder2, seg_off2 = vid_eval.class_orders(t["score"], labels2, meta["counts"], C, dev)
    with torch.cuda.device(dev):
        ap6 = ops.vid_eval_ap(match, pign, st["gorder"], st["seg_off"], npos.contiguous())
        ap_cls = ops.vid_eval_ap(m_cls[None].contiguous(), p_cls[None].contiguous(), gorder2, seg_off2,
                                 n_pos[None].contiguous())
    return ap6.cpu().numpy(), ap_cls.cpu().numpy()[0]


def _nanmean(a):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # nanmean of an all-NaN row is NaN, as in the evaluation
        return float(np.nanmean(a))


def summarize(ap6, ap_cls):
    """ap6 [6,C] (base, dupe, loc, both, bkg, miss) and ap_cls [C] -> (map, {fix: dAP}, {fix: dAP per class [C]})."""
    rows = {"dupe": ap6[1], "loc": ap6[2], "cls": ap_cls, "both": ap6[3], "bkg": ap6[4], "miss": ap6[5]}
    base = _nanmean(ap6[0])
    return base, {k: _nanmean(rows[k]) - base for k in FIXES}, {k: rows[k] - ap6[0] for k in FIXES}


def format_result(res):
    """The text of result_diagnosis.txt from evaluate_errors' dict (or the twin's, with the same keys)."""
    def row(names, counts):
        return " ".join("%s %d" % (n, int(c)) for n, c in zip(names, counts))
    s = "mAP = {:0.4f}\n".format(res["map"])
    for k in FIXES:
        s += "dAP {:<4s} = {:0.4f}\n".format(k, res["dap"][k])
    s += "kinds | all          : " + row(KINDS, res["kind_counts"]) + "\n"
    s += "kinds | score>={:<5.2f} : ".format(res["score_thresh"]) + row(KINDS, res["kind_counts_thr"]) + "\n"
    s += "GT    | all          : " + row(GT_STATES, res["gt_state_counts"]) + "\n"
    if res.get("motion") is not None:
        for ri, name in enumerate(vid_eval.MOTION_NAMES[1:]):
            s += "GT    | motion={:>6s}: ".format(name) + row(GT_STATES, res["motion"]["gt_state_counts"][ri]) + "\n"
            s += "kinds | motion={:>6s}: ".format(name) + row([KINDS[k] for k in MOTION_KINDS],
                                                             res["motion"]["kind_counts"][ri]) + "\n"
    return s


def evaluate_errors(predictions, groundtruth, motion_iou=None, score_thresh=SCORE_THRESH, bg_thresh=BG_THRESH,
                    output_folder=None, device="cuda", logger=None):
    """The diagnosis of `predictions` against `groundtruth` (see the module docstring) -> dict: "map", "ap" [C], "dap" and
    "dap_by_class" ({fix: value} / {fix: [C]} for FIXES), the tables (tables()'s keys), the per-detection arrays "det_kind",
    "det_gt", "det_iou" and the per-GT arrays "gt_det" [3,G], "gt_state" [G] as numpy, "score_thresh", "bg_thresh" and
    "text", which also goes to the log and to <output_folder>/result_diagnosis.txt."""
    score_thresh, bg_thresh = check_params(score_thresh, bg_thresh)
    st = _run(predictions, groundtruth, motion_iou, bg_thresh, device)
    ap6, ap_cls = _fixed_rows(st)
    res = {k: v.cpu().numpy() for k, v in st["out"].items()}
    host, meta = st["host"], st["meta"]
    res.update(tables(res["det_kind"], res["det_gt"], host["det_label"], host["score"], res["gt_det"], host["gt_label"],
                      meta["C"], score_thresh, st["motion"]))
    res["gt_state"] = gt_states(res["gt_det"])
    res["ap"] = ap6[0].copy()
    res["map"], res["dap"], res["dap_by_class"] = summarize(ap6, ap_cls)
    res["score_thresh"], res["bg_thresh"] = score_thresh, bg_thresh
    res["text"] = format_result(res)
    vid_eval.write_result(res["text"], logger, "diagnose", output_folder, RESULT_NAME)
    return res
