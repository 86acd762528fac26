"""Test helper: a numpy f32 twin of the VID proposal recall the HIP kernel implements (mega/pytorch_amd/vid_eval.py
evaluate_proposals, csrc/proposal_recall.hip), written as the reference's loop (vid_eval.py:72-119) with the orders this
package defines: proposals by descending objectness, equal values by ascending position; among equal IoUs the lower GT
index, then the lower proposal position (torch's CPU max(dim) returns the first maximum).

Frames are dicts:  proposals {"box": [n,4] f32, "obj": [n] f32, "size": (width, height)},
                   GT        {"box": [g,4] f32, "im_info": (height, width)}.
"""
import numpy as np

import vid_twin


def desc_order(obj):
    """objectness descending, equal values by ascending position (-0 and +0 are equal)."""
    return np.argsort(-(np.asarray(obj, np.float32) + np.float32(0)), kind="stable")


def match_frame(p, g, limit):
    """-> (gt_overlap [G] f32, gt_prop [G] i32) of one frame: per GT box the IoU it was matched with (0: none) and the
    matched proposal's position in the frame's objectness order (-1: none)."""
    gb = np.asarray(g["box"], np.float32).reshape(-1, 4)
    G = len(gb)
    ov = np.zeros(G, np.float32)
    pr = np.full(G, -1, np.int32)
    order = desc_order(p["obj"])[:limit]
    P = len(order)
    if G == 0 or P == 0:
        return ov, pr
    pb = vid_twin.rescale(np.asarray(p["box"], np.float32).reshape(-1, 4)[order], p["size"], g["im_info"])
    iou = vid_twin.iou_f32(pb, gb)                      # [P, G]
    iou = np.where(np.isnan(iou), np.float32(-np.inf), iou).astype(np.float32)     # a NaN IoU is never chosen
    for _ in range(min(P, G)):
        col_arg = iou.argmax(axis=0)                    # first maximum: the lower proposal position
        col_max = iou[col_arg, np.arange(G)]
        gi = int(col_max.argmax())                      # first maximum: the lower GT index
        if col_max[gi] == -np.inf:
            break
        pi = int(col_arg[gi])
        ov[gi] = iou[pi, gi]
        pr[gi] = pi
        iou[pi, :] = -np.inf
        iou[:, gi] = -np.inf
    return ov, pr


def match(preds, gts, limit=300):
    """All frames -> (gt_overlap [G_total] f32, gt_prop [G_total] i32), GT boxes frame by frame."""
    outs = [match_frame(p, g, limit) for p, g in zip(preds, gts)]
    if not outs:
        return np.zeros(0, np.float32), np.zeros(0, np.int32)
    return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])


def recall(gt_overlap, iou_thresh=0.5):
    """(gt_overlaps >= iou_thresh).float().sum() / float(num_pos) in f32 (vid_eval.py:115); NaN without GT boxes."""
    n = len(gt_overlap)
    if n == 0:
        return np.float32(np.nan)
    return np.float32(np.count_nonzero(gt_overlap >= np.float32(iou_thresh))) / np.float32(n)


def result_text(rec):
    return "Recall: {:.4f}".format(rec)


def make_frames(seed, F=80, max_gt=8, max_prop=60, ties=False, special=True):
    """Seeded synthetic frames: proposals jittered around GT boxes, clutter and exact duplicates of earlier proposals;
    prediction sizes whose width and height ratios to the annotation differ.  special=True plants: frame 3 without GT,
    frame 5 without proposals, frame 7 with 12 GT boxes and 4 proposals, frame 9 with 450 proposals, frame 11 with one
    GT box and one proposal.  ties=False: all objectness values of a frame are distinct; True: values on a grid of 8
    (ties in objectness; the duplicates tie in IoU either way).  -> (preds, gts)"""
    rng = np.random.default_rng(seed)
    sizes = ((640, 480), (500, 375), (1280, 720), (1000, 600))
    preds, gts = [], []
    for f in range(F):
        H, W = [(480, 640), (375, 500), (720, 1280)][f % 3]
        psize = sizes[(f * 7 + 1) % len(sizes)] if f % 4 else (W, H)
        g = int(rng.integers(0, max_gt + 1))
        n = int(rng.integers(0, max_prop + 1))
        if special:
            g, n = {3: (0, max(n, 5)), 5: (max(g, 2), 0), 7: (12, 4), 9: (max(g, 3), 450), 11: (1, 1)}.get(f, (g, n))
        x1 = rng.uniform(0, W * 0.7, g)
        y1 = rng.uniform(0, H * 0.7, g)
        gb = np.round(np.stack([x1, y1, np.minimum(x1 + rng.uniform(8, W * 0.3, g), W - 1),
                                np.minimum(y1 + rng.uniform(8, H * 0.3, g), H - 1)], 1)).astype(np.float32).reshape(-1, 4)
        sx, sy = psize[0] / float(W), psize[1] / float(H)
        boxes = []
        for i in range(n):
            u = rng.random()
            if boxes and u < 0.15:
                b = boxes[int(rng.integers(0, len(boxes)))].copy()       # an exact duplicate
            elif g and u < 0.65:
                b = gb[int(rng.integers(0, g))] + rng.normal(0, 6, 4)
                b = np.clip([b[0] * sx, b[1] * sy, b[2] * sx, b[3] * sy], 0, [psize[0] - 1, psize[1] - 1] * 2)
            else:
                cx, cy = rng.uniform(0, W), rng.uniform(0, H)
                w, h = rng.uniform(4, W / 3), rng.uniform(4, H / 3)
                b = np.clip([(cx - w / 2) * sx, (cy - h / 2) * sy, (cx + w / 2) * sx, (cy + h / 2) * sy], 0,
                            [psize[0] - 1, psize[1] - 1] * 2)
            boxes.append(np.asarray(b, np.float64))
        box = np.asarray(boxes, np.float32).reshape(-1, 4)
        if ties:
            obj = (rng.integers(0, 8, n) / 8.0).astype(np.float32)
        else:
            obj = ((rng.permutation(4 * n + 4)[:n] + 1).astype(np.float64) / (4 * n + 5)).astype(np.float32)
        preds.append({"box": box, "obj": obj, "size": tuple(int(v) for v in psize)})
        gts.append({"box": gb, "im_info": (H, W)})
    return preds, gts


def to_boxlists(preds, gts):
    """the twin's frame dicts -> (list[BoxList] with "objectness", VIDGroundTruth) for mega.pytorch_amd.vid_eval."""
    import torch
    from mega.pytorch_amd import vid_eval
    from mega.pytorch_amd.structures import BoxList
    out = []
    for p in preds:
        b = BoxList(torch.from_numpy(np.asarray(p["box"], np.float32).reshape(-1, 4).copy()), tuple(p["size"]))
        b.add_field("objectness", torch.from_numpy(np.asarray(p["obj"], np.float32).copy()))
        out.append(b)
    gt = vid_eval.VIDGroundTruth.from_annotations(
        [{"boxes": g["box"], "labels": np.ones(len(g["box"]), np.int64), "im_info": g["im_info"]} for g in gts])
    return out, gt


def from_fixture(z):
    """ref_proposal_recall.npz -> (preds, gts)."""
    preds, gts = [], []
    for f in range(len(z["pred_off"]) - 1):
        s, e = z["pred_off"][f], z["pred_off"][f + 1]
        preds.append({"box": z["pred_box"][s:e], "obj": z["pred_obj"][s:e], "size": tuple(int(v) for v in z["pred_size"][f])})
        s, e = z["gt_off"][f], z["gt_off"][f + 1]
        gts.append({"box": z["gt_box"][s:e], "im_info": tuple(int(v) for v in z["gt_hw"][f])})
    return preds, gts
