"""Seq-NMS (Han et al., 2016, "Seq-NMS for Video Object Detection"): video-level rescoring of per-frame detections.

The reference has no Seq-NMS; this module defines it, and the kernels (csrc/seq_nms.hip) and the test twin
(tests/seq_nms_twin.py) implement this definition.

Input: predictions, a list[BoxList] in dataset order (bbox [n,4] xyxy f32, fields "scores" f32 >= 0 and "labels" int >= 0),
and videos, (start, length) pairs (or VIDTestIndex.videos records) that partition [0, len(predictions)) into contiguous
ranges.  Parameters: link_iou = 0.5, nms_iou = 0.3 (both rounded to f32, compared in f32), rescore = "avg" or "max".

IoU, the +1 convention of boxlist_iou, in f32 and in this order (boxes as each BoxList carries them, no rescale):
    area(b) = (b.x2 - b.x1 + 1) * (b.y2 - b.y1 + 1)
    w = max(min(a.x2, b.x2) - max(a.x1, b.x1) + 1, 0);  h likewise in y
    iou = (w * h) / ((area(a) + area(b)) - w * h)
A NaN IoU (0 / 0) neither links nor suppresses.

Classes and videos are independent (no links across a video boundary).  For each (video, class), with A_t the alive
boxes of that class in frame t (at first all of them), repeat until every A_t is empty:
  1. forward DP in f64, t ascending: S(t,i) = s(t,i) + max{ S(t-1,j) : j in A_{t-1}, iou(j,i) > link_iou }, or s(t,i)
     without such a j; P(t,i) = the arg-max j, the smallest position j on equal S, -1 without a j ("position": the index
     in the frame's BoxList);
  2. the (t*, i*) with the largest S over all alive boxes; on equal S the earliest t, then the smallest position;
     backtrack through P to the path t0 .. t*;
  3. rescore: "avg" gives every path box f32(S(t*,i*) / L) (the division in f64, L the path length), "max" the largest
     original score on the path;
  4. in every path frame remove from A_t the path box and every alive box k with iou(k, path box) > nms_iou (strict >,
     as NMS_STRICT_GT); the removed non-path boxes are suppressed.
With scores >= 0 a linked predecessor never lowers S, so step 1 has no max(0, .).  A one-frame video is greedy per-class
NMS at nms_iou with strict >.  A score of -0.0 counts as +0.0.

Output: a new list[BoxList] of the same sizes and modes; each frame keeps its path boxes in their original order with
"scores" the rescored values, every other field filtered by the same mask; suppressed boxes are dropped.

All input checks run on the host before any device work (ValueError).  There is no CPU path: the work runs on a HIP
device, one workgroup per (video, class) task with an incremental DP (csrc/seq_nms.hip).
"""
import numpy as np
import torch

from . import flat
from .structures import BoxList

RESCORE_MODES = ("avg", "max")


def check_params(link_iou=0.5, nms_iou=0.3, rescore="avg"):
    if rescore not in RESCORE_MODES:
        raise ValueError("seq_nms: rescore must be one of %s, got %r" % (RESCORE_MODES, rescore))
    for name, v in (("link_iou", link_iou), ("nms_iou", nms_iou)):
        if not (0.0 <= float(v) <= 1.0):
            raise ValueError("seq_nms: %s must lie in [0, 1], got %r" % (name, v))
    return float(np.float32(link_iou)), float(np.float32(nms_iou))


def pack(predictions, videos):
    """flat.pack with this module's error prefix (tracks reuses it, prefix included)."""
    return flat.pack(predictions, videos, "seq_nms")


def run(predictions, videos, link_iou=0.5, nms_iou=0.3, rescore="avg", device="cuda", with_stats=False):
    """Seq-NMS as flat host arrays over the boxes in frame-by-frame order: {"keep": [N] bool, "scores": [N] f32 (the new
    score where keep), plus the packed input under "packed"}; with_stats also "tasks" [T,3] (class, first frame, frames)
    and "stats" [T,2] (iterations, DP frame steps) per task, longest task first."""
    link, nms = check_params(link_iou, nms_iou, rescore)
    dev = torch.device(device)
    flat.require_hip(dev, "seq_nms", device)
    pk = pack(predictions, videos)
    F, N, C = pk["F"], pk["N"], pk["C"]
    out = {"packed": pk, "keep": np.zeros(N, bool), "scores": np.zeros(N, np.float32)}
    if with_stats:
        out["tasks"], out["stats"] = np.zeros((0, 3), np.int32), np.zeros((0, 2), np.int64)
    if N == 0:
        return out
    from . import ops
    with torch.cuda.device(dev):
        v = flat.video_tasks(pk, dev, by_score=False)      # each (class, frame) segment in position order
        order, seg_off, tasks = v["order"], v["seg_off"], v["tasks"]
        box_s = v["t"]["box"][order].contiguous()
        score_s = v["t"]["score"][order].contiguous()
        keep_s, ns_s, stats = ops.seq_nms(box_s, score_s, seg_off, tasks, F, C, link, nms, rescore == "max")
        res = torch.empty(N * 5, dtype=torch.uint8, device=dev)      # [new scores f32 | keep u8]: one copy back
        res[:4 * N].view(torch.float32)[order] = ns_s
        res[4 * N:][order] = keep_s
        host = res.cpu().numpy()
        if with_stats:
            out["tasks"], out["stats"] = tasks.cpu().numpy(), stats.cpu().numpy()
    out["scores"] = host[:4 * N].view(np.float32).copy()
    out["keep"] = host[4 * N:].astype(bool)
    return out


def _split(predictions, keep, new_scores, counts):
    """The output list[BoxList]: each frame's kept boxes in order, "scores" replaced, every other field masked."""
    F = len(predictions)
    names = predictions[0].fields() if F else []
    for p in predictions:
        if sorted(p.fields()) != sorted(names):
            raise ValueError("seq_nms: every BoxList must carry the same fields")
    kept_counts = np.bincount(np.repeat(np.arange(F), counts)[keep], minlength=F).tolist()
    mask = torch.from_numpy(keep)
    per_field = {}
    for name in ["__bbox__"] + [k for k in names if k != "scores"]:
        parts = [p.bbox.reshape(-1, 4) if name == "__bbox__" else p.get_field(name) for p in predictions]
        for p, x in zip(predictions, parts):
            if x.shape[0] != len(p):
                raise ValueError("seq_nms: field %r does not hold one entry per box" % name)
        cat = torch.cat(parts) if parts else torch.zeros(0)
        per_field[name] = torch.split(cat[mask.to(cat.device)], kept_counts)
    sc = torch.from_numpy(new_scores[keep].copy())
    sdev = predictions[0].get_field("scores").device if F else torch.device("cpu")
    per_field["scores"] = torch.split(sc.to(sdev), kept_counts)
    out = []
    for f, p in enumerate(predictions):
        b = BoxList(per_field["__bbox__"][f], p.size, p.mode)
        for k in names:
            b.add_field(k, per_field[k][f])
        out.append(b)
    return out


def seq_nms(predictions, videos, link_iou=0.5, nms_iou=0.3, rescore="avg", device="cuda"):
    """Seq-NMS of `predictions` (list[BoxList]) over `videos` ((start, length) pairs, e.g. from
    inference.VIDTestIndex(img_index).videos) -> a new list[BoxList] (see the module docstring for the definition)."""
    r = run(predictions, videos, link_iou, nms_iou, rescore, device)
    return _split(predictions, r["keep"], r["scores"], r["packed"]["counts"])
