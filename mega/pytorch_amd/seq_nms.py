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

from . import vid_eval
from .structures import BoxList

RESCORE_MODES = ("avg", "max")


def _video_ranges(videos, F):
    """(start, length) int64 arrays from (start, length) pairs or {"start", "seg_len"} records; ValueError unless they
    partition [0, F) into contiguous ranges, in order."""
    vs, vl = [], []
    for v in videos:
        if isinstance(v, dict):
            s, n = v["start"], v["seg_len"]
        else:
            s, n = v
        vs.append(int(s))
        vl.append(int(n))
    vs, vl = np.asarray(vs, np.int64), np.asarray(vl, np.int64)
    pos = 0
    for s, n in zip(vs, vl):
        if s != pos or n < 0:
            raise ValueError("seq_nms: the videos must partition the %d frames into contiguous ranges in order "
                             "(a video starts at %d, expected %d, length %d)" % (F, s, pos, n))
        pos += n
    if pos != F:
        raise ValueError("seq_nms: the videos cover %d frames, the predictions hold %d" % (pos, F))
    return vs, vl


def check_params(link_iou, nms_iou, rescore):
    if rescore not in RESCORE_MODES:
        raise ValueError("seq_nms: rescore must be one of %s, got %r" % (RESCORE_MODES, rescore))
    for name, v in (("link_iou", link_iou), ("nms_iou", nms_iou)):
        if not (0.0 <= float(v) <= 1.0):
            raise ValueError("seq_nms: %s must lie in [0, 1], got %r" % (name, v))
    return float(np.float32(link_iou)), float(np.float32(nms_iou))


def pack(predictions, videos):
    """Host checks and flat arrays: dict of counts [F], off [F+1], boxes [N,4] f32, scores [N] f32 (-0 -> +0), labels [N]
    i64, video start / length [V] i64, C (classes: max label + 1)."""
    F = len(predictions)
    counts, off, boxes, scores, labels = vid_eval.concat_predictions(predictions)
    vs, vl = _video_ranges(videos, F)
    N = int(off[-1])
    if not np.isfinite(boxes).all():
        raise ValueError("seq_nms: a prediction box is not finite")
    if np.isnan(scores).any() or (scores < 0).any():
        raise ValueError("seq_nms: a prediction score is negative or NaN")
    if N and labels.min() < 0:
        raise ValueError("seq_nms: negative class label")
    C = int(labels.max()) + 1 if N else 0
    if N > 0x7fffffff or C * F >= 0x7fffffff:
        raise ValueError("seq_nms: %d boxes, %d classes x %d frames: too many" % (N, C, F))
    return {"F": F, "N": N, "C": C, "counts": counts, "off": off, "boxes": boxes, "scores": scores + np.float32(0),
            "labels": labels, "video_start": vs, "video_len": vl}


def run(predictions, videos, link_iou=0.5, nms_iou=0.3, rescore="avg", device="cuda", with_stats=False):
    """Seq-NMS as flat host arrays over the boxes in frame-by-frame order: {"keep": [N] bool, "scores": [N] f32 (the new
    score where keep), plus the packed input under "packed"}; with_stats also "tasks" [T,3] (class, first frame, frames)
    and "stats" [T,2] (iterations, DP frame steps) per task, longest task first."""
    link, nms = check_params(link_iou, nms_iou, rescore)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("seq_nms runs on a HIP device (no CPU path); got device %r" % (device,))
    pk = pack(predictions, videos)
    F, N, C = pk["F"], pk["N"], pk["C"]
    out = {"packed": pk, "keep": np.zeros(N, bool), "scores": np.zeros(N, np.float32)}
    if with_stats:
        out["tasks"], out["stats"] = np.zeros((0, 3), np.int32), np.zeros((0, 2), np.int64)
    if N == 0:
        return out
    from . import ops
    buf, layout = vid_eval.one_buffer([("box", pk["boxes"]), ("score", pk["scores"]), ("label", pk["labels"]),
                                       ("count", pk["counts"]), ("vs", pk["video_start"]), ("vl", pk["video_len"])])
    t = vid_eval.device_views(torch.from_numpy(buf).to(dev), layout)
    with torch.cuda.device(dev):
        # (class, frame) segments: a stable sort by class * F + frame keeps each frame's boxes in position order
        fid = torch.repeat_interleave(torch.arange(F, device=dev), t["count"], output_size=N)
        key = t["label"] * F + fid
        order = torch.sort(key, stable=True).indices
        seg_off = torch.zeros(C * F + 1, dtype=torch.int64, device=dev)
        seg_off[1:] = torch.cumsum(torch.bincount(key, minlength=C * F), 0)
        box_s = t["box"][order].contiguous()
        score_s = t["score"][order].contiguous()
        # tasks: every (class, video) with a box, the most boxes first (ties: class, then video)
        cls = torch.arange(C, device=dev)[:, None] * F
        first = seg_off[cls + t["vs"][None, :]]
        cnt = (seg_off[cls + (t["vs"] + t["vl"])[None, :]] - first).reshape(-1)
        ids = torch.nonzero(cnt > 0).reshape(-1)
        ids = ids[torch.sort(cnt[ids], descending=True, stable=True).indices]
        V = t["vs"].shape[0]
        tasks = torch.stack([ids // V, t["vs"][ids % V], t["vl"][ids % V]], 1).to(torch.int32).contiguous()
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
