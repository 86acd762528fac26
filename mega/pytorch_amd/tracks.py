"""Linking per-frame detections into tracks (tubelets): a "track_ids" field, a per-track table, and the causal
alternative to Seq-NMS that tracks give for free -- a linked box's score replaced by its track's mean or max, frame by
frame in one forward pass, nothing dropped.

The reference has no counterpart; this docstring defines it, and the kernel (csrc/tracks.hip) and the test twin
(tests/tracks_twin.py) implement this definition.

Input, as for Seq-NMS: predictions, a list[BoxList] in dataset order (bbox [n,4] xyxy f32, fields "scores" f32 >= 0 and
"labels" int >= 0), and videos, (start, length) pairs (or VIDTestIndex.videos records) that partition
[0, len(predictions)) into contiguous ranges.  seq_nms.pack and its host checks are reused; every check raises
ValueError before any device work.

Parameters:
    score_thresh = 0.05   rounded to f32 (not NaN); a box takes part iff score >= score_thresh in f32
    link_iou     = 0.5    rounded to f32; must lie in [0, 1]
    max_gap      = 1      int >= 0: frames a track may go without a box
    min_len      = 1      int >= 1
    rescore      = None   None, "avg" or "max"

IoU: exactly Seq-NMS's -- the +1 convention of boxlist_iou, in f32 and in this order (no FMA contraction):
    area(b) = (b.x2 - b.x1 + 1) * (b.y2 - b.y1 + 1)
    w = max(min(a.x2, b.x2) - max(a.x1, b.x1) + 1, 0);  h likewise in y
    iou = (w * h) / ((area(a) + area(b)) - w * h)
A NaN IoU never links.

Linking.  Classes and videos are independent.  For each (video, class), an open track holds its root (the flat index of
its first box; flat index = position in the frame-by-frame concatenation), its last box, the frame of its last box and
its box count.  Go through the frames t in ascending order:
  1. close every open track whose last frame is < t - max_gap - 1;
  2. the candidates are the class's boxes of frame t with score >= score_thresh, taken in descending score; equal scores
     go by ascending position, and -0.0 counts as +0.0;
  3. for each candidate in that order, consider the open tracks whose last frame is < t (a track that was extended or
     born in frame t is not available): pick the one with the largest iou(track's last box, candidate), requiring
     iou > link_iou (strict); on equal IoU the smallest root.  If one is found the candidate joins it (the track's last
     box and last frame are updated and its count grows by one); otherwise the candidate opens a new track with itself as
     the root.
Boxes below score_thresh belong to no track.

Ids.  Within each video, the tracks of all classes with at least min_len boxes are numbered 0, 1, ... by ascending root.
Every member box gets that number, every other box -1.

Rescoring.  Only members of numbered tracks change: "avg" gives every member f32(sum of the members' f32 scores, added
in f64 in frame order, / count), "max" the largest member score.  Every other score is unchanged, bit for bit.

Output: a new list[BoxList] of the same sizes, order, modes and fields, plus "track_ids" (int64) and, with rescore, new
"scores"; and a track table, one row per numbered track: video index, id, label, first frame, last frame (both relative
to the video), box count and mean score (f64: the f64 sum / count).

There is no CPU path: the association runs on a HIP device, one workgroup per (video, class) task (csrc/tracks.hip); the
ids, the rescoring and the table are a few segment operations on the device over the kernel's per-box root and per-root
count / sum / max, then one copy back.
"""
import numpy as np
import torch

from . import flat, seq_nms, vid_eval
from .structures import BoxList

RESCORE_MODES = (None, "avg", "max")
TABLE_DTYPE = np.dtype([("video", np.int64), ("id", np.int64), ("label", np.int64), ("first", np.int64),
                        ("last", np.int64), ("count", np.int64), ("mean", np.float64)])


def check_params(score_thresh=0.05, link_iou=0.5, max_gap=1, min_len=1, rescore=None):
    """-> (score_thresh, link_iou) rounded to f32 (as Python floats), max_gap, min_len; ValueError for a bad value."""
    if rescore not in RESCORE_MODES:
        raise ValueError("tracks: rescore must be one of %s, got %r" % (RESCORE_MODES, rescore))
    if not (0.0 <= float(link_iou) <= 1.0):
        raise ValueError("tracks: link_iou must lie in [0, 1], got %r" % (link_iou,))
    if float(score_thresh) != float(score_thresh):
        raise ValueError("tracks: score_thresh must not be NaN")
    for name, v, lo in (("max_gap", max_gap, 0), ("min_len", min_len, 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or v > 0x7fffffff:
            raise ValueError("tracks: %s must be an int >= %d, got %r" % (name, lo, v))
    return float(np.float32(score_thresh)), float(np.float32(link_iou)), int(max_gap), int(min_len)


def _empty_table():
    return np.zeros(0, TABLE_DTYPE)


def run(predictions, videos, score_thresh=0.05, link_iou=0.5, max_gap=1, min_len=1, rescore=None, device="cuda"):
    """The linking as flat host arrays over the boxes in frame-by-frame order: {"track_ids": [N] i64, "scores": [N] f32
    (rescored where rescore is set and the box is in a numbered track, else the packed input score, a -0.0 as +0.0), "table": the track table (a
    structured array, TABLE_DTYPE, rows by video then id), "packed": the packed input (seq_nms.pack)}."""
    thr, link, max_gap, min_len = check_params(score_thresh, link_iou, max_gap, min_len, rescore)
    dev = torch.device(device)
    flat.require_hip(dev, "tracks", device)
    pk = seq_nms.pack(predictions, videos)
    F, N, C = pk["F"], pk["N"], pk["C"]
    out = {"packed": pk, "track_ids": np.full(N, -1, np.int64), "scores": pk["scores"].copy(), "table": _empty_table()}
    if N == 0:
        return out
    from . import ops
    with torch.cuda.device(dev):
        # each (class, frame) segment in descending score, equal scores in position order
        v = flat.video_tasks(pk, dev, by_score=True)
        t, fid, order, seg_off, tasks, V = v["t"], v["fid"], v["order"], v["seg_off"], v["tasks"], v["V"]
        box_s = t["box"][order].contiguous()
        score_s = t["score"][order].contiguous()
        pos_s = order.to(torch.int32)
        # open tracks of a task <= its boxes in max_gap + 2 consecutive frames (each open track's last box is one of them);
        # a window that runs over a video or class boundary only over-counts
        w = min(max_gap + 2, C * F)
        max_open = int((seg_off[w:] - seg_off[:-w]).max())
        root_s, cnt_s, sum_s, max_s = ops.link_tracks(box_s, score_s, pos_s, seg_off, tasks, F, C, thr, link, max_gap,
                                                      max_open)
        # back to the frame-by-frame order
        ar = torch.arange(N, device=dev)
        root = torch.empty(N, dtype=torch.int64, device=dev)
        root[order] = torch.where(root_s >= 0, order[root_s.clamp(min=0)], root_s)
        tcnt = torch.empty(N, dtype=torch.int64, device=dev)
        tcnt[order] = cnt_s.to(torch.int64)
        tsum = torch.empty(N, dtype=torch.float64, device=dev)
        tsum[order] = sum_s
        tmax = torch.empty(N, dtype=torch.float32, device=dev)
        tmax[order] = max_s
        rf = root.clamp(min=0)
        numbered = (root >= 0) & (tcnt[rf] >= min_len)              # member of a track that gets an id
        mark = (numbered & (root == ar)).to(torch.int64)            # ... and its root
        before = torch.cumsum(mark, 0) - mark                       # numbered roots with a smaller flat index
        off = torch.zeros(F + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(t["count"], 0)
        vid_of_frame = flat.frame_ids(t["vl"], dev, F)             # the same op over videos: each frame's video
        box_vid = vid_of_frame[fid]
        vid_base = before[off[t["vs"]].clamp(max=N - 1)]            # (a video without boxes is never looked up)
        ids = torch.where(numbered, before[rf] - vid_base[box_vid], torch.full_like(root, -1))
        if rescore == "avg":
            new = torch.where(numbered, (tsum[rf] / tcnt[rf].to(torch.float64)).to(torch.float32), t["score"])
        elif rescore == "max":
            new = torch.where(numbered, tmax[rf], t["score"])
        else:
            new = t["score"]
        roots = torch.nonzero(mark).reshape(-1)
        sel = torch.nonzero(numbered).reshape(-1)
        last = torch.zeros(N, dtype=torch.int64, device=dev).scatter_reduce_(0, rf[sel], fid[sel], "amax")
        rv = box_vid[roots]
        tab_i = torch.stack([rv, ids[roots], t["label"][roots], fid[roots] - t["vs"][rv], last[roots] - t["vs"][rv],
                             tcnt[roots]], 1).contiguous()
        mean = tsum[roots] / tcnt[roots].to(torch.float64)
        K = int(roots.shape[0])
        # [ids i32 | scores f32 | table i64 [K,6] | mean f64 [K]]: one copy back
        res = torch.cat([ids.to(torch.int32).view(torch.uint8), new.contiguous().view(torch.uint8),
                         tab_i.view(torch.uint8).reshape(-1), mean.view(torch.uint8)])
        host = res.cpu().numpy()
    out["track_ids"] = host[:4 * N].view(np.int32).astype(np.int64)
    out["scores"] = host[4 * N:8 * N].view(np.float32).copy()
    ti = host[8 * N:8 * N + 48 * K].view(np.int64).reshape(K, 6)
    table = np.zeros(K, TABLE_DTYPE)
    for k, name in enumerate(("video", "id", "label", "first", "last", "count")):
        table[name] = ti[:, k]
    table["mean"] = host[8 * N + 48 * K:].view(np.float64)
    out["table"] = table
    return out


def _attach(predictions, track_ids, new_scores, counts):
    """The output list[BoxList]: every BoxList copied with its fields, plus "track_ids"; "scores" replaced if given."""
    F = len(predictions)
    names = predictions[0].fields() if F else []
    for p in predictions:
        if sorted(p.fields()) != sorted(names):
            raise ValueError("tracks: every BoxList must carry the same fields")
    split = [int(c) for c in counts]
    ids = torch.split(torch.from_numpy(track_ids.astype(np.int64)), split) if F else []
    sc = None
    if new_scores is not None and F:
        sc = torch.split(torch.from_numpy(np.ascontiguousarray(new_scores, np.float32)), split)
    out = []
    for f, p in enumerate(predictions):
        b = BoxList(p.bbox, p.size, p.mode)
        for k in names:
            v = p.get_field(k)
            if k == "scores" and sc is not None:      # (the others keep their own bits: run() carries -0.0 as +0.0)
                v = torch.where((ids[f] >= 0).to(v.device).reshape(v.shape), sc[f].to(v.device).reshape(v.shape), v)
            b.add_field(k, v)
        b.add_field("track_ids", ids[f].to(p.bbox.device))
        out.append(b)
    return out


def link(predictions, videos, score_thresh=0.05, link_iou=0.5, max_gap=1, min_len=1, rescore=None, device="cuda"):
    """Link `predictions` (list[BoxList]) over `videos` ((start, length) pairs, e.g. from
    inference.VIDTestIndex(img_index).videos) -> (a new list[BoxList] with "track_ids", the track table); see the module
    docstring for the definition."""
    r = run(predictions, videos, score_thresh, link_iou, max_gap, min_len, rescore, device)
    return _attach(predictions, r["track_ids"], r["scores"] if rescore is not None else None,
                   r["packed"]["counts"]), r["table"]


def format_table(table, classes=None):
    """The text of tracks.txt, one line per track: video, id, class name, first frame, last frame, box count, mean score.
    classes: names by label (default vid_eval.CLASSES); a label outside it is written as its number."""
    classes = vid_eval.CLASSES if classes is None else classes
    s = ""
    for r in table:
        lab = int(r["label"])
        name = classes[lab] if 0 <= lab < len(classes) else str(lab)
        s += "{:d} {:d} {} {:d} {:d} {:d} {:.6f}\n".format(int(r["video"]), int(r["id"]), name, int(r["first"]),
                                                            int(r["last"]), int(r["count"]), float(r["mean"]))
    return s
