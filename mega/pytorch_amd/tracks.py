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


Refinement (refine): filling a track's gap frames by interpolation and smoothing its boxes along the track.  The reference
has no counterpart either; this section defines it, and the kernel (csrc/track_refine.hip) and the test twin
(tests/track_refine_twin.py) implement it.

Input: predictions, a list[BoxList] in dataset order with "scores" (f32, >= 0, not NaN), "labels" (int >= 0) and
"track_ids" (int64, -1 = in no track) -- what link returns or predictions_tracks.pth holds -- and optionally "filled"
(uint8), so that refining twice is defined; videos as for link.

Parameters:
    fill       = True    bool
    smooth     = 0       int radius r, 0 <= r <= 64 (a bool is not accepted)
    fill_scale = 1.0     rounded to f32; must lie in (0, 1]

Track: all boxes of one video with the same track id >= 0.  Boxes with id -1 are never touched; where fill is off, neither
is a box that the smoothing does not reach.

Host checks, each a ValueError with the prefix "tracks:" before any device work: a missing "track_ids" field or an id
< -1; two boxes of one track in the same frame; a track with more than one label; a non-finite box; a NaN or negative
score, a negative label (flat.pack's checks); frames of one video with different size or mode; with fill a field other
than "scores", "labels", "track_ids", "filled" (a filled box has no value for it); an output of more than 2^31 - 1
boxes; the parameter ranges above.

Filling (fill = True).  For consecutive members a, b of a track at frames fa < fb with fb - fa > 1, every frame f with
fa < f < fb gets one new box.  Per coordinate, in f32, in this order, with no FMA contraction:
    w = f32(f - fa) / f32(fb - fa)
    c = a.c + (b.c - a.c) * w
Its score is min(a.score, b.score) * fill_scale, one f32 multiply (a -0.0 score counts as +0.0); its label and track id are
the track's; its "filled" is 1.  A filled box lies in the convex hull of two boxes of the same image size, so no clipping
is defined.

Smoothing (r > 0) runs after filling and reads only unsmoothed values.  It applies to every box s of a track, filled boxes
included: take the track's boxes s' with |frame(s') - frame(s)| <= r (the window is cut at the track's first and last
frame; with fill = False it holds only the boxes that exist); per coordinate, their f32 values are added in f64 in
ascending frame order, starting from the first of them, the sum is divided by their count in f64 and rounded once to f32.
Scores, labels and ids do not change.  A track of one box is unchanged, bit for bit.

Output: a new list[BoxList] of the same length, sizes and modes.  In every frame the input boxes come first, in their input
order, with all fields bit for bit -- only the bbox of smoothed members changes -- then the frame's filled boxes by
ascending track id.  The field "filled" (uint8) is always present: the input's own value where it carried one, else 0 for
input boxes.  refine also returns {"tracks": K, "filled": n_new}.  Refining a refined list with smooth = 0 adds nothing and
changes no bit.  DETECTIONS_PER_IMG is not re-applied.

There is no CPU path here either.  The host checks order the members by (video, track id, frame) and so know every track's
members m_off[K + 1] and output slots o_off[K + 1] (last - first + 1 frames with fill, the member count without); the
kernel fills and smooths one tile of 256 slots per workgroup; the results go back to their frames with a few torch
operations on the device and one copy.
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


# ------------------------------------------------------------------------------------------------ refinement
REFINE_FIELDS = ("scores", "labels", "track_ids", "filled")
MAX_SMOOTH = 64


def check_refine_params(fill=True, smooth=0, fill_scale=1.0):
    """-> (fill, smooth, fill_scale rounded to f32 as a Python float); ValueError for a bad value."""
    if not isinstance(fill, (bool, np.bool_)):
        raise ValueError("tracks: fill must be a bool, got %r" % (fill,))
    if isinstance(smooth, (bool, np.bool_)) or not isinstance(smooth, (int, np.integer)) or not 0 <= smooth <= MAX_SMOOTH:
        raise ValueError("tracks: smooth must be an int in [0, %d], got %r" % (MAX_SMOOTH, smooth))
    try:
        scale = float(np.float32(fill_scale))
    except (TypeError, ValueError):
        raise ValueError("tracks: fill_scale must be a number in (0, 1], got %r" % (fill_scale,))
    if isinstance(fill_scale, (bool, np.bool_)) or not 0.0 < scale <= 1.0:
        raise ValueError("tracks: fill_scale must lie in (0, 1] (in f32), got %r" % (fill_scale,))
    return bool(fill), int(smooth), scale


def _refine_pack(predictions, videos, fill):
    """The host checks of refine and what they compute on the way: flat.pack's dict plus "track_ids" [N] i64, "order" [M] i64
    (the members' flat positions by (video, track id, frame)), "frame" [M] (their frames, in that order), "m_off" / "o_off"
    [K+1] i64, "track_id" / "track_label" [K] i64, "K", "M", "S" (slots) and "n_new" (S - M)."""
    for f, p in enumerate(predictions):
        if not p.has_field("track_ids"):
            raise ValueError("tracks: refine needs the field \"track_ids\" (tracks.link's output); frame %d has none" % f)
        extra = sorted(set(p.fields()) - set(REFINE_FIELDS))
        if fill and extra:
            raise ValueError("tracks: fill=True cannot give a filled box a value for the field(s) %s (frame %d)"
                             % (", ".join(extra), f))
        if p.get_field("track_ids").numel() != len(p):
            raise ValueError("tracks: frame %d has %d boxes and %d track ids" % (f, len(p), p.get_field("track_ids").numel()))
    pk = flat.pack(predictions, videos, "tracks")
    F, N, vs, vl = pk["F"], pk["N"], pk["video_start"], pk["video_len"]
    for s0, n in zip(vs.tolist(), vl.tolist()):
        for p in predictions[s0 + 1:s0 + n]:
            if tuple(p.size) != tuple(predictions[s0].size) or p.mode != predictions[s0].mode:
                raise ValueError("tracks: the frames of the video at %d differ in size or mode" % s0)
    ids = np.zeros(0, np.int64)
    if N:
        ids = torch.cat([p.get_field("track_ids").reshape(-1).to("cpu", torch.int64) for p in predictions]).numpy()
        if ids.min() < -1:
            raise ValueError("tracks: a track id is below -1")
    fid = np.repeat(np.arange(F, dtype=np.int64), pk["counts"])
    vid = np.repeat(np.arange(len(vl), dtype=np.int64), vl)[fid]
    mem = np.nonzero(ids >= 0)[0]
    # by (video, track id); the flat order is by frame, and the sort is stable: frames ascend within a track
    order = mem[np.lexsort((ids[mem], vid[mem]))]
    sv, si, sf, sl = vid[order], ids[order], fid[order], pk["labels"][order]
    same = (sv[1:] == sv[:-1]) & (si[1:] == si[:-1])
    if (same & (sf[1:] == sf[:-1])).any():
        raise ValueError("tracks: two boxes of one track in the same frame")
    if (same & (sl[1:] != sl[:-1])).any():
        raise ValueError("tracks: a track with more than one label")
    M = int(order.shape[0])
    starts = np.nonzero(np.concatenate([[True], ~same]))[0] if M else np.zeros(0, np.int64)      # each track's first member
    m_off = np.concatenate([starts, [M]]).astype(np.int64)
    K = int(starts.shape[0])
    first, last = sf[m_off[:-1]], sf[m_off[1:] - 1]
    o_off = np.zeros(K + 1, np.int64)
    o_off[1:] = np.cumsum(last - first + 1 if fill else np.diff(m_off))
    S = int(o_off[-1])
    if N + S - M > 0x7fffffff:
        raise ValueError("tracks: refine would return %d boxes: too many" % (N + S - M))
    pk.update(track_ids=ids, order=order, frame=sf, m_off=m_off, o_off=o_off, track_id=si[m_off[:-1]],
              track_label=sl[m_off[:-1]], K=K, M=M, S=S, n_new=S - M)
    return pk


def refine_run(predictions, videos, fill=True, smooth=0, fill_scale=1.0, device="cuda"):
    """The refinement as flat host arrays: {"boxes": [N,4] f32, the input boxes in frame-by-frame order (smoothed where
    they are in a track); "fill_box" [n_new,4] f32, "fill_score" [n_new] f32, "fill_frame", "fill_label", "fill_id" [n_new]
    i64: the filled boxes by frame, then track id; "tracks": K; "packed": the checked input (_refine_pack)}."""
    fill, r, scale = check_refine_params(fill, smooth, fill_scale)
    pk = _refine_pack(predictions, videos, fill)
    dev = torch.device(device)
    flat.require_hip(dev, "tracks", device)
    N, K, M, S, n_new = pk["N"], pk["K"], pk["M"], pk["S"], pk["n_new"]
    out = {"packed": pk, "tracks": K, "boxes": pk["boxes"].copy(), "fill_box": np.zeros((0, 4), np.float32),
           "fill_score": np.zeros(0, np.float32), "fill_frame": np.zeros(0, np.int64), "fill_label": np.zeros(0, np.int64),
           "fill_id": np.zeros(0, np.int64)}
    if K == 0:
        return out
    from . import ops
    with torch.cuda.device(dev):
        t = flat.upload([("box", pk["boxes"]), ("score", pk["scores"]), ("order", pk["order"]),
                         ("frame", pk["frame"].astype(np.int32)), ("m_off", pk["m_off"]), ("o_off", pk["o_off"])], dev)
        box, score, frame, track, src, _ = ops.refine_tracks(t["box"][t["order"]].contiguous(),
                                                             t["score"][t["order"]].contiguous(), t["frame"], t["m_off"],
                                                             t["o_off"], S, fill, r, scale)
        # members return to their source positions
        new_box = t["box"].clone()
        kept = torch.nonzero(src >= 0).reshape(-1)
        new_box[t["order"][src[kept].to(torch.int64)]] = box[kept]
        # the filled slots are in (video, track id, frame) order; a stable sort by frame groups them by frame with the
        # track ids ascending within it (a frame lies in one video)
        new = torch.nonzero(src < 0).reshape(-1)
        new = new[torch.sort(frame[new], stable=True).indices]
        # [boxes f32 [N,4] | fill_box f32 [n_new,4] | fill_score f32 | fill_frame i32 | fill track i32]: one copy back
        res = torch.cat([x.contiguous().view(torch.uint8).reshape(-1)
                         for x in (new_box, box[new], score[new], frame[new], track[new])])
        host = res.cpu().numpy()
    if host.shape[0] != 16 * N + 28 * n_new:
        raise RuntimeError("tracks: the refinement kernel filled %d bytes of boxes, expected %d"
                           % (host.shape[0] - 16 * N, 28 * n_new))
    o = 16 * N
    out["boxes"] = host[:o].view(np.float32).reshape(N, 4).copy()
    out["fill_box"] = host[o:o + 16 * n_new].view(np.float32).reshape(n_new, 4).copy()
    o += 16 * n_new
    out["fill_score"] = host[o:o + 4 * n_new].view(np.float32).copy()
    out["fill_frame"] = host[o + 4 * n_new:o + 8 * n_new].view(np.int32).astype(np.int64)
    k = host[o + 8 * n_new:].view(np.int32)
    out["fill_label"], out["fill_id"] = pk["track_label"][k], pk["track_id"][k]
    return out


def refine(predictions, videos, fill=True, smooth=0, fill_scale=1.0, device="cuda"):
    """Fill the gap frames of the tracks in `predictions` (list[BoxList] with "track_ids") and smooth their boxes ->
    (a new list[BoxList] with the field "filled", {"tracks": K, "filled": n_new}); see the module docstring."""
    r = refine_run(predictions, videos, fill, smooth, fill_scale, device)
    pk = r["packed"]
    off = pk["off"]
    foff = np.zeros(pk["F"] + 1, np.int64)
    foff[1:] = np.cumsum(np.bincount(r["fill_frame"], minlength=pk["F"]))
    n_new = int(foff[-1])
    boxes = torch.from_numpy(r["boxes"])
    added = {"bbox": torch.from_numpy(r["fill_box"]), "scores": torch.from_numpy(r["fill_score"]),
             "labels": torch.from_numpy(r["fill_label"]), "track_ids": torch.from_numpy(r["fill_id"]),
             "filled": torch.ones(n_new, dtype=torch.uint8)}
    out = []
    for f, p in enumerate(predictions):
        a, b = int(foff[f]), int(foff[f + 1])
        d = p.bbox.device
        bbox = boxes[int(off[f]):int(off[f + 1])]
        if b > a:
            bbox = torch.cat([bbox, added["bbox"][a:b]])
        bl = BoxList(bbox.to(d), p.size, p.mode)
        for k in p.fields():
            v = p.get_field(k)
            if b > a:              # (fill is on: the frame carries none but the four fields a filled box has a value for)
                v = torch.cat([v.reshape(-1), added[k][a:b].to(device=v.device, dtype=v.dtype)])
            bl.add_field(k, v)
        if not p.has_field("filled"):
            bl.add_field("filled", torch.cat([torch.zeros(len(p), dtype=torch.uint8), added["filled"][a:b]]).to(d))
        out.append(bl)
    return out, {"tracks": r["tracks"], "filled": n_new}


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
