"""Motion IoU: the table motion-specific AP ("fast" / "medium" / "slow", vid_eval.evaluate_detections) needs, derived from
the annotations' tracks instead of read from vid_groundtruth_motion_iou.mat -- for a subset of videos, a re-split, another
VID-style dataset or anyone who has only the annotations.  A motion IoU is FGFA's quantity: the mean IoU of an object
with its own boxes in the +-10 neighbouring frames.

The reference has no generator (it ships the file); this docstring defines the values, and the kernel
(csrc/motion_iou.hip) and the test twin (tests/motion_iou_twin.py) implement this definition.  Agreement with the
published file is not claimed: its generator, IoU convention and treatment of lone boxes are not in the reference
(compare() and tools/make_motion_iou.py --compare measure it for whoever has the dataset).

Inputs.  groundtruth: a vid_eval.VIDTrackGroundTruth (boxes [G,4] f32, off [F+1], track_ids [G]).  videos: as for
tracks.link, (start, length) pairs or VIDTestIndex.videos records that partition the F frames.  window W: an int,
1 <= W <= 64, default 10.

Neighbours.  Box b lies in frame f of video v and has track id t.  Its neighbours are the boxes with track id t in the
frames f + d of the same video, d = -W .. -1, +1 .. +W, by dataset position; frames outside the video do not exist.
Track ids are per video (every VID video starts at 0): nothing links across a video boundary.

Pair IoU.  Exactly the detection AP's IoU of a detection that coincides with b, against the neighbour's GT box g: b gets
+1 on x2 / y2 (b'), then csrc/box_math.h's vid_iou(b', box_area1(b'), g) -- g gets its own +1, then area, intersection and
union in the +1 convention, in f32, no FMA contraction.  No rescale: one video has one frame size.

Value.  An f64: the neighbours' f32 IoUs, added in f64 in ascending d (-W first), divided by their count in f64.  A box
without any neighbour gets 0.0: that is how the reference reads an empty cell of the file (vid_eval.py:135), and 0.0 lies
in "all" and "fast".  A NaN pair IoU (a degenerate box: 0 / 0) makes the value the quiet NaN 0x7ff8000000000000; NaN lies
outside every range, as a NaN entry of a loaded file does in vid_eval today.

Result.  values [G] f64 and counts [G] i32 (the neighbours found), flat like groundtruth.boxes: run().  derive() gives
vid_eval.load_motion_iou's layout, one f64 array per frame; a frame without GT boxes holds the single entry 0.0, which is
what load_motion_iou returns for such a frame of the file -- so vid_eval.empty_weights, and with it the AP, equal what the
reference's evaluation computes from the .mat save_mat() writes.

Host checks (ValueError with the prefix "motion_iou:", before any device work): a window that is no int in 1 .. 64;
videos that do not partition the frames; a ground truth without track_ids; two boxes of one frame with the same track
id; a non-finite box; a frame with more than vid_eval.MAX_GT_PER_FRAME boxes.

There is no CPU path: one wave64 per frame computes the frame's (box, offset) pair IoUs and one lane per box adds them
(csrc/motion_iou.hip).
"""
import numpy as np
import torch

from . import flat, vid_eval

WINDOW = 10
MAX_WINDOW = 64
LDS_PAIRS = 2048            # csrc/motion_iou.hip MI_LDS_PAIRS: a frame's boxes x 2W beyond this live in the workspace
NAN = np.array([0x7ff8000000000000], np.uint64).view(np.float64)[0]


def check_window(window=WINDOW):
    """-> the window as an int; ValueError for a bad value."""
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or not 1 <= window <= MAX_WINDOW:
        raise ValueError("motion_iou: window must be an int in 1 .. %d, got %r" % (MAX_WINDOW, window))
    return int(window)


def _pack(groundtruth, videos, window):
    """The host checks -> (W, [(name, ndarray)] for flat.upload, the most boxes of a frame)."""
    W = check_window(window)
    if not hasattr(groundtruth, "track_ids"):
        raise ValueError("motion_iou: the ground truth carries no track ids (use vid_eval.VIDTrackGroundTruth)")
    F = len(groundtruth)
    off = np.ascontiguousarray(groundtruth.off, np.int64)
    boxes = np.ascontiguousarray(groundtruth.boxes, np.float32).reshape(-1, 4)
    tid = np.ascontiguousarray(groundtruth.track_ids, np.int64).reshape(-1)
    G = int(off[-1])
    if off[0] != 0 or (np.diff(off) < 0).any() or boxes.shape[0] != G or tid.shape[0] != G:
        raise ValueError("motion_iou: %d GT boxes, %d track ids, offsets ending at %d" % (boxes.shape[0], tid.shape[0], G))
    vs, vl = flat.video_ranges(videos, F, "motion_iou")
    if not np.isfinite(boxes).all():
        raise ValueError("motion_iou: a GT box is not finite")
    gcount = np.diff(off)
    max_gt = int(gcount.max()) if F else 0
    if max_gt > vid_eval.MAX_GT_PER_FRAME:
        raise ValueError("motion_iou: a frame holds %d GT boxes (at most %d)" % (max_gt, vid_eval.MAX_GT_PER_FRAME))
    if G > 0x7fffffff or F >= 0x7fffffff:
        raise ValueError("motion_iou: %d boxes in %d frames: too many" % (G, F))
    fid = np.repeat(np.arange(F, dtype=np.int64), gcount)
    o = np.lexsort((tid, fid))
    same = (fid[o][1:] == fid[o][:-1]) & (tid[o][1:] == tid[o][:-1])
    if same.any():
        i = int(o[1:][same][0])
        raise ValueError("motion_iou: frame %d holds two boxes with the track id %d" % (fid[i], tid[i]))
    parts = [("box", boxes), ("track", tid), ("off", off), ("v0", np.repeat(vs, vl).astype(np.int32)),
             ("v1", np.repeat(vs + vl, vl).astype(np.int32))]
    return W, parts, max_gt


def run(groundtruth, videos, window=WINDOW, device="cuda"):
    """-> (values [G] f64, counts [G] i32), host arrays, flat like groundtruth.boxes; see the module docstring."""
    W, parts, max_gt = _pack(groundtruth, videos, window)
    dev = torch.device(device)
    flat.require_hip(dev, "motion_iou", device)
    from . import ops
    with torch.cuda.device(dev):
        t = flat.upload(parts, dev)
        values, counts = ops.motion_iou(t["box"], t["track"], t["off"], t["v0"], t["v1"], W, max_gt)
        values, counts = values.cpu().numpy(), counts.cpu().numpy()
    if counts.size and counts.min() < 0:
        raise RuntimeError("motion_iou: the kernel skipped a frame (its offsets do not fit the arrays)")
    return values, counts


def to_per_frame(values, off):
    """Flat values [G] -> vid_eval.load_motion_iou's layout: one f64 array per frame, the single entry 0.0 for a frame
    without GT boxes."""
    values = np.asarray(values, np.float64)
    return [values[s:e].copy() if e > s else np.zeros(1, np.float64) for s, e in zip(off[:-1], off[1:])]


def derive(groundtruth, videos, window=WINDOW, device="cuda"):
    """The motion IoU table of `groundtruth` -> list, one f64 array per frame: what evaluate_detections(motion_iou=...)
    takes in place of vid_eval.load_motion_iou's lists."""
    values, _ = run(groundtruth, videos, window, device)
    return to_per_frame(values, np.asarray(groundtruth.off, np.int64))


def save_mat(path, per_frame, off=None):
    """Writes per-frame motion IoUs as the `motion_iou` cell array of vid_groundtruth_motion_iou.mat: [F x 1] cells, frame
    i an [n x 1] f64 column and a frame without GT boxes [1 x 0] -- both vid_eval.load_motion_iou and the reference's own
    expression (vid_eval.py:135-137) read the values back bit for bit, an empty frame as one 0.  off: the ground truth's
    frame offsets [F+1]; with them a frame without GT boxes is written [1 x 0], as is every empty entry; without them
    derive()'s lone 0.0 of such a frame is written as the one value it reads back as."""
    import scipy.io as sio
    cells = np.empty((len(per_frame), 1), dtype=object)
    if off is not None and len(off) != len(per_frame) + 1:
        raise ValueError("motion_iou: %d frames, %d offsets" % (len(per_frame), len(off)))
    for i, m in enumerate(per_frame):
        m = np.asarray(m, np.float64).reshape(-1)
        if m.size == 0 or (off is not None and off[i + 1] == off[i]):
            cells[i, 0] = np.zeros((1, 0), np.float64)
        else:
            cells[i, 0] = m.reshape(-1, 1)
    sio.savemat(path, {"motion_iou": cells})


def _range_index(v, ranges):
    """The set of ranges (a bit per range) each value lies in: NaN lies in none."""
    v = np.asarray(v, np.float64)
    bits = np.zeros(v.shape, np.int64)
    for i, (lo, hi) in enumerate(ranges):
        bits |= ((v >= lo) & (v <= hi)).astype(np.int64) << i
    return bits


def compare(per_frame_a, per_frame_b, ranges=None):
    """Two per-frame tables of the same frames -> {"frames", "entries" (of the frames whose entry counts agree),
    "count_mismatch": the frames whose entry counts differ, "max_abs_diff", "median_abs_diff" (over those entries; a NaN
    on one side only counts as inf, on both as 0), "range_changed": the share of those entries that lie in a different
    set of `ranges` (default vid_eval.MOTION_RANGES[1:], fast / medium / slow)}."""
    ranges = vid_eval.MOTION_RANGES[1:] if ranges is None else ranges
    if len(per_frame_a) != len(per_frame_b):
        raise ValueError("motion_iou: the tables cover %d and %d frames" % (len(per_frame_a), len(per_frame_b)))
    bad, a, b = [], [], []
    for i, (x, y) in enumerate(zip(per_frame_a, per_frame_b)):
        x, y = np.asarray(x, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
        if x.size != y.size:
            bad.append(i)
        else:
            a.append(x)
            b.append(y)
    a = np.concatenate(a) if a else np.zeros(0)
    b = np.concatenate(b) if b else np.zeros(0)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
    d[np.isnan(a) != np.isnan(b)] = np.inf
    d[np.isnan(a) & np.isnan(b)] = 0.0
    changed = _range_index(a, ranges) != _range_index(b, ranges)
    return {"frames": len(per_frame_a), "entries": int(a.size), "count_mismatch": bad,
            "max_abs_diff": float(d.max()) if d.size else 0.0, "median_abs_diff": float(np.median(d)) if d.size else 0.0,
            "range_changed": float(changed.mean()) if changed.size else 0.0}


def check_request(motion_iou, anno_path):
    """inference(motion_iou=...)'s value -> the window when it asks for a derived table ("derive" or {"derive": True,
    "window": N}), None for everything else (None, a path, lists); ValueError for a bad request."""
    if isinstance(motion_iou, dict):
        if sorted(set(motion_iou) - {"derive", "window"}) or motion_iou.get("derive") is not True:
            raise ValueError("motion_iou: a dict must be {\"derive\": True, \"window\": N}, got %r" % (motion_iou,))
        window = check_window(motion_iou.get("window", WINDOW))
    elif isinstance(motion_iou, str) and motion_iou == "derive":
        window = WINDOW
    else:
        return None
    if anno_path is None:
        raise ValueError("motion_iou: deriving the table needs anno_path (the annotations carry the tracks)")
    return window


def resolve(motion_iou, img_index, anno_path, device="cuda", cache=None):
    """inference(motion_iou=...)'s value -> (per-frame lists or None, the VIDTrackGroundTruth they were derived from or
    None).  None, a path or lists behave as ever; a request (check_request) derives the table from the annotations."""
    window = check_request(motion_iou, anno_path)
    if window is None:
        return (vid_eval.load_motion_iou(motion_iou) if isinstance(motion_iou, str) else motion_iou), None
    from .inference import VIDTestIndex
    gt = vid_eval.VIDTrackGroundTruth(img_index, anno_path, cache=cache)
    return derive(gt, VIDTestIndex(img_index).videos, window, device), gt


