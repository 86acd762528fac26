"""A list[BoxList] as flat arrays: what VID evaluation, proposal recall, Seq-NMS and track linking share before their
kernels run -- the predictions as flat host arrays and one host-to-device copy, each box's frame, the (segment, score)
order as two stable sorts, and the video layer of Seq-NMS and tracks (checked input, (class, frame) segments, the
(class, video) task table).  Error texts carry the caller's prefix; the torch ops run on any device."""
import numpy as np
import torch


def concat_predictions(predictions, fields=("scores", "labels")):
    """A list[BoxList] as flat host arrays: counts [F] i64, off [F+1] i64 (frame f's boxes are off[f] .. off[f+1]),
    boxes [N,4] f32, then one [N] array per name in `fields` (i64 for "labels", f32 otherwise)."""
    F = len(predictions)
    counts = np.fromiter((len(p) for p in predictions), dtype=np.int64, count=F)
    off = np.zeros(F + 1, np.int64)
    off[1:] = np.cumsum(counts)
    dts = [(torch.int64, np.int64) if name == "labels" else (torch.float32, np.float32) for name in fields]
    if off[-1]:
        boxes = torch.cat([p.bbox.reshape(-1, 4).to("cpu", torch.float32) for p in predictions]).numpy()
        vals = [torch.cat([p.get_field(name).reshape(-1).to("cpu", dt[0]) for p in predictions]).numpy()
                for name, dt in zip(fields, dts)]
    else:
        boxes, vals = np.zeros((0, 4), np.float32), [np.zeros(0, dt[1]) for dt in dts]
    return (counts, off, boxes) + tuple(vals)


def one_buffer(parts):
    """[(name, ndarray)] -> (one u8 host buffer, 16-byte aligned, [(name, dtype, shape, byte offset)]) for a single
    host-to-device copy; device_views() cuts the copied buffer back into tensors."""
    layout, off = [], 0
    for name, a in parts:
        a = np.ascontiguousarray(a)
        layout.append((name, a, off))
        off += (a.nbytes + 15) // 16 * 16
    buf = np.empty(max(off, 16), np.uint8)
    for name, a, o in layout:
        buf[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    return buf, [(name, a.dtype, a.shape, o) for name, a, o in layout]


def _torch_dtype(dt):
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32,
            np.dtype(np.int64): torch.int64, np.dtype(np.uint8): torch.uint8}[np.dtype(dt)]


def device_views(dbuf, layout):
    t = {}
    for name, dt, shape, o in layout:
        n = int(np.prod(shape))
        t[name] = dbuf[o:o + n * np.dtype(dt).itemsize].view(_torch_dtype(dt)).reshape(shape)
    return t


def upload(parts, dev):
    """one_buffer + the copy to `dev` + device_views: {name: tensor}."""
    buf, layout = one_buffer(parts)
    return device_views(torch.from_numpy(buf).to(dev), layout)


def frame_ids(counts, dev, N=None):
    """[N] i64 on dev: every box's frame.  counts [F]: a host array, or a tensor on dev with N (their sum: no sync)."""
    if not torch.is_tensor(counts):
        N = int(np.sum(counts))
        counts = torch.from_numpy(np.ascontiguousarray(counts, np.int64)).to(dev)
    return torch.repeat_interleave(torch.arange(counts.shape[0], device=dev), counts, output_size=N)


def segment_order(score, key, start=None):
    """The permutation into (key ascending, score descending) order, two stable sorts: equal scores of a segment keep
    the order they have in `start` (default: ascending position)."""
    if start is None:
        perm = torch.sort(score, descending=True, stable=True).indices
    else:
        perm = start[torch.sort(score[start], descending=True, stable=True).indices]
    return perm[torch.sort(key[perm], stable=True).indices]


# ------------------------------------------------------------------------------------------------ the video layer
def video_ranges(videos, F, prefix):
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
            raise ValueError("%s: the videos must partition the %d frames into contiguous ranges in order "
                             "(a video starts at %d, expected %d, length %d)" % (prefix, F, s, pos, n))
        pos += n
    if pos != F:
        raise ValueError("%s: the videos cover %d frames, the predictions hold %d" % (prefix, pos, F))
    return vs, vl


def pack(predictions, videos, prefix):
    """Host checks and flat arrays: dict of counts [F], off [F+1], boxes [N,4] f32, scores [N] f32 (-0 -> +0), labels [N]
    i64, video start / length [V] i64, C (classes: max label + 1)."""
    F = len(predictions)
    counts, off, boxes, scores, labels = concat_predictions(predictions)
    vs, vl = video_ranges(videos, F, prefix)
    N = int(off[-1])
    if not np.isfinite(boxes).all():
        raise ValueError("%s: a prediction box is not finite" % prefix)
    if np.isnan(scores).any() or (scores < 0).any():
        raise ValueError("%s: a prediction score is negative or NaN" % prefix)
    if N and labels.min() < 0:
        raise ValueError("%s: negative class label" % prefix)
    C = int(labels.max()) + 1 if N else 0
    if N > 0x7fffffff or C * F >= 0x7fffffff:
        raise ValueError("%s: %d boxes, %d classes x %d frames: too many" % (prefix, N, C, F))
    return {"F": F, "N": N, "C": C, "counts": counts, "off": off, "boxes": boxes, "scores": scores + np.float32(0),
            "labels": labels, "video_start": vs, "video_len": vl}


def video_tasks(pk, dev, by_score):
    """Uploads a pack()ed input (N > 0) in one copy and lays out the (video, class) tasks -> dict of "t" (device views
    "box" [N,4], "score", "label", "count" [F], "vs" / "vl" [V]), "fid" [N] (frame), "key" = label * F + fid (the box's
    (class, frame) segment), "order" [N] (into segment order; within a segment by position, or with by_score by descending
    score, equal scores by position), "seg_off" [C*F+1], "tasks" [T,3] i32 (class, first frame, frames: every (class,
    video) with a box, the most boxes first, ties by class, then video) and "V" (the number of videos)."""
    F, N, C = pk["F"], pk["N"], pk["C"]
    t = upload([("box", pk["boxes"]), ("score", pk["scores"]), ("label", pk["labels"]), ("count", pk["counts"]),
                ("vs", pk["video_start"]), ("vl", pk["video_len"])], dev)
    fid = frame_ids(t["count"], dev, N)
    key = t["label"] * F + fid
    # (a stable sort by the key alone keeps each frame's boxes in position order)
    order = segment_order(t["score"], key) if by_score else torch.sort(key, stable=True).indices
    seg_off = torch.zeros(C * F + 1, dtype=torch.int64, device=dev)
    seg_off[1:] = torch.cumsum(torch.bincount(key, minlength=C * F), 0)
    cls = torch.arange(C, device=dev)[:, None] * F
    first = seg_off[cls + t["vs"][None, :]]
    cnt = (seg_off[cls + (t["vs"] + t["vl"])[None, :]] - first).reshape(-1)
    ids = torch.nonzero(cnt > 0).reshape(-1)
    ids = ids[torch.sort(cnt[ids], descending=True, stable=True).indices]
    V = t["vs"].shape[0]
    tasks = torch.stack([ids // V, t["vs"][ids % V], t["vl"][ids % V]], 1).to(torch.int32).contiguous()
    return {"t": t, "fid": fid, "key": key, "order": order, "seg_off": seg_off, "tasks": tasks, "V": V}


def require_hip(dev, what, device):
    if dev.type != "cuda":
        raise RuntimeError("%s runs on a HIP device (no CPU path); got device %r" % (what, device))
