"""Test helper: a plain numpy restatement of mega/pytorch_amd/motion_iou.py's docstring -- the pair IoU term by term in
f32 (csrc/box_math.h's vid_iou on the box with +1 on x2 / y2), the f64 sum in ascending offset.  Loops, no vector
tricks: it is the thing the kernel is compared with bit for bit."""
import numpy as np

F32 = np.float32
ONE = F32(1.0)
ZERO = F32(0.0)
NAN = np.array([0x7ff8000000000000], np.uint64).view(np.float64)[0]


def _area1(b):
    return F32(F32(F32(b[2] - b[0]) + ONE) * F32(F32(b[3] - b[1]) + ONE))


def pair_iou(b, g):
    """vid_iou(b', box_area1(b'), g) with b' = b plus 1 on x2 / y2; every operation rounds to f32 on its own."""
    b, g = np.asarray(b, F32), np.asarray(g, F32)
    with np.errstate(all="ignore"):
        p = [b[0], b[1], F32(b[2] + ONE), F32(b[3] + ONE)]
        q = [g[0], g[1], F32(g[2] + ONE), F32(g[3] + ONE)]
        pa, qa = _area1(p), _area1(q)
        left, right = max(p[0], q[0]), min(p[2], q[2])
        top, bottom = max(p[1], q[1]), min(p[3], q[3])
        width = max(F32(F32(right - left) + ONE), ZERO)
        height = max(F32(F32(bottom - top) + ONE), ZERO)
        inter = F32(width * height)
        union = F32(F32(pa + qa) - inter)
        return F32(inter / union)


def run(boxes, off, track_ids, videos, window=10):
    """boxes [G,4] f32, off [F+1], track_ids [G], videos: (start, length) pairs -> (values [G] f64, counts [G] i32)."""
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    off = np.asarray(off, np.int64)
    tid = np.asarray(track_ids, np.int64)
    G = boxes.shape[0]
    values, counts = np.zeros(G, np.float64), np.zeros(G, np.int32)
    for start, length in videos:
        for f in range(start, start + length):
            for i in range(off[f], off[f + 1]):
                acc, n, nan = np.float64(0.0), 0, False
                for d in list(range(-window, 0)) + list(range(1, window + 1)):
                    fn = f + d
                    if fn < start or fn >= start + length:
                        continue
                    for m in range(off[fn], off[fn + 1]):
                        if tid[m] == tid[i]:
                            v = pair_iou(boxes[i], boxes[m])
                            nan = nan or bool(np.isnan(v))
                            with np.errstate(invalid="ignore"):
                                acc = acc + np.float64(v)
                            n += 1
                            break
                values[i] = NAN if nan else (acc / np.float64(n) if n else 0.0)
                counts[i] = n
    return values, counts


def per_frame(values, off):
    """load_motion_iou's layout: one f64 array per frame, a frame without GT boxes the single entry 0.0."""
    return [np.asarray(values[s:e], np.float64).copy() if e > s else np.zeros(1, np.float64)
            for s, e in zip(off[:-1], off[1:])]


class GroundTruth(object):
    """The attributes of a vid_eval.VIDTrackGroundTruth that motion_iou and the detection AP read."""

    def __init__(self, boxes, off, track_ids, labels=None, size=(200, 200)):
        self.boxes = np.ascontiguousarray(boxes, F32).reshape(-1, 4)
        self.off = np.ascontiguousarray(off, np.int64)
        if track_ids is not None:
            self.track_ids = np.ascontiguousarray(track_ids, np.int64)
        self.labels = np.ones(self.boxes.shape[0], np.int64) if labels is None else np.ascontiguousarray(labels, np.int64)
        F = len(self.off) - 1
        self.width = np.full(F, size[0], np.int64)
        self.height = np.full(F, size[1], np.int64)

    def __len__(self):
        return len(self.off) - 1
