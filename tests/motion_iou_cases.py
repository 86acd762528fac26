"""Test helper: motion-IoU cases (mega/pytorch_amd/motion_iou.py's definition), shared by the twin's CPU tests and the
kernel's GPU tests.  A case is a dict: "gt" (motion_iou_twin.GroundTruth), "videos" [(start, length)], "window".

Boxes: B = [0, 0, 8, 8] is 10 x 10 = 100 after the +1 on x2 / y2 and the IoU's own +1; shifted by half its width,
[5, 0, 13, 8], the intersection is 5 x 10 = 50 and the union 150: IoU 1/3, rounded to f32."""
import numpy as np

from motion_iou_twin import GroundTruth

B = [0, 0, 8, 8]
B_HALF = [5, 0, 13, 8]


def build(videos, window=10, labels=None):
    """videos: per video a list of frames, a frame a list of (track id, box) -> a case."""
    boxes, tids, counts, ranges, pos = [], [], [], [], 0
    for frames in videos:
        ranges.append((pos, len(frames)))
        pos += len(frames)
        for fr in frames:
            counts.append(len(fr))
            for t, b in fr:
                tids.append(t)
                boxes.append(b)
    off = np.zeros(len(counts) + 1, np.int64)
    off[1:] = np.cumsum(counts)
    gt = GroundTruth(np.asarray(boxes, np.float32).reshape(-1, 4), off, np.asarray(tids, np.int64), labels=labels)
    return {"gt": gt, "videos": ranges, "window": window}


def _moving(t, k, step=3.0):
    """Track k's box in frame t: a 40 x 30 box that moves by `step` pixels a frame (k sets the lane and the speed)."""
    x, y = 5.0 + step * (k + 1) * t, 10.0 + 35.0 * k
    return [x, y, x + 40.0, y + 30.0]


def random_videos(seed, n_videos=6, max_len=40, max_tracks=5, presence=0.7):
    """Ragged random videos: 1 .. max_len frames, 1 .. max_tracks tracks each present in a frame with probability
    `presence`, integer-jittered moving boxes, the frame's boxes in a random order."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_videos):
        L, K = int(rng.integers(1, max_len + 1)), int(rng.integers(1, max_tracks + 1))
        frames = []
        for t in range(L):
            fr = []
            for k in range(K):
                if rng.random() < presence:
                    b = np.asarray(_moving(t, k, step=float(rng.integers(0, 6)))) + rng.integers(-3, 4, 4)
                    fr.append((k, [float(b[0]), float(b[1]), float(b[2] + 6), float(b[3] + 6)]))
            fr = [fr[i] for i in rng.permutation(len(fr))]
            frames.append(fr)
        out.append(frames)
    return out


def cases():
    out = {}
    # (a) one video of one frame: no neighbour frame exists
    out["a_one_frame"] = build([[[(0, B), (1, B_HALF)]]])
    # (b) two adjacent videos whose track ids both start at 0, overlapping boxes: a link across the boundary would
    # change every value near it
    out["b_adjacent_videos"] = build([[[(0, _moving(t, 0))] for t in range(3)], [[(0, _moving(t + 1, 0))] for t in range(4)]])
    # (c) a track with gaps (frames 0, 1, 4, 5, 9) beside a full one, and frame 3 without any GT
    frames = []
    for t in range(10):
        fr = [(7, _moving(t, 1))] if t != 3 else []
        if t in (0, 1, 4, 5, 9):
            fr.append((2, _moving(t, 0)))
        frames.append(fr)
    out["c_gaps_and_empty_frame"] = build([frames], window=3)
    # (d) two tracks listed in swapped order in alternate frames: matching goes by id, not by position
    out["d_swapped_order"] = build([[[(0, _moving(t, 0)), (1, _moving(t, 1, step=7.0))][::1 if t % 2 == 0 else -1]
                                     for t in range(6)]], window=2)
    # (e) W = 1, 10 and 64 on a 5-frame video: the clamp at both ends
    five = [[[(0, _moving(t, 0)), (1, _moving(t, 1))] for t in range(5)]]
    for w in (1, 10, 64):
        out["e_window_%d" % w] = build(five, window=w)
    # (f) a frame with 130 boxes of distinct ids beside 3-box neighbours: the lane stride (130 x 20 pairs, 130 boxes) and
    # the workspace path (2600 pairs > 2048)
    big = [(k, [float(3 * (k % 40)), float(20 * (k // 40)), float(3 * (k % 40) + 30), float(20 * (k // 40) + 25)])
           for k in range(130)]
    small = lambda dx: [(k, [b[0] + dx, b[1], b[2] + dx, b[3]]) for k, b in big if k in (0, 64, 129)]
    out["f_130_boxes"] = build([[small(-4.0), small(-2.0), big, small(3.0), small(5.0)]])
    # (g) six ragged random videos
    out["g_random"] = build(random_videos(11))
    # (h) G = 0: frames, no boxes
    out["h_no_boxes"] = build([[[], [], []], [[]]])
    # a degenerate box (area -96) beside a disjoint one of area +96 in the same track: union 0, IoU 0 / 0 = NaN; the track
    # beside it is not touched
    out["nan_pair"] = build([[[(0, [10, 10, 0, 20]), (1, B)], [(0, [100, 100, 106, 110]), (1, B_HALF)]]])
    return out


def motion_ranges_set():
    """GT for the end-to-end check: three tracks of one video, standing still (IoU 1: slow), drifting (medium) and
    jumping (fast), plus a lone box in a second video (0.0: fast)."""
    frames = []
    for t in range(8):
        frames.append([(0, [20, 20, 80, 70]), (1, [10 + 4 * t, 100, 90 + 4 * t, 160]), (2, [5 + 18 * t, 170, 65 + 18 * t, 199])])
    return build([frames, [[(0, [30, 30, 60, 60])]]], window=10,
                 labels=np.asarray([1, 2, 3] * 8 + [2], np.int64))
