"""Test helper: track-refinement cases with hand-computed answers (the refinement section of mega/pytorch_amd/tracks.py's
docstring), one per rule, shared by the twin's CPU tests and the kernel's GPU tests.  Each case: (frames, videos, kwargs,
expected frames, expected info).  Frames are track_refine_twin's dicts; an expected frame holds "box" (rows of four f32),
"score", "label", "track" and "filled", the input boxes first, then the filled ones by ascending track id.

The expected numbers are f32 literals or short float64 expressions rounded once: the sum or product of two f32 values is
exact in f64, so f32(float64 expression) is the f32 operation's result; sums of small integers are exact in f64."""
import numpy as np


def f32(x):
    return np.float32(x)


def _frame(boxes, scores, labels, tracks, filled=None):
    f = {"box": np.asarray(boxes, np.float32).reshape(-1, 4), "score": np.asarray(scores, np.float32),
         "label": np.asarray(labels, np.int64), "track": np.asarray(tracks, np.int64)}
    if filled is not None:
        f["filled"] = np.asarray(filled, np.uint8)
    return f


def _want(boxes, scores, labels, tracks, filled):
    return _frame(boxes, scores, labels, tracks, filled)


EMPTY = _frame([], [], [], [])
NONE = _want([], [], [], [], [])
W13 = f32(1.0 / 3.0)       # f32(1) / f32(3)
W23 = f32(2.0 / 3.0)       # f32(2) / f32(3)


def lerp(a, b, w):
    """a + (b - a) * w, each operation rounded to f32: b - a is a small integer here (exact), the product and the sum of two
    f32 values are exact in f64."""
    return f32(float(f32(a)) + float(f32(float(f32(b) - f32(a)) * float(w))))


def mean(*v):
    """small integers and halves: the f64 sum is exact in any order"""
    return f32(sum(float(x) for x in v) / len(v))


def cases():
    out = {}
    # one track with members in frames 0, 2 and 5: a gap of 1 (w = 1/2, exact) and a gap of 2 frames (w = 1/3, 2/3)
    a, b, c = [0, 0, 10, 10], [1, 3, 11, 13], [2, 5, 13, 20]
    gaps = [_frame([a], [0.9], [1], [0]), EMPTY, _frame([b], [0.5], [1], [0]), EMPTY, EMPTY, _frame([c], [0.7], [1], [0])]
    want = [_want([a], [0.9], [1], [0], [0]),
            _want([[0.5, 1.5, 10.5, 11.5]], [0.5], [1], [0], [1]),
            _want([b], [0.5], [1], [0], [0]),
            _want([[lerp(p, q, W13) for p, q in zip(b, c)]], [0.5], [1], [0], [1]),
            _want([[lerp(p, q, W23) for p, q in zip(b, c)]], [0.5], [1], [0], [1]),
            _want([c], [0.7], [1], [0], [0])]
    assert want[3]["box"][0].tolist() == [f32(1.0) + W13, f32(3.0) + f32(f32(2.0) * W13), f32(11.0) + f32(f32(2.0) * W13),
                                          f32(13.0) + f32(f32(7.0) * W13)]
    out["gap_1_and_gap_3"] = (gaps, [(0, 6)], {}, want, {"tracks": 1, "filled": 3})
    # the same with fill_scale = 0.5: only the filled boxes' scores change, one f32 multiply of the smaller neighbour
    half = [dict(w) for w in want]
    for t, s in ((1, 0.5), (3, 0.5), (4, 0.5)):
        half[t] = dict(half[t], score=np.asarray([f32(f32(s) * f32(0.5))], np.float32))
    out["fill_scale_half"] = (gaps, [(0, 6)], {"fill_scale": 0.5}, half, {"tracks": 1, "filled": 3})
    # fill off: nothing is added, and without smoothing nothing changes
    out["fill_off_smooth_0"] = (gaps, [(0, 6)], {"fill": False},
                                [_want(f["box"], f["score"], f["label"], f["track"], [0] * len(f["score"])) for f in gaps],
                                {"tracks": 1, "filled": 0})

    # integer-lattice motion, 2 px a frame, boxes in the even frames: the midpoints are exact integers
    lat = [_frame([[2 * t, 10 + 2 * t, 20 + 2 * t, 40 + 2 * t]], [0.9], [3], [0]) if t % 2 == 0 else EMPTY for t in range(5)]
    out["lattice_midpoints"] = (lat, [(0, 5)], {},
                                [_want([[2 * t, 10 + 2 * t, 20 + 2 * t, 40 + 2 * t]], [0.9], [3], [0], [t % 2]) for t in range(5)],
                                {"tracks": 1, "filled": 2})

    # smoothing at a track's first and last frame: x1 = 0, 3, 4, 8, 20 (the other coordinates shifted by 100, 200, 300)
    xs = [0, 3, 4, 8, 20]

    def row(x):
        return [x, x + 100, x + 200, x + 300]

    def rows(m):
        return [[f32(float(m) + k) for k in (0, 100, 200, 300)]]

    full = [_frame([row(x)], [0.8], [1], [7]) for x in xs]
    r1 = [mean(0, 3), mean(0, 3, 4), mean(3, 4, 8), mean(4, 8, 20), mean(8, 20)]
    r2 = [mean(0, 3, 4), mean(0, 3, 4, 8), mean(0, 3, 4, 8, 20), mean(3, 4, 8, 20), mean(4, 8, 20)]
    assert r1[0] == f32(1.5) and r1[4] == f32(14.0) and r2[2] == f32(7.0) and r1[1] == f32(7.0 / 3.0)
    # (a coordinate x + 100 k has the mean m + 100 k: the shifted sums are integers too; 7/3 + 100 is rounded from f64)
    out["smooth_r1_ends"] = (full, [(0, 5)], {"smooth": 1},
                             [_want([[mean(*(v + k for v in w)) for k in (0, 100, 200, 300)]], [0.8], [1], [7], [0])
                              for w in ((0, 3), (0, 3, 4), (3, 4, 8), (4, 8, 20), (8, 20))], {"tracks": 1, "filled": 0})
    out["smooth_r2_ends"] = (full, [(0, 5)], {"smooth": 2},
                             [_want([[mean(*(v + k for v in w)) for k in (0, 100, 200, 300)]], [0.8], [1], [7], [0])
                              for w in ((0, 3, 4), (0, 3, 4, 8), (0, 3, 4, 8, 20), (3, 4, 8, 20), (4, 8, 20))],
                             {"tracks": 1, "filled": 0})
    # r larger than the track: every box becomes the mean of all five, 35 / 5 = 7
    out["smooth_r_larger_than_track"] = (full, [(0, 5)], {"smooth": 64}, [_want(rows(7), [0.8], [1], [7], [0])] * 5,
                                         {"tracks": 1, "filled": 0})

    # fill off, r = 2, members in frames 0, 2, 3, 6: the windows hold only the boxes that exist --
    # frame 0: {0, 2}; frame 2: {0, 2, 3}; frame 3: {2, 3} (frames 0 and 6 are 3 away); frame 6: itself
    gx = {0: 0, 2: 6, 3: 9, 6: 30}
    sparse = [_frame([row(gx[t])], [0.6], [2], [0]) if t in gx else EMPTY for t in range(7)]
    sm = {0: mean(0, 6), 2: mean(0, 6, 9), 3: mean(6, 9), 6: f32(30)}
    assert sm[0] == f32(3.0) and sm[2] == f32(5.0) and sm[3] == f32(7.5)
    out["fill_off_r2_across_a_gap"] = (sparse, [(0, 7)], {"fill": False, "smooth": 2},
                                       [_want(rows(sm[t]), [0.6], [2], [0], [0]) if t in gx else NONE for t in range(7)],
                                       {"tracks": 1, "filled": 0})
    # the same with fill on: frames 1, 4, 5 are filled first (x1 = 3, and 9 + 21 * W13, 9 + 21 * W23 as lerp rounds them:
    # the weights are inexact), then r = 1 reads the unsmoothed boxes, filled ones included, and adds them in frame order
    def m64(*v):
        acc = np.float64(v[0])
        for x in v[1:]:
            acc = acc + np.float64(x)
        return f32(acc / np.float64(len(v)))

    def urow(t, k):
        return {0: f32(gx[0] + k), 1: f32(3 + k), 2: f32(6 + k), 3: f32(9 + k), 4: lerp(9 + k, 30 + k, W13),
                5: lerp(9 + k, 30 + k, W23), 6: f32(30 + k)}[t]
    assert urow(1, 0) == lerp(0, 6, f32(0.5)) and abs(float(urow(4, 0)) - 16.0) < 1e-5
    want = []
    for t in range(7):
        win = [s for s in (t - 1, t, t + 1) if 0 <= s <= 6]
        want.append(_want([[m64(*[urow(s, k) for s in win]) for k in (0, 100, 200, 300)]], [0.6], [2], [0],
                          [0 if t in gx else 1]))
    out["fill_then_smooth_r1"] = (sparse, [(0, 7)], {"smooth": 1}, want, {"tracks": 1, "filled": 3})

    # a track of one box is unchanged bit for bit (a -0.0 coordinate included), whatever r; so is a box with id -1
    one = [_frame([[-0.0, 1, 5, 6], [50, 50, 60, 60]], [0.4, 0.3], [1, 1], [0, -1]), _frame([[3, 3, 9, 9]], [0.2], [1], [-1])]
    out["one_box_track"] = (one, [(0, 2)], {"smooth": 2},
                            [_want(f["box"], f["score"], f["label"], f["track"], [0] * len(f["score"])) for f in one],
                            {"tracks": 1, "filled": 0})

    # two tracks of different classes interleaved in the same frames, 1000 apart: each is filled and smoothed from its own
    # boxes only; frame 1's filled boxes come by ascending track id (track 1 stands first in the input frames)
    # x moves 1 px a frame, so the unsmoothed x1 of track 0 is 0, 1, 2 (frame 1 filled); with r = 1 the means are 0.5, 1, 1.5
    two = [_frame([[1000 + t, 1000, 1010 + t, 1010], [t, 0, 10 + t, 10]], [0.9, 0.8], [2, 1], [1, 0]) if t != 1 else EMPTY
           for t in range(3)]
    out["two_classes_interleaved"] = (two, [(0, 3)], {"smooth": 1},
                                      [_want([[1000.5, 1000, 1010.5, 1010], [0.5, 0, 10.5, 10]], [0.9, 0.8], [2, 1], [1, 0], [0, 0]),
                                       _want([[1, 0, 11, 10], [1001, 1000, 1011, 1010]], [0.8, 0.9], [1, 2], [0, 1], [1, 1]),
                                       _want([[1001.5, 1000, 1011.5, 1010], [1.5, 0, 11.5, 10]], [0.9, 0.8], [2, 1], [1, 0], [0, 0])],
                                      {"tracks": 2, "filled": 2})

    # ids all -1: nothing to do
    loose = [_frame([[0, 0, 9, 9], [5, 5, 20, 20]], [0.5, 0.25], [1, 2], [-1, -1]), EMPTY, _frame([[1, 1, 8, 8]], [0.75], [1], [-1])]
    out["ids_all_minus_one"] = (loose, [(0, 3)], {"smooth": 3},
                                [_want(f["box"], f["score"], f["label"], f["track"], [0] * len(f["score"])) for f in loose],
                                {"tracks": 0, "filled": 0})

    # a video without boxes between two that have some; id 0 in the first and in the last video are two tracks, and a
    # track never reaches over a video's end
    v0 = [_frame([[0, 0, 8, 8]], [0.5], [1], [0]), EMPTY, _frame([[4, 2, 12, 10]], [0.75], [1], [0])]
    v2 = [_frame([[100, 100, 108, 108]], [0.25], [1], [0]), EMPTY, EMPTY, EMPTY, _frame([[104, 108, 116, 124]], [1.0], [1], [0])]
    want = [_want([[0, 0, 8, 8]], [0.5], [1], [0], [0]), _want([[2, 1, 10, 9]], [0.5], [1], [0], [1]),
            _want([[4, 2, 12, 10]], [0.75], [1], [0], [0]), NONE, NONE,
            _want([[100, 100, 108, 108]], [0.25], [1], [0], [0]), _want([[101, 102, 110, 112]], [0.25], [1], [0], [1]),
            _want([[102, 104, 112, 116]], [0.25], [1], [0], [1]), _want([[103, 106, 114, 120]], [0.25], [1], [0], [1]),
            _want([[104, 108, 116, 124]], [1.0], [1], [0], [0])]
    out["empty_video_between"] = (v0 + [EMPTY, EMPTY] + v2, [(0, 3), (3, 2), (5, 5)], {}, want, {"tracks": 2, "filled": 4})

    # an input "filled" field: the input's own values stay, the new boxes get 1
    again = [_frame([[0, 0, 8, 8], [30, 30, 40, 40]], [0.5, 0.5], [1, 1], [0, -1], [1, 0]), EMPTY,
             _frame([[4, 2, 12, 10]], [0.75], [1], [0], [0])]
    out["input_filled_field"] = (again, [(0, 3)], {},
                                 [_want([[0, 0, 8, 8], [30, 30, 40, 40]], [0.5, 0.5], [1, 1], [0, -1], [1, 0]),
                                  _want([[2, 1, 10, 9]], [0.5], [1], [0], [1]), _want([[4, 2, 12, 10]], [0.75], [1], [0], [0])],
                                 {"tracks": 1, "filled": 1})
    return out
