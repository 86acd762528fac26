"""Test helper: track-linking cases with hand-computed answers (mega/pytorch_amd/tracks.py's definition), one per rule,
shared by the twin's CPU tests and the kernel's GPU tests.  Each case: (frames, videos, kwargs, expected track ids per
frame, expected scores per frame (all boxes, f32), expected table rows or None).  A table row is (video, id, label, first
frame, last frame, count, mean f64).

IoUs used (the +1 convention, 10 x 10 boxes of area 100): a shift by 2 in x or y gives 80 / 120 = 0.667; by 2 in both
64 / 136 = 0.47; [0,0,9,9] against [0,0,9,7] 80 / 100, against [0,0,9,8] 90 / 100, against [0,0,9,4] 50 / 100 = 0.5."""
import numpy as np


def f32(x):
    return np.float32(x)


def _frame(boxes, scores, labels):
    return {"box": np.asarray(boxes, np.float32).reshape(-1, 4), "score": np.asarray(scores, np.float32),
            "label": np.asarray(labels, np.int64)}


EMPTY = _frame([], [], [])
BOX = [0, 0, 9, 9]
FAR = [100, 100, 109, 109]
FAR2 = [200, 200, 209, 209]


def _sum(*s):
    acc = np.float64(f32(s[0]))
    for v in s[1:]:
        acc = acc + np.float64(f32(v))
    return acc


def _mean(*s):
    return float(_sum(*s) / len(s))


def _avg(*s):
    return f32(_sum(*s) / len(s))


def _same(frames):
    """The input scores as the expected ones (no rescoring)."""
    return [[f32(s) for s in f["score"]] for f in frames]


def cases():
    out = {}
    # two objects of one class crossing: A (0.9) moves right along y = 0, B (0.8) left along y = 2, 2 pixels a frame; each
    # box has IoU 0.667 with its own track's last box and 0.47 (at the crossing, frames 2 and 3) or less with the other's.
    # B stands first in every frame, so B's root is flat index 0
    cross = [_frame([[8 - 2 * t, 2, 17 - 2 * t, 11], [2 * t, 0, 9 + 2 * t, 9]], [0.8, 0.9], [1, 1]) for t in range(5)]
    out["crossing"] = (cross, [(0, 5)], {}, [[0, 1]] * 5, _same(cross),
                       [(0, 0, 1, 0, 4, 5, _mean(*[0.8] * 5)), (0, 1, 1, 0, 4, 5, _mean(*[0.9] * 5))])
    # IoU exactly link_iou does not link (strict >); a lower threshold links the same pair
    half = [_frame([BOX], [0.6], [1]), _frame([[0, 0, 9, 4]], [0.7], [1])]
    out["iou_equal_link_iou_no_link"] = (half, [(0, 2)], {}, [[0], [1]], _same(half), None)
    out["iou_above_link_iou_links"] = (half, [(0, 2)], {"link_iou": 0.49}, [[0], [0]], _same(half), None)
    # two tracks with equal IoU (80 / 120) to one candidate: the smaller root wins.  The track of root 1 scores higher, so
    # it is opened first: the order of the track list must not decide
    tie = [_frame([[2, 0, 11, 9], [0, 2, 9, 11]], [0.5, 0.9], [1, 1]), _frame([BOX], [0.7], [1])]
    out["equal_iou_smallest_root"] = (tie, [(0, 2)], {}, [[0, 1], [0]], _same(tie), None)
    # equal scores are taken by position: position 0 (IoU 0.8) takes the only track although position 1 has IoU 1
    eqs = [_frame([BOX], [0.9], [1]), _frame([[0, 0, 9, 7], BOX], [0.5, 0.5], [1, 1])]
    out["equal_scores_by_position"] = (eqs, [(0, 2)], {}, [[0], [0, 1]], _same(eqs), None)
    # the higher-scoring candidate (position 1, IoU 0.8) takes the shared track; the other (IoU 1) opens a new one
    hi = [_frame([BOX], [0.9], [1]), _frame([BOX, [0, 0, 9, 7]], [0.4, 0.6], [1, 1])]
    out["higher_score_takes_shared_track"] = (hi, [(0, 2)], {}, [[0], [1, 0]], _same(hi), None)
    # two near-identical boxes in one frame give two tracks (a track born in t is not available in t); the next frame's
    # box joins the one with the larger IoU
    twin = [_frame([BOX, [0, 0, 9, 8]], [0.9, 0.8], [1, 1]), _frame([BOX], [0.7], [1])]
    out["born_in_frame_not_available"] = (twin, [(0, 2)], {}, [[0, 1], [0]], _same(twin), None)
    # max_gap: 1 bridges one missing frame and not two; 0 bridges none; 2 bridges two
    one = [_frame([BOX], [0.9], [1]), EMPTY, _frame([BOX], [0.8], [1])]
    two = [_frame([BOX], [0.9], [1]), EMPTY, EMPTY, _frame([BOX], [0.8], [1])]
    out["max_gap_1_bridges_one"] = (one, [(0, 3)], {"max_gap": 1}, [[0], [], [0]], _same(one),
                                    [(0, 0, 1, 0, 2, 2, _mean(0.9, 0.8))])
    out["max_gap_1_not_two"] = (two, [(0, 4)], {"max_gap": 1}, [[0], [], [], [1]], _same(two), None)
    out["max_gap_0_bridges_none"] = (one, [(0, 3)], {"max_gap": 0}, [[0], [], [1]], _same(one), None)
    out["max_gap_2_bridges_two"] = (two, [(0, 4)], {"max_gap": 2}, [[0], [], [], [0]], _same(two), None)
    # a box below score_thresh gets -1 and does not bridge
    low = [_frame([BOX], [0.9], [1]), _frame([BOX], [0.01], [1]), _frame([BOX], [0.8], [1])]
    out["below_thresh_no_track_no_bridge"] = (low, [(0, 3)], {"max_gap": 0}, [[0], [-1], [1]], _same(low), None)
    # a score equal to score_thresh takes part (>=)
    eq = [_frame([BOX], [0.9], [1]), _frame([BOX], [0.05], [1])]
    out["score_equal_thresh_takes_part"] = (eq, [(0, 2)], {}, [[0], [0]], _same(eq), None)
    # classes do not link; a video boundary does not link (each video numbers from 0)
    cl = [_frame([BOX], [0.9], [1]), _frame([BOX], [0.8], [2])]
    out["classes_do_not_link"] = (cl, [(0, 2)], {}, [[0], [1]], _same(cl), None)
    vb = [_frame([BOX], [0.9], [1]), _frame([BOX], [0.8], [1])]
    out["video_boundary"] = (vb, [(0, 1), (1, 1)], {}, [[0], [0]], _same(vb),
                             [(0, 0, 1, 0, 0, 1, _mean(0.9)), (1, 0, 1, 0, 0, 1, _mean(0.8))])
    # min_len 2 drops the one-box track of flat index 0; the rest are renumbered 0, 1 by root (flat 1: A, flat 3: C)
    ml = [_frame([FAR, BOX], [0.8, 0.9], [1, 1]), _frame([BOX, FAR2], [0.9, 0.6], [1, 1]),
          _frame([FAR2, BOX], [0.6, 0.9], [1, 1])]
    out["min_len_drops_and_renumbers"] = (ml, [(0, 3)], {"min_len": 2, "max_gap": 0}, [[-1, 0], [0, 1], [1, 0]],
                                          _same(ml), [(0, 0, 1, 0, 2, 3, _mean(0.9, 0.9, 0.9)),
                                                      (0, 1, 1, 1, 2, 2, _mean(0.6, 0.6))])
    out["min_len_1_numbers_all"] = (ml, [(0, 3)], {"max_gap": 0}, [[0, 1], [1, 2], [2, 1]], _same(ml), None)
    # ids order by root across classes (the class-major task order must not show)
    ac = [_frame([BOX, FAR, FAR2], [0.9, 0.8, 0.7], [5, 2, 5]), _frame([FAR, FAR2], [0.8, 0.7], [2, 5])]
    out["ids_by_root_across_classes"] = (ac, [(0, 2)], {}, [[0, 1, 2], [1, 2]], _same(ac),
                                         [(0, 0, 5, 0, 0, 1, _mean(0.9)), (0, 1, 2, 0, 1, 2, _mean(0.8, 0.8)),
                                          (0, 2, 5, 0, 1, 2, _mean(0.7, 0.7))])
    # rescoring: the 3-box chain gets f32((0.9f + 0.1f + 0.8f) / 3) in f64, or 0.9f; the one-box track (min_len 2) and the
    # box below score_thresh keep their scores and get -1
    rs = [_frame([BOX, FAR], [0.9, 0.3], [1, 1]), _frame([BOX, BOX], [0.1, 0.01], [1, 1]), _frame([BOX], [0.8], [1])]
    a = _avg(0.9, 0.1, 0.8)
    out["rescore_avg"] = (rs, [(0, 3)], {"min_len": 2, "rescore": "avg"}, [[0, -1], [0, -1], [0]],
                          [[a, f32(0.3)], [a, f32(0.01)], [a]], [(0, 0, 1, 0, 2, 3, _mean(0.9, 0.1, 0.8))])
    out["rescore_max"] = (rs, [(0, 3)], {"min_len": 2, "rescore": "max"}, [[0, -1], [0, -1], [0]],
                          [[f32(0.9), f32(0.3)], [f32(0.9), f32(0.01)], [f32(0.9)]],
                          [(0, 0, 1, 0, 2, 3, _mean(0.9, 0.1, 0.8))])
    # a NaN IoU ([5,5,4,4] has area 0: 0 / 0 against itself) never links, not even at link_iou 0
    nan = [_frame([[5, 5, 4, 4]], [0.9], [1]), _frame([[5, 5, 4, 4]], [0.8], [1])]
    out["nan_iou_never_links"] = (nan, [(0, 2)], {"link_iou": 0.0}, [[0], [1]], _same(nan), None)
    # an IoU of 0 does not link at link_iou 0 either (strict >)
    zero = [_frame([BOX], [0.9], [1]), _frame([FAR], [0.8], [1])]
    out["iou_zero_no_link_at_zero"] = (zero, [(0, 2)], {"link_iou": 0.0}, [[0], [1]], _same(zero), None)
    # empty frames, an empty video, no boxes at all, no frames at all
    ev = [EMPTY, _frame([BOX], [0.9], [1]), EMPTY, _frame([BOX], [0.8], [1])]
    out["empty_frames_and_video"] = (ev, [(0, 2), (2, 0), (2, 2)], {}, [[], [0], [], [0]], _same(ev),
                                     [(0, 0, 1, 1, 1, 1, _mean(0.9)), (2, 0, 1, 1, 1, 1, _mean(0.8))])
    out["no_boxes"] = ([EMPTY, EMPTY], [(0, 2)], {"rescore": "avg"}, [[], []], [[], []], [])
    out["no_frames"] = ([], [], {}, [], [], [])
    return out
