"""Test helper: Seq-NMS cases with hand-computed answers (mega/pytorch_amd/seq_nms.py's definition), shared by the twin's
CPU tests and the kernels' GPU tests.  Each case: (frames, videos, kwargs, expected keep per frame, expected scores of the
kept boxes per frame)."""
import numpy as np


def f32(x):
    return np.float32(x)


def _frame(boxes, scores, labels):
    return {"box": np.asarray(boxes, np.float32).reshape(-1, 4), "score": np.asarray(scores, np.float32),
            "label": np.asarray(labels, np.int64)}


EMPTY = _frame([], [], [])
BOX = [0, 0, 9, 9]


def _avg(*s):
    acc = np.float64(f32(s[0]))
    for v in s[1:]:
        acc = acc + np.float64(f32(v))
    return f32(acc / len(s))


def cases():
    out = {}
    # a 3-frame chain: every box gets f32((0.9f + 0.1f + 0.8f) / 3) in f64, or 0.9f under "max"
    chain = [_frame([BOX], [0.9], [1]), _frame([BOX], [0.1], [1]), _frame([BOX], [0.8], [1])]
    out["chain_avg"] = (chain, [(0, 3)], {}, [[True]] * 3, [[_avg(0.9, 0.1, 0.8)]] * 3)
    out["chain_max"] = (chain, [(0, 3)], {"rescore": "max"}, [[True]] * 3, [[f32(0.9)]] * 3)
    # a second, weaker overlapping track (IoU 0.9) is suppressed frame by frame
    two = [_frame([[0, 0, 9, 8], BOX], [0.5, 0.9], [1, 1]) for _ in range(3)]
    out["weaker_track"] = (two, [(0, 3)], {}, [[False, True]] * 3, [[f32(0.9)]] * 3)
    # IoU exactly 0.5 ([0,0,9,9] vs [0,0,9,4]: 50 / 100) does not link: two one-box paths keep their own scores
    half = [_frame([BOX], [0.6], [1]), _frame([[0, 0, 9, 4]], [0.7], [1])]
    out["iou_half_no_link"] = (half, [(0, 2)], {}, [[True], [True]], [[f32(0.6)], [f32(0.7)]])
    # IoU exactly f32(0.3) ([0,0,9,2]: 30 / 100) does not suppress; 40 / 100 does
    out["iou_0_3_no_suppress"] = ([_frame([BOX, [0, 0, 9, 2], [0, 0, 9, 3]], [0.9, 0.5, 0.4], [1, 1, 1])], [(0, 1)], {},
                                  [[True, True, False]], [[f32(0.9), f32(0.5)]])
    # equal boxes with different labels both survive
    out["labels_independent"] = ([_frame([BOX, BOX], [0.9, 0.8], [1, 2])], [(0, 1)], {}, [[True, True]],
                                 [[f32(0.9), f32(0.8)]])
    # no link across a video boundary
    out["video_boundary"] = ([_frame([BOX], [0.9], [1]), _frame([BOX], [0.1], [1])], [(0, 1), (1, 1)], {},
                             [[True], [True]], [[f32(0.9)], [f32(0.1)]])
    # step 1 ties: frame 1's box links to two frame-0 boxes with equal S -> P = the smaller position (0); frame 0's
    # position 1 is then suppressed by the path box (IoU 90 / 110)
    tie1 = [_frame([BOX, [1, 0, 10, 9]], [0.5, 0.5], [1, 1]), _frame([BOX], [0.5], [1])]
    out["tie_step1_smallest_position"] = (tie1, [(0, 2)], {}, [[True, False], [True]], [[f32(0.5)], [f32(0.5)]])
    # step 2 ties: S(0, A) = 0.5 = S(1, B) (B scores 0 and links to A) -> the earliest frame: path [A] first (0.5), then
    # [B] alone (0.0); the later end box would have given the path A -> B, 0.25 each
    tie2 = [_frame([BOX], [0.5], [1]), _frame([BOX], [0.0], [1])]
    out["tie_step2_earliest_frame"] = (tie2, [(0, 2)], {}, [[True], [True]], [[f32(0.5)], [f32(0.0)]])
    # step 2 ties within a frame: the smaller position wins and suppresses the other
    out["tie_step2_smallest_position"] = ([_frame([[0, 0, 9, 8], BOX], [0.5, 0.5], [1, 1])], [(0, 1)], {},
                                          [[True, False]], [[f32(0.5)]])
    # empty frames, an empty video, no boxes at all
    out["empty_frames_and_video"] = ([EMPTY, _frame([BOX], [0.9], [1]), EMPTY, _frame([BOX], [0.8], [1])],
                                     [(0, 2), (2, 0), (2, 2)], {}, [[], [True], [], [True]],
                                     [[], [f32(0.9)], [], [f32(0.8)]])
    out["no_boxes"] = ([EMPTY, EMPTY], [(0, 2)], {}, [[], []], [[], []])
    return out
