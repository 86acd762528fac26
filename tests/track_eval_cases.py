"""Test helper: tubelet-AP cases with hand-computed answers (mega/pytorch_amd/track_eval.py's definition), shared by the
twin's CPU tests and the kernel's GPU tests.  Each case is a dict:
  preds / gts / videos   the twin's frame dicts (tests/track_eval_twin.py)
  pairs    {(video, label): {"tubelets": track ids in rank order, "gt": GT track numbers, "hits": [P][G], "both": [P][G]}}
  match    {(video, track id): [true positive? at 1/4, 1/2, 3/4]}
  matched  {(video, track id): [GT track number or -1 at 1/4, 1/2, 3/4]}
  n_pos    {label: GT tracks}
  ap       {label: [AP at 1/4, 1/2, 3/4]} for every label with a GT track; every other label's AP is NaN.

Boxes: B = [0, 0, 8, 8] is 10 x 10 = 100 after the +1 on x2 / y2 and the IoU's own +1; against [0, 0, 8, 3] (10 x 5) the
IoU is 50 / 100 = 0.5 exactly, against [0, 0, 8, 2.99] 49.9 / 100.  Images and annotations are 200 x 200 unless stated."""
import numpy as np

from track_eval_twin import _gt, _pred

B = [0, 0, 8, 8]
FAR = [100, 100, 108, 108]
SIZE = (200, 200)
NO_P = ([], [], [], [])
NO_G = ([], [], [])


def _frames(P, G, size=SIZE, im_info=SIZE):
    """P: per frame (boxes, scores, labels, track ids); G: per frame (boxes, labels, track ids)."""
    return [_pred(*p, size=size) for p in P], [_gt(*g, im_info=im_info) for g in G]


def _case(P, G, videos, pairs, match, matched, n_pos, ap, **kw):
    preds, gts = _frames(P, G, **kw)
    return {"preds": preds, "gts": gts, "videos": videos, "pairs": pairs, "match": match, "matched": matched,
            "n_pos": n_pos, "ap": ap}


def _one(tubelets, gt, hits, both):
    return {"tubelets": tubelets, "gt": gt, "hits": hits, "both": both}


def cases():
    out = {}
    gt4 = [([B], [1], [0])] * 4
    # a perfect track: 4 of 4 frames hit, union 4
    out["perfect"] = _case([([B], [0.9], [1], [0])] * 4, gt4, [(0, 4)], {(0, 1): _one([0], [0], [[4]], [[4]])},
                           {(0, 0): [1, 1, 1]}, {(0, 0): [0, 0, 0]}, {1: 1}, {1: [1.0, 1.0, 1.0]})
    # a 9-frame GT track, the detection missing in the middle frame, linked without a gap: two 4-frame tubelets, each
    # hits 4, union 4 + 9 - 4 = 9.  4/9 >= 1/4 (16 >= 9) but not 1/2 (8 < 9): the higher-scored one takes the track at
    # 1/4 and the other is a false positive; AP there = 1 (the TP ranks first), elsewhere 0
    P = [([B], [0.9], [1], [0])] * 4 + [NO_P] + [([B], [0.8], [1], [1])] * 4
    out["split_track"] = _case(P, [([B], [1], [0])] * 9, [(0, 9)], {(0, 1): _one([0, 1], [0], [[4], [4]], [[4], [4]])},
                               {(0, 0): [1, 0, 0], (0, 1): [0, 0, 0]}, {(0, 0): [0, -1, -1], (0, 1): [-1, -1, -1]},
                               {1: 1}, {1: [1.0, 0.0, 0.0]})
    # two tubelets compete for one GT track: id 1 (0.9; 3 of the 4 frames, tIoU 3/4) goes first and takes it at every
    # threshold; id 0 (0.6; all 4 frames, tIoU 1) finds it taken
    P = [([B, B], [0.6, 0.9], [1, 1], [0, 1])] * 3 + [([B], [0.6], [1], [0])]
    out["two_compete"] = _case(P, gt4, [(0, 4)], {(0, 1): _one([1, 0], [0], [[3], [4]], [[3], [4]])},
                               {(0, 0): [0, 0, 0], (0, 1): [1, 1, 1]}, {(0, 0): [-1, -1, -1], (0, 1): [0, 0, 0]},
                               {1: 1}, {1: [1.0, 1.0, 1.0]})
    # one 2-frame tubelet over two GT tracks: id 5 (number 0; frame 0 only: 1 / (2 + 1 - 1) = 1/2) and id 7 (number 1;
    # frames 0 .. 3: 2 / (2 + 4 - 2) = 2/4): equal tIoU, the lower number; nothing reaches 3/4.  One TP of two GT tracks
    G = [([B, B], [1, 1], [7, 5])] + [([B], [1], [7])] * 3
    P = [([B], [0.9], [1], [3])] * 2 + [NO_P] * 2
    out["equal_tiou_lower_number"] = _case(P, G, [(0, 4)], {(0, 1): _one([3], [0, 1], [[1, 2]], [[1, 2]])},
                                           {(0, 3): [1, 1, 0]}, {(0, 3): [0, 0, -1]}, {1: 2}, {1: [0.5, 0.5, 0.0]})
    # tIoU exactly 1/4, 2/4, 3/4 (labels 1, 2, 3: 1, 2, 3 frames of a 4-frame GT track) and 1/3 (label 4: 1 frame of a
    # 3-frame GT track): >= holds with equality
    P, G = [], []
    for t in range(4):
        labs = [l for l in (1, 2, 3) if t < l] + ([4] if t == 0 else [])
        P.append(([B] * len(labs), [0.5] * len(labs), labs, labs))
        gl = [1, 2, 3] + ([4] if t < 3 else [])
        G.append(([B] * len(gl), gl, [10 * l for l in gl]))
    out["exact_thresholds"] = _case(
        P, G, [(0, 4)], {(0, 1): _one([1], [0], [[1]], [[1]]), (0, 2): _one([2], [1], [[2]], [[2]]),
                         (0, 3): _one([3], [2], [[3]], [[3]]), (0, 4): _one([4], [3], [[1]], [[1]])},
        {(0, 1): [1, 0, 0], (0, 2): [1, 1, 0], (0, 3): [1, 1, 1], (0, 4): [1, 0, 0]},
        {(0, 1): [0, -1, -1], (0, 2): [1, 1, -1], (0, 3): [2, 2, 2], (0, 4): [3, -1, -1]},
        {1: 1, 2: 1, 3: 1, 4: 1}, {1: [1.0, 0.0, 0.0], 2: [1.0, 1.0, 0.0], 3: [1.0, 1.0, 1.0], 4: [1.0, 0.0, 0.0]})
    # box IoU exactly 0.5 is a hit, 0.499 is none: hits 1, both 2, union 2 -> tIoU 1/2
    G = [([[0, 0, 8, 3]], [1], [0]), ([[0, 0, 8, 2.99]], [1], [0])]
    out["box_iou_at_half"] = _case([([B], [0.9], [1], [0])] * 2, G, [(0, 2)], {(0, 1): _one([0], [0], [[1]], [[2]])},
                                   {(0, 0): [1, 1, 0]}, {(0, 0): [0, 0, -1]}, {1: 1}, {1: [1.0, 1.0, 0.0]})
    # labels that differ are never paired: no task at all
    out["labels_differ"] = _case([([B], [0.9], [2], [0])] * 4, gt4, [(0, 4)], {}, {(0, 0): [0, 0, 0]},
                                 {(0, 0): [-1, -1, -1]}, {1: 1}, {1: [0.0, 0.0, 0.0]})
    # boxes with track id -1 are ignored, whatever their score and place
    out["minus_one_ignored"] = _case([([B, B, FAR], [0.99, 0.9, 0.99], [1, 1, 1], [-1, 0, -1])] * 4, gt4, [(0, 4)],
                                     {(0, 1): _one([0], [0], [[4]], [[4]])}, {(0, 0): [1, 1, 1]}, {(0, 0): [0, 0, 0]},
                                     {1: 1}, {1: [1.0, 1.0, 1.0]})
    # predictions made on a 100 x 50 image of the 200 x 200 annotation: ratios 2 and 4
    out["rescaled"] = _case([([[0, 0, 4, 2]], [0.9], [1], [0])] * 4, gt4, [(0, 4)], {(0, 1): _one([0], [0], [[4]], [[4]])},
                            {(0, 0): [1, 1, 1]}, {(0, 0): [0, 0, 0]}, {1: 1}, {1: [1.0, 1.0, 1.0]}, size=(100, 50))
    # label 3 has a GT track and no tubelet (AP 0), label 5 a tubelet and no GT track (AP NaN), label 1 both
    P = [([B, FAR], [0.9, 0.8], [1, 5], [0, 1])] * 4
    G = [([B, FAR], [1, 3], [0, 1])] * 4
    out["one_sided_labels"] = _case(P, G, [(0, 4)], {(0, 1): _one([0], [0], [[4]], [[4]])},
                                    {(0, 0): [1, 1, 1], (0, 1): [0, 0, 0]}, {(0, 0): [0, 0, 0], (0, 1): [-1, -1, -1]},
                                    {1: 1, 3: 1}, {1: [1.0, 1.0, 1.0], 3: [0.0, 0.0, 0.0]})
    # equal tubelet scores go by ascending track id, although id 1 stands first in every frame: id 0 takes the track and
    # ranks first in the label's list too (AP 1; the other order would give 1/2)
    out["equal_scores"] = _case([([B, B], [0.5, 0.5], [1, 1], [1, 0])] * 4, gt4, [(0, 4)],
                                {(0, 1): _one([0, 1], [0], [[4], [4]], [[4], [4]])},
                                {(0, 0): [1, 1, 1], (0, 1): [0, 0, 0]}, {(0, 0): [0, 0, 0], (0, 1): [-1, -1, -1]},
                                {1: 1}, {1: [1.0, 1.0, 1.0]})
    # two videos: ids and GT numbers restart; video 1's tubelet (0.95) misses its GT track and ranks before video 0's
    # true positive (0.9): precision 0, 1/2 at recall 0, 1/2 of two GT tracks -> AP 1/4
    P = [([B], [0.9], [1], [0])] * 4 + [([FAR], [0.95], [1], [0])] * 2
    G = gt4 + [([B], [1], [0])] * 2
    out["two_videos"] = _case(P, G, [(0, 4), (4, 2)],
                              {(0, 1): _one([0], [0], [[4]], [[4]]), (1, 1): _one([0], [0], [[0]], [[2]])},
                              {(0, 0): [1, 1, 1], (1, 0): [0, 0, 0]}, {(0, 0): [0, 0, 0], (1, 0): [-1, -1, -1]},
                              {1: 2}, {1: [0.25, 0.25, 0.25]})
    return out


def check(case, got):
    """Assert a run()-shaped result (the module's or the twin's) against the case's literals."""
    tub = [(int(t[0]), int(t[1])) for t in got["tubelets"]]
    assert sorted(tub) == sorted(case["match"]) and tub == sorted(tub)
    for u, key in enumerate(tub):
        assert [int(got["match"][r][u]) for r in range(3)] == case["match"][key], key
        assert [int(got["matched_gt"][r][u]) for r in range(3)] == case["matched"][key], key
    assert sorted(got["pairs"]) == sorted(case["pairs"])
    for key, want in case["pairs"].items():
        have = got["pairs"][key]
        assert list(have["tubelets"]) == want["tubelets"] and list(have["gt"]) == want["gt"], key
        assert np.asarray(have["hits"]).tolist() == want["hits"] and np.asarray(have["both"]).tolist() == want["both"], key
    n_pos = np.asarray(got["n_pos"]).tolist()
    assert {l: n for l, n in enumerate(n_pos) if n} == case["n_pos"]
    ap = np.asarray(got["ap"])
    for l in range(ap.shape[1]):
        if l in case["ap"]:
            np.testing.assert_allclose(ap[:, l], case["ap"][l], rtol=0, atol=1e-12)
        else:
            assert np.isnan(ap[:, l]).all(), l
