"""GPU: the kernels that share csrc/box_math.h's IoU decide alike on the same pair of boxes.  Six two-box problems at the
threshold 0.5, each fed to greedy NMS (ops.nms, strict >), to Seq-NMS as a one-frame video (the lower-scored box is
suppressed iff iou > nms_iou) and to track linking as two consecutive frames (linked iff iou > link_iou), against each
other, against the numpy twins and against the decisions written out here."""
import numpy as np
import pytest
import torch

import seq_nms_twin
import tracks_twin
from mega.pytorch_amd import ops, seq_nms, tracks

pytestmark = pytest.mark.gpu
THR = 0.5
# (name, higher-scored box, the other box, iou > 0.5)
PAIRS = [
    ("identical", [10, 10, 50, 50], [10, 10, 50, 50], True),
    ("disjoint", [0, 0, 9, 9], [100, 100, 109, 109], False),
    ("touching by one pixel", [0, 0, 9, 9], [9, 0, 18, 9], False),               # +1 width 1: 10 / 190
    ("exactly at the threshold", [0, 0, 9, 9], [0, 0, 9, 4], False),             # 50 / 100, strict >
    ("well above", [0, 0, 9, 9], [0, 0, 9, 8], True),                            # 90 / 100
    ("NaN", [5, 0, 3, 9], [0, 0, 0, 9], False),          # x2 < x1 - 1: areas -10 and 10, no overlap: 0 / 0
]


def _frame(boxes, scores):
    return {"box": np.asarray(boxes, np.float32).reshape(-1, 4), "score": np.asarray(scores, np.float32),
            "label": np.full(len(scores), 3, np.int64)}


def test_nms_seq_nms_and_tracks_decide_alike(dev):
    want = [w for _, _, _, w in PAIRS]
    nms = []
    for _, a, b, _ in PAIRS:
        keep = ops.nms(torch.tensor([a, b], dtype=torch.float32, device=dev),
                       torch.tensor([0.9, 0.8], dtype=torch.float32, device=dev), THR, strict_gt=True).cpu().tolist()
        assert 0 in keep
        nms.append(1 not in keep)
    # Seq-NMS: one one-frame video per problem
    one = [_frame([a, b], [0.9, 0.8]) for _, a, b, _ in PAIRS]
    vid1 = [(i, 1) for i in range(len(PAIRS))]
    r = seq_nms.run(seq_nms_twin.to_boxlists(one), vid1, link_iou=THR, nms_iou=THR, device=dev)
    keep = r["keep"].reshape(len(PAIRS), 2)
    assert keep[:, 0].all()
    sup = (~keep[:, 1]).tolist()
    tk, _, _ = seq_nms_twin.seq_nms(one, vid1, link_iou=THR, nms_iou=THR)
    # tracks: one two-frame video per problem
    two = [_frame([x], [s]) for _, a, b, _ in PAIRS for x, s in ((a, 0.9), (b, 0.8))]
    vid2 = [(2 * i, 2) for i in range(len(PAIRS))]
    ids = tracks.run(tracks_twin.to_boxlists(two), vid2, link_iou=THR, device=dev)["track_ids"].reshape(len(PAIRS), 2)
    assert (ids[:, 0] == 0).all()
    linked = (ids[:, 1] == ids[:, 0]).tolist()
    tids, _, _ = tracks_twin.link(two, vid2, link_iou=THR)
    for i, (name, _, _, _) in enumerate(PAIRS):
        print(name, "nms", nms[i], "seq_nms", sup[i], "tracks", linked[i])
    assert nms == sup == linked == want
    assert sup == [not bool(k[1]) for k in tk]
    assert linked == [int(tids[2 * i + 1][0]) == int(tids[2 * i][0]) for i in range(len(PAIRS))]
    assert not nms[-1] and not sup[-1] and not linked[-1]               # the NaN pair does none of the three
