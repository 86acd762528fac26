"""CPU: Seq-NMS (mega/pytorch_amd/seq_nms.py) -- hand-computed answers through the numpy twin (tests/seq_nms_twin.py), the
host checks of seq_nms.seq_nms, and the new C-ABI entry points' argument checks (no GPU needed)."""
import numpy as np
import pytest
import torch

import seq_nms_cases
import seq_nms_twin
from mega.pytorch_amd import _lib, seq_nms
from mega.pytorch_amd.structures import BoxList

CASES = seq_nms_cases.cases()


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def test_hand_computed_values():
    """The expected values themselves, written out without the twin or the cases' helper."""
    f = np.float32
    want = f((np.float64(f(0.9)) + np.float64(f(0.1)) + np.float64(f(0.8))) / 3)
    assert CASES["chain_avg"][4][0][0] == want and CASES["chain_max"][4][0][0] == f(0.9)
    # the exact-threshold IoUs the cases rely on, in the stated f32 order
    one = f(1)

    def iou(a, b):
        a, b = np.asarray(a, f), np.asarray(b, f)
        aa = (a[2] - a[0] + one) * (a[3] - a[1] + one)
        ab = (b[2] - b[0] + one) * (b[3] - b[1] + one)
        w = max(min(a[2], b[2]) - max(a[0], b[0]) + one, f(0))
        h = max(min(a[3], b[3]) - max(a[1], b[1]) + one, f(0))
        return (w * h) / ((aa + ab) - w * h)
    assert iou([0, 0, 9, 9], [0, 0, 9, 4]) == f(0.5)
    assert iou([0, 0, 9, 9], [0, 0, 9, 2]) == f(0.3)
    assert iou([0, 0, 9, 9], [0, 0, 9, 3]) > f(0.3)


@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_reproduces_hand_computed_cases(name):
    frames, videos, kw, keep, scores = CASES[name]
    k, s, _ = seq_nms_twin.seq_nms(frames, videos, **kw)
    assert [a.tolist() for a in k] == keep
    assert [_bits(a[m]) for a, m in zip(s, k)] == [_bits(e) for e in scores]


def test_twin_one_frame_video_is_greedy_nms():
    """A one-frame video: greedy per-class NMS at nms_iou with strict > (distinct scores)."""
    frames, _ = seq_nms_twin.make_videos(3, n_videos=1, lengths=[40], tie_scores=False, special=False, clutter=20)
    for f in frames:
        k, s, _ = seq_nms_twin.seq_nms([f], [(0, 1)])
        box, sc, lab = f["box"], f["score"], f["label"]
        want = np.zeros(len(sc), bool)
        for c in np.unique(lab):
            idx = np.nonzero(lab == c)[0]
            idx = idx[np.argsort(-sc[idx], kind="stable")]
            alive = np.ones(len(idx), bool)
            for a in range(len(idx)):
                if not alive[a]:
                    continue
                want[idx[a]] = True
                alive[a] = False
                with np.errstate(invalid="ignore"):
                    alive &= ~(seq_nms_twin.vid_twin.iou_f32(box[idx], box[idx[a]][None])[:, 0] > np.float32(0.3))
        assert k[0].tolist() == want.tolist()
        np.testing.assert_array_equal(s[0][k[0]], sc[k[0]])


def _bl(boxes, scores, labels):
    b = BoxList(torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4), (20, 20))
    b.add_field("scores", torch.tensor(scores, dtype=torch.float32))
    b.add_field("labels", torch.tensor(labels, dtype=torch.int64))
    return b


def test_bad_input_raises_before_device_work():
    ok = [_bl([[0, 0, 9, 9]], [0.5], [1])]
    cases = [
        ([_bl([[0, 0, 9, 9]], [-0.1], [1])], [(0, 1)], {}, "negative or NaN"),
        ([_bl([[0, 0, 9, 9]], [float("nan")], [1])], [(0, 1)], {}, "negative or NaN"),
        ([_bl([[0, 0, float("inf"), 9]], [0.5], [1])], [(0, 1)], {}, "not finite"),
        ([_bl([[0, 0, float("nan"), 9]], [0.5], [1])], [(0, 1)], {}, "not finite"),
        ([_bl([[0, 0, 9, 9]], [0.5], [-1])], [(0, 1)], {}, "negative class"),
        (ok, [(0, 2)], {}, "cover"),
        (ok, [(1, 1)], {}, "partition"),
        (ok + ok, [(0, 1), (0, 1)], {}, "partition"),
        (ok + ok, [(1, 1), (0, 1)], {}, "partition"),
        (ok, [(0, 1)], {"link_iou": 1.5}, "link_iou"),
        (ok, [(0, 1)], {"nms_iou": -0.1}, "nms_iou"),
        (ok, [(0, 1)], {"nms_iou": float("nan")}, "nms_iou"),
        (ok, [(0, 1)], {"rescore": "sum"}, "rescore"),
    ]
    for preds, videos, kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            seq_nms.seq_nms(preds, videos, **kw)      # device="cuda": the checks come first
    with pytest.raises(RuntimeError, match="no CPU path"):
        seq_nms.seq_nms(ok, [(0, 1)], device="cpu")
    # VIDTestIndex.videos records are accepted as videos
    pk = seq_nms.pack(ok + ok, [{"start": 0, "seg_len": 2}])
    assert pk["N"] == 2 and pk["C"] == 2 and pk["video_len"].tolist() == [2]


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.mega_seq_nms(None, None, None, None, 1, 1, 1, 1, 0.5, 0.3, 0, None, None, None, None, 0, None) == 1
    args = [8, 8, 8, 8, 1, 1, 1, 1, 0.5, 0.3, 0, 8, 8, None, 8, 1 << 20, None]
    for i in (0, 1, 2, 3, 11, 12, 14):                  # each required pointer NULL
        a = list(args)
        a[i] = None
        assert lib.mega_seq_nms(*a) == 1
    for i in (4, 5, 6, 7):                              # T, F, C, N not positive
        a = list(args)
        a[i] = 0
        assert lib.mega_seq_nms(*a) == 1
    for i, v in ((8, 1.5), (9, -0.5), (8, float("nan"))):   # a threshold outside [0, 1]
        a = list(args)
        a[i] = v
        assert lib.mega_seq_nms(*a) == 1
    nb = lib.mega_seq_nms_workspace_bytes(1000, 31 * 50)
    assert nb >= 1000 * 12 + 31 * 50 * 16
    a = list(args)
    a[7], a[5], a[6], a[15] = 1000, 50, 31, nb - 1
    assert lib.mega_seq_nms(*a) == 3                    # workspace too small
    assert lib.mega_seq_nms_workspace_bytes(0, 10) == 0 and lib.mega_seq_nms_workspace_bytes(10, 0) == 0
