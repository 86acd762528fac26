"""CPU: track linking (mega/pytorch_amd/tracks.py) -- hand-computed answers through the numpy twin (tests/tracks_twin.py),
the host checks of tracks.link, format_table, the new C-ABI entry points' declaration and argument checks (no GPU needed)
and the command line's option check."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import tracks_cases
import tracks_twin
from mega.pytorch_amd import _lib, tracks
from mega.pytorch_amd.structures import BoxList

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = tracks_cases.cases()


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def test_hand_computed_values():
    """The expected values themselves, written out without the twin or the cases' helpers."""
    f = np.float32
    want = f((np.float64(f(0.9)) + np.float64(f(0.1)) + np.float64(f(0.8))) / 3)
    assert CASES["rescore_avg"][4][0][0] == want and CASES["rescore_max"][4][0][0] == f(0.9)
    assert CASES["rescore_avg"][4][1][1] == f(0.01) and CASES["rescore_avg"][4][0][1] == f(0.3)
    one = f(1)

    def iou(a, b):
        a, b = np.asarray(a, f), np.asarray(b, f)
        aa = (a[2] - a[0] + one) * (a[3] - a[1] + one)
        ab = (b[2] - b[0] + one) * (b[3] - b[1] + one)
        w = max(min(a[2], b[2]) - max(a[0], b[0]) + one, f(0))
        h = max(min(a[3], b[3]) - max(a[1], b[1]) + one, f(0))
        with np.errstate(invalid="ignore"):
            return (w * h) / ((aa + ab) - w * h)
    assert iou([0, 0, 9, 9], [0, 0, 9, 4]) == f(0.5)
    assert iou([2, 0, 11, 9], [0, 0, 9, 9]) == iou([0, 2, 9, 11], [0, 0, 9, 9]) > f(0.5)      # the equal-IoU case's tie
    assert iou([4, 0, 13, 9], [6, 2, 15, 11]) < f(0.5) < iou([4, 0, 13, 9], [2, 0, 11, 9])    # the crossing
    assert np.isnan(iou([5, 5, 4, 4], [5, 5, 4, 4])) and iou([0, 0, 9, 9], [100, 100, 109, 109]) == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_reproduces_hand_computed_cases(name):
    frames, videos, kw, ids, scores, table = CASES[name]
    got_ids, got_scores, got_table = tracks_twin.link(frames, videos, **kw)
    assert [a.tolist() for a in got_ids] == ids
    assert [_bits(a) for a in got_scores] == [_bits(e) for e in scores]
    if table is not None:
        assert got_table == table


def test_twin_does_not_depend_on_the_track_list_order():
    """The same boxes with the two frame-0 scores exchanged: the tracks are opened in the other order, the ids (by root)
    and the winner of the equal-IoU tie stay."""
    frames, videos, kw, ids, _, _ = CASES["equal_iou_smallest_root"]
    swapped = [dict(frames[0], score=frames[0]["score"][::-1].copy()), frames[1]]
    assert [a.tolist() for a in tracks_twin.link(swapped, videos, **kw)[0]] == ids


def test_twin_minus_zero_counts_as_plus_zero():
    f = tracks_cases._frame
    frames = [f([tracks_cases.BOX], [0.9], [1]), f([[0, 0, 9, 7], tracks_cases.BOX], [0.0, -0.0], [1, 1])]
    ids, new, _ = tracks_twin.link(frames, [(0, 2)], score_thresh=0.0)
    assert [a.tolist() for a in ids] == [[0], [0, 1]]          # equal scores: position 0 goes first
    assert _bits(new[1]) == _bits(np.asarray([0.0, -0.0], np.float32))


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
        ([_bl([[0, 0, 9, 9]], [0.5], [-1])], [(0, 1)], {}, "negative class"),
        (ok, [(0, 2)], {}, "cover"),
        (ok, [(1, 1)], {}, "partition"),
        (ok + ok, [(1, 1), (0, 1)], {}, "partition"),
        (ok, [(0, 1)], {"link_iou": 1.5}, "link_iou"),
        (ok, [(0, 1)], {"link_iou": -0.1}, "link_iou"),
        (ok, [(0, 1)], {"link_iou": float("nan")}, "link_iou"),
        (ok, [(0, 1)], {"score_thresh": float("nan")}, "score_thresh"),
        (ok, [(0, 1)], {"max_gap": -1}, "max_gap"),
        (ok, [(0, 1)], {"max_gap": 1.5}, "max_gap"),
        (ok, [(0, 1)], {"min_len": 0}, "min_len"),
        (ok, [(0, 1)], {"min_len": True}, "min_len"),
        (ok, [(0, 1)], {"rescore": "sum"}, "rescore"),
    ]
    for preds, videos, kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            tracks.link(preds, videos, **kw)          # device="cuda": the checks come first
        with pytest.raises(ValueError, match=msg):
            tracks.run(preds, videos, **kw)
    assert tracks.check_params(0.05, 0.5, 1, 1, None) == (float(np.float32(0.05)), 0.5, 1, 1)


def test_cpu_device_is_a_runtime_error():
    ok = [_bl([[0, 0, 9, 9]], [0.5], [1])]
    with pytest.raises(RuntimeError, match="no CPU path"):
        tracks.link(ok, [(0, 1)], device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        tracks.run([], [], device="cpu")


def test_format_table():
    table = np.zeros(3, tracks.TABLE_DTYPE)
    table[0] = (0, 0, 1, 0, 4, 5, 0.8)
    table[1] = (0, 1, 30, 2, 2, 1, 1.0 / 3.0)
    table[2] = (7, 0, 99, 10, 12, 2, 0.5)
    names = ["bg"] + ["c%d" % i for i in range(1, 31)]
    assert tracks.format_table(table, names) == "0 0 c1 0 4 5 0.800000\n0 1 c30 2 2 1 0.333333\n7 0 99 10 12 2 0.500000\n"
    from mega.pytorch_amd import vid_eval
    assert tracks.format_table(table[:1]) == "0 0 %s 0 4 5 0.800000\n" % vid_eval.CLASSES[1]
    assert tracks.format_table(table[:0]) == ""


def test_entry_points_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "mega_hip.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in ("mega_link_tracks", "mega_link_tracks_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, decl), name + " is not declared in mega_hip.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["mega_link_tracks"]
    m = re.search(r"int\s+mega_link_tracks\s*\((.*?)\);", decl, flags=re.S)
    assert res is _lib.c_int and len(args) == len(m.group(1).split(","))
    assert _lib.SIGNATURES["mega_link_tracks_workspace_bytes"] == (_lib.c_size_t, [_lib.c_int, _lib.c_int])
    assert "tracks.py" in src[src.index("Linking detections into tracks"):src.index("mega_link_tracks_workspace_bytes(int")]


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    #       box score pos seg tasks T  F  C  N  thr  link gap open root cnt sum mx ws  bytes     stream
    args = [8, 8, 8, 8, 8, 1, 1, 1, 1, 0.05, 0.5, 1, 4, 8, 8, 8, 8, 8, 1 << 20, None]
    for i in (0, 1, 2, 3, 4, 13, 14, 15, 16, 17):          # each required pointer NULL with N > 0
        a = list(args)
        a[i] = None
        assert lib.mega_link_tracks(*a) == 1
    for i in (5, 6, 7, 8, 11, 12):                         # T, F, C, N, max_gap, max_open negative
        a = list(args)
        a[i] = -1
        assert lib.mega_link_tracks(*a) == 1
    for i in (6, 7, 12):                                   # F, C, max_open zero with N > 0
        a = list(args)
        a[i] = 0
        assert lib.mega_link_tracks(*a) == 1
    for i, v in ((10, 1.5), (10, -0.5), (10, float("nan")), (9, float("nan"))):     # thresholds
        a = list(args)
        a[i] = v
        assert lib.mega_link_tracks(*a) == 1
    a = list(args)
    a[8] = 1 << 31                                         # more boxes than an i32 index holds
    assert lib.mega_link_tracks(*a) == 1
    # N = 0 or T = 0: nothing to do, not an error, nothing is touched
    assert lib.mega_link_tracks(None, None, None, None, None, 0, 0, 0, 0, 0.05, 0.5, 1, 0, None, None, None, None, None, 0,
                                None) == 0
    # workspace: the status word always; 44 bytes per open track beyond the 1024 kept in LDS, per task
    small = lib.mega_link_tracks_workspace_bytes(5, 1024)
    assert 4 <= small <= 4096 and lib.mega_link_tracks_workspace_bytes(5, 1) == small
    big = lib.mega_link_tracks_workspace_bytes(5, 1024 + 1000)
    assert big >= small + 5 * 1000 * 44
    assert lib.mega_link_tracks_workspace_bytes(0, 10) == 0 and lib.mega_link_tracks_workspace_bytes(10, 0) == 0
    a = list(args)
    a[5], a[12], a[18] = 5, 1024 + 1000, big - 1
    assert lib.mega_link_tracks(*a) == 3                   # workspace too small


def test_eval_vid_rejects_tracks_with_box_only(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_vid.py"), "--predictions", "p.pth",
                        "--img-index", "i.txt", "--anno-path", "a", "--tracks", "--box-only"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 2 and b"--tracks" in r.stdout
    from mega.pytorch_amd import config, inference
    cfg = config.get_cfg("R-50")
    cfg.MODEL.RPN_ONLY = True
    with pytest.raises(ValueError, match="RPN_ONLY"):
        inference.inference(cfg, None, "nowhere", "nothing.txt", tracks=True)
