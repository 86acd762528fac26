"""CPU: derived motion IoUs (mega/pytorch_amd/motion_iou.py) -- the Python twin (tests/motion_iou_twin.py) against values
worked out by hand, every host check, save_mat read back by vid_eval.load_motion_iou and by the reference's indexing
expression, compare on a planted difference, the C-ABI entry point's argument checks (no GPU needed) and the command
line's option checks."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import motion_iou_cases
import motion_iou_twin
from mega.pytorch_amd import _lib, motion_iou, vid_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = motion_iou_cases.cases()
B, B_HALF = motion_iou_cases.B, motion_iou_cases.B_HALF


def _twin(case):
    gt = case["gt"]
    return motion_iou_twin.run(gt.boxes, gt.off, gt.track_ids, case["videos"], case["window"])


def test_pair_iou_by_hand():
    """B = [0, 0, 8, 8]: with the +1 on x2 / y2 and the IoU's own +1 it is 10 x 10.  Shifted by half its width (5) the
    intersection is (9 - 5 + 1) x 10 = 50 and the union 100 + 100 - 50 = 150: the exact rational 1/3, rounded to f32."""
    f = np.float32
    assert motion_iou_twin.pair_iou(B, B) == f(1.0)
    inter, union = Fraction(9 - 5 + 1) * Fraction(9 - 0 + 1), Fraction(100 + 100 - 50)
    assert inter / union == Fraction(1, 3)
    assert motion_iou_twin.pair_iou(B, B_HALF) == f(50.0) / f(150.0) == f(float(Fraction(1, 3)))
    assert motion_iou_twin.pair_iou(B_HALF, B) == f(50.0) / f(150.0)
    assert motion_iou_twin.pair_iou(B, [100, 100, 108, 108]) == f(0.0)
    assert np.isnan(motion_iou_twin.pair_iou([10, 10, 0, 20], [100, 100, 106, 110]))       # areas -96 and +96: 0 / 0


def test_twin_values_by_hand():
    third = np.float64(np.float32(50.0) / np.float32(150.0))
    # two identical boxes: 1.0 each, one neighbour each
    v, c = _twin(motion_iou_cases.build([[[(0, B)], [(0, B)]]]))
    assert v.tolist() == [1.0, 1.0] and c.tolist() == [1, 1] and v.dtype == np.float64 and c.dtype == np.int32
    # the half-width shift; then B, B, B_HALF: the middle box sees 1 and 1/3, added in ascending offset, / 2
    v, c = _twin(motion_iou_cases.build([[[(0, B)], [(0, B_HALF)]]]))
    assert v.tolist() == [third, third] and c.tolist() == [1, 1]
    v, c = _twin(motion_iou_cases.build([[[(0, B)], [(0, B)], [(0, B_HALF)]]]))
    assert v.tolist() == [(1.0 + third) / 2.0, (1.0 + third) / 2.0, (third + third) / 2.0] and c.tolist() == [2, 2, 2]
    # with W = 1 the first box no longer sees the third
    v, c = _twin(motion_iou_cases.build([[[(0, B)], [(0, B)], [(0, B_HALF)]]], window=1))
    assert v.tolist() == [1.0, (1.0 + third) / 2.0, third] and c.tolist() == [1, 2, 1]
    # a lone box; another track id in the next frame is no neighbour; nor is the same id in the next video
    v, c = _twin(motion_iou_cases.build([[[(0, B)], [(1, B)]], [[(0, B)]]]))
    assert v.tolist() == [0.0, 0.0, 0.0] and c.tolist() == [0, 0, 0]


def test_twin_on_the_shared_cases():
    v, c = _twin(CASES["a_one_frame"])
    assert v.tolist() == [0.0, 0.0] and c.tolist() == [0, 0]
    # (b) video 0 has 3 frames, video 1 has 4: nobody has more neighbours than its own video holds
    v, c = _twin(CASES["b_adjacent_videos"])
    assert c.tolist() == [2, 2, 2, 3, 3, 3, 3]
    one_video = motion_iou_cases.build([[[(0, motion_iou_cases._moving(t, 0))] for t in range(3)] +
                                        [[(0, motion_iou_cases._moving(t + 1, 0))] for t in range(4)]])
    v1, c1 = _twin(one_video)
    assert c1.tolist() == [6] * 7 and (v1 != v).all()         # a link across the boundary would change every value
    # (c) W = 3; track 2 lives in frames 0, 1, 4, 5, 9; frame 3 is empty
    gt = CASES["c_gaps_and_empty_frame"]["gt"]
    v, c = _twin(CASES["c_gaps_and_empty_frame"])
    assert np.diff(gt.off).tolist() == [2, 2, 1, 0, 2, 2, 1, 1, 1, 2]
    assert c[gt.track_ids == 2].tolist() == [1, 2, 2, 1, 0]
    assert c[gt.track_ids == 7].tolist() == [2, 3, 4, 5, 5, 5, 5, 4, 3]         # frame 3 holds no box of it
    # (d) by id: the same values as with both tracks listed in the same order everywhere
    v, c = _twin(CASES["d_swapped_order"])
    gt = CASES["d_swapped_order"]["gt"]
    same_order = motion_iou_cases.build([[[(0, motion_iou_cases._moving(t, 0)), (1, motion_iou_cases._moving(t, 1, step=7.0))]
                                          for t in range(6)]], window=2)
    v2, _ = _twin(same_order)
    for k in (0, 1):
        assert v[gt.track_ids == k].tolist() == v2[same_order["gt"].track_ids == k].tolist()
    assert gt.track_ids.tolist() == [0, 1, 1, 0] * 3 and len(set(v.tolist())) > 2
    # (e) the clamp: W = 10 and W = 64 see the whole 5-frame video, W = 1 only the adjacent frames
    c1, c10, c64 = (_twin(CASES["e_window_%d" % w])[1] for w in (1, 10, 64))
    assert c1.tolist() == [1, 1, 2, 2, 2, 2, 2, 2, 1, 1] and c10.tolist() == [4] * 10 == c64.tolist()
    assert _twin(CASES["e_window_10"])[0].tolist() == _twin(CASES["e_window_64"])[0].tolist()
    # (f) the 130-box frame: three of its boxes have 4 neighbours, the others none; 130 x 20 pairs do not fit LDS
    gt = CASES["f_130_boxes"]["gt"]
    v, c = _twin(CASES["f_130_boxes"])
    mid = c[gt.off[2]:gt.off[3]]
    assert len(mid) == 130 and 130 * 2 * 10 > motion_iou.LDS_PAIRS
    assert np.nonzero(mid)[0].tolist() == [0, 64, 129] and mid[[0, 64, 129]].tolist() == [4, 4, 4]
    assert v[gt.off[2] + 5] == 0.0 and 0.5 < v[gt.off[2] + 64] < 1.0
    # (h) frames, no boxes
    v, c = _twin(CASES["h_no_boxes"])
    assert v.shape == (0,) and c.shape == (0,) and len(CASES["h_no_boxes"]["gt"]) == 4
    # the NaN pair: both boxes of track 0 get the quiet NaN, track 1 its 1/3
    v, c = _twin(CASES["nan_pair"])
    assert v.view(np.uint64)[[0, 2]].tolist() == [0x7ff8000000000000] * 2 and c.tolist() == [1, 1, 1, 1]
    assert v[1] == v[3] == np.float64(np.float32(50.0) / np.float32(150.0))


def test_every_motion_range_holds_a_box():
    """The end-to-end GPU test's ground truth: slow, medium and fast each hold a box, and the lone box counts as fast."""
    case = motion_iou_cases.motion_ranges_set()
    v, c = _twin(case)
    (lo_f, hi_f), (lo_m, hi_m), (lo_s, hi_s) = vid_eval.MOTION_RANGES[1:]
    n = [int(((v >= lo) & (v <= hi)).sum()) for lo, hi in vid_eval.MOTION_RANGES]
    assert n[0] == len(v) == 25 and min(n[1:]) >= 1
    assert (v[0::3][:8] == 1.0).all() and v[-1] == 0.0 and c[-1] == 0
    assert ((v[1:24:3] > lo_m) & (v[1:24:3] <= hi_m)).any() and (v[2:24:3] < hi_f).all()


class _NoTracks(object):
    def __init__(self, gt):
        self.boxes, self.off = gt.boxes, gt.off

    def __len__(self):
        return len(self.off) - 1


def test_host_checks():
    case = motion_iou_cases.build([[[(0, B), (1, B_HALF)], [(0, B)]], [[(0, B)]]])
    gt, videos = case["gt"], case["videos"]
    for w in (0, 65, -1, 2.0, "10", None, True):
        with pytest.raises(ValueError, match=r"^motion_iou: window"):
            motion_iou.run(gt, videos, w, device="cpu")
    for bad in ([(0, 2)], [(0, 1), (2, 1)], [(0, 2), (2, 2)], [(1, 2)], []):
        with pytest.raises(ValueError, match=r"^motion_iou: the videos"):
            motion_iou.run(gt, bad, device="cpu")
    with pytest.raises(ValueError, match=r"^motion_iou: the ground truth carries no track ids"):
        motion_iou.run(_NoTracks(gt), videos, device="cpu")
    dup = motion_iou_cases.build([[[(3, B), (1, B_HALF), (3, B_HALF)]]])
    with pytest.raises(ValueError, match=r"^motion_iou: frame 0 holds two boxes with the track id 3$"):
        motion_iou.run(dup["gt"], dup["videos"], device="cpu")
    for v in (np.nan, np.inf, -np.inf):
        inf = motion_iou_cases.build([[[(0, [0, 0, v, 8])]]])
        with pytest.raises(ValueError, match=r"^motion_iou: a GT box is not finite$"):
            motion_iou.run(inf["gt"], inf["videos"], device="cpu")
    # the checks come first; then there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU path"):
        motion_iou.run(gt, videos, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        motion_iou.derive(gt, videos, device="cpu")


def test_request_checks():
    assert motion_iou.check_request(None, None) is None and motion_iou.check_request("file.mat", None) is None
    assert motion_iou.check_request([np.zeros(1)], None) is None
    assert motion_iou.check_request("derive", "anno") == 10
    assert motion_iou.check_request({"derive": True, "window": 4}, "anno") == 4
    assert motion_iou.check_request({"derive": True}, "anno") == 10
    for bad in ({"derive": True, "window": 0}, {"derive": True, "window": 65}, {"derive": False}, {"window": 3},
                {"derive": True, "windows": 3}):
        with pytest.raises(ValueError, match=r"^motion_iou: "):
            motion_iou.check_request(bad, "anno")
    with pytest.raises(ValueError, match=r"^motion_iou: deriving the table needs anno_path"):
        motion_iou.check_request("derive", None)
    from mega.pytorch_amd import config, inference
    cfg = config.get_cfg("R-50")
    with pytest.raises(ValueError, match=r"^motion_iou: window"):       # before the run, not after it
        inference.inference(cfg, None, "nowhere", "nothing.txt", anno_path="a", motion_iou={"derive": True, "window": 99})


def _reference_read(path):
    """The reference's indexing expression (its vid_eval.py:135-137), frame by frame instead of np.array over the ragged
    rows."""
    import scipy.io as sio
    motion_ious = sio.loadmat(path)
    return [[motion_ious['motion_iou'][i][0][j][0] if len(motion_ious['motion_iou'][i][0][j]) != 0 else 0
             for j in range(len(motion_ious['motion_iou'][i][0]))]
            for i in range(len(motion_ious['motion_iou']))]


@pytest.mark.parametrize("with_off", [True, False])
def test_save_mat_round_trip(tmp_path, with_off):
    pytest.importorskip("scipy.io")
    import scipy.io as sio
    case = CASES["c_gaps_and_empty_frame"]
    gt = case["gt"]
    v, _ = _twin(case)
    table = motion_iou_twin.per_frame(v, gt.off)
    assert [len(m) for m in table] == [2, 2, 1, 1, 2, 2, 1, 1, 1, 2] and table[3].tolist() == [0.0]
    assert len({x for m in table for x in m.tolist()}) > 8               # not just round numbers
    same = motion_iou.to_per_frame(v, gt.off)
    assert all(a.tolist() == b.tolist() and a.dtype == np.float64 for a, b in zip(same, table))
    path = str(tmp_path / "motion.mat")
    motion_iou.save_mat(path, table, off=gt.off if with_off else None)
    back = vid_eval.load_motion_iou(path)
    ref = _reference_read(path)
    assert len(back) == len(ref) == len(table)
    for m, b, r in zip(table, back, ref):
        r = np.asarray(r, np.float64).reshape(-1)
        assert b.dtype == np.float64
        assert b.view(np.uint64).tolist() == m.view(np.uint64).tolist() == r.view(np.uint64).tolist()
    # the file's layout: frame i an [n x 1] column, the frame without GT [1 x 0] (given the offsets)
    cells = sio.loadmat(path)["motion_iou"]
    assert cells.shape == (10, 1) and cells[0][0].shape == (2, 1) and cells[2][0].shape == (1, 1)
    assert cells[3][0].shape == ((1, 0) if with_off else (1, 1))
    # empty_weights, the evaluation's only use of the whole table, is the same from the file
    assert vid_eval.empty_weights(back, vid_eval.MOTION_RANGES) == vid_eval.empty_weights(table, vid_eval.MOTION_RANGES)


def test_save_mat_keeps_nan_and_rejects_other_offsets(tmp_path):
    pytest.importorskip("scipy.io")
    path = str(tmp_path / "m.mat")
    motion_iou.save_mat(path, [np.asarray([motion_iou.NAN, 0.25]), np.zeros(0)])
    back = vid_eval.load_motion_iou(path)
    assert np.isnan(back[0][0]) and back[0][1] == 0.25 and back[1].tolist() == [0.0]
    with pytest.raises(ValueError, match=r"^motion_iou: 2 frames, 2 offsets"):
        motion_iou.save_mat(path, [np.zeros(1), np.zeros(1)], off=[0, 1])


def test_compare_on_a_planted_difference():
    a = [np.asarray([0.95, 0.5]), np.asarray([0.0]), np.asarray([0.8, 0.85, 0.1]), np.asarray([0.3])]
    same = motion_iou.compare(a, [m.copy() for m in a])
    assert same == {"frames": 4, "entries": 7, "count_mismatch": [], "max_abs_diff": 0.0, "median_abs_diff": 0.0,
                    "range_changed": 0.0}
    b = [m.copy() for m in a]
    b[0][0] = 0.85              # slow -> medium: another range
    b[2][1] = 0.875             # medium -> medium
    b[3] = np.asarray([0.3, 0.4])       # another entry count: the frame is listed and left out of the figures
    r = motion_iou.compare(a, b)
    assert r["frames"] == 4 and r["entries"] == 6 and r["count_mismatch"] == [3]
    assert r["max_abs_diff"] == abs(0.95 - 0.85) and r["median_abs_diff"] == 0.0
    assert r["range_changed"] == 1.0 / 6.0
    # 0.7 and 0.9 lie in two ranges each (the bounds are closed): a move from 0.7 to 0.75 leaves "fast"
    r = motion_iou.compare([np.asarray([0.7, 0.9])], [np.asarray([0.75, 0.9])])
    assert r["range_changed"] == 0.5
    # other ranges; NaN lies in none
    r = motion_iou.compare([np.asarray([0.2, np.nan, np.nan])], [np.asarray([0.6, np.nan, 0.1])], ranges=[[0.0, 0.5], [0.5, 1.0]])
    assert r["range_changed"] == 2.0 / 3.0 and r["max_abs_diff"] == np.inf
    with pytest.raises(ValueError, match=r"^motion_iou: the tables cover 1 and 2 frames"):
        motion_iou.compare([np.zeros(1)], [np.zeros(1), np.zeros(1)])


def test_abi_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data
    ok = (p, p, p, p, p, 1, 1, 10, 1, p, p, None, 0, None)

    def call(**kw):
        names = ("gt_box", "gt_track", "gt_off", "v0", "v1", "F", "G", "W", "max_gt", "values", "counts", "ws", "ws_bytes",
                 "stream")
        args = dict(zip(names, ok))
        args.update(kw)
        return lib.mega_motion_iou(*[args[n] for n in names])
    for name in ("gt_box", "gt_track", "gt_off", "v0", "v1", "values", "counts"):
        assert call(**{name: None}) == 1, name
    assert call(G=-1) == 1 and call(F=-1) == 1
    for w in (0, -3, 65):
        assert call(W=w) == 1
    assert call(max_gt=4097) == 1 and call(max_gt=-1) == 1
    # 130 boxes x 20 slots do not fit LDS: the workspace holds every box's slots, and a smaller one is refused
    assert lib.mega_motion_iou_workspace_bytes(1000, 10, 102) == 0
    assert lib.mega_motion_iou_workspace_bytes(1000, 10, 103) == 1000 * 20 * 4 + 128 == 80128
    assert lib.mega_motion_iou_workspace_bytes(7, 64, 17) == 3584 and lib.mega_motion_iou_workspace_bytes(7, 64, 16) == 0
    assert lib.mega_motion_iou_workspace_bytes(0, 10, 4096) == 0 and lib.mega_motion_iou_workspace_bytes(5, 0, 4096) == 0
    assert call(G=1000, max_gt=130, ws=p, ws_bytes=80127) == 3 and call(G=1000, max_gt=130, ws=None, ws_bytes=0) == 1
    # nothing to do: no launch, no device needed
    assert call(F=0, v0=None, v1=None) == 0 and call(G=0, gt_box=None, gt_track=None, values=None, counts=None) == 0


def _eval_vid(tmp_path, *extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_vid.py"), "--predictions", "p.pth", "--img-index",
                           "i.txt", "--anno-path", "a"] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          cwd=str(tmp_path), timeout=120)


def test_eval_vid_argument_errors(tmp_path):
    r = _eval_vid(tmp_path, "--box-only", "--motion-iou", "derive")
    assert r.returncode == 2 and b"--motion-iou" in r.stdout
    r = _eval_vid(tmp_path, "--motion-window", "5")
    assert r.returncode == 2 and b"--motion-iou derive" in r.stdout
    r = _eval_vid(tmp_path, "--motion-iou", "file.mat", "--save-motion-iou", "out.mat")
    assert r.returncode == 2 and b"--motion-iou derive" in r.stdout
    for w in ("0", "65"):
        r = _eval_vid(tmp_path, "--motion-iou", "derive", "--motion-window", w)
        assert r.returncode == 2 and b"--motion-window must be in 1 .. 64" in r.stdout
    r = _eval_vid(tmp_path, "--motion-iou", "derive", "--motion-window", "ten")
    assert r.returncode == 2 and b"--motion-window" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_motion_iou.py"), "--img-index", "i.txt",
                        "--anno-path", "a", "--out", "m.mat", "--window", "0"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 2 and b"--window must be in 1 .. 64" in r.stdout
