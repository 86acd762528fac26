"""CPU: tubelet AP (mega/pytorch_amd/track_eval.py) -- the Python twin (tests/track_eval_twin.py) against the hand-computed
cases, VIDTrackGroundTruth on XML files with and without <trackid>, every host check, the text, the new C-ABI entry
points' declaration and argument checks (no GPU needed) and the command line's option checks."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import track_eval_cases
import track_eval_twin
from mega.pytorch_amd import _lib, track_eval, vid_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = track_eval_cases.cases()


def test_hand_computed_box_ious():
    """The IoUs the cases rest on, written out without the twin."""
    f = np.float32
    b = [f(0), f(0), f(8) + f(1), f(8) + f(1)]
    area_b = (b[2] - b[0] + f(1)) * (b[3] - b[1] + f(1))
    assert area_b == f(100)
    for y2, want in ((f(3), True), (f(2.99), False)):
        g = [f(0), f(0), f(8) + f(1), y2 + f(1)]
        inter = (min(b[2], g[2]) - f(0) + f(1)) * (min(b[3], g[3]) - f(0) + f(1))
        area_g = (g[2] - g[0] + f(1)) * (g[3] - g[1] + f(1))
        iou = inter / ((area_b + area_g) - inter)
        assert (iou >= f(0.5)) == want and (iou == f(0.5)) == want
    size = (200, 200)
    assert track_eval_twin.box_iou([0, 0, 8, 8], size, [0, 0, 8, 3], size) == f(0.5)
    assert f(0.49) < track_eval_twin.box_iou([0, 0, 8, 8], size, [0, 0, 8, 2.99], size) < f(0.5)
    assert track_eval_twin.box_iou([0, 0, 4, 2], (100, 50), [0, 0, 8, 8], size) == f(1)
    assert np.isnan(track_eval_twin.box_iou([5, 5, 3, 3], size, [5, 5, 3, 3], size))      # 0 / 0: no hit


@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_reproduces_hand_computed_cases(name):
    case = CASES[name]
    track_eval_cases.check(case, track_eval_twin.run(case["preds"], case["gts"], case["videos"]))


def test_twin_gt_table_and_max_score():
    case = CASES["equal_tiou_lower_number"]
    r = track_eval_twin.run(case["preds"], case["gts"], case["videos"])
    # (video, number, label, length, tubelet, hits, union) at the 1/2 threshold: number 0 (id 5) is taken, 1 (id 7) is not
    assert r["gt_table"] == [(0, 0, 1, 1, 3, 1, 2), (0, 1, 1, 4, -1, 0, 0)]
    case = CASES["two_compete"]
    preds = [dict(p, score=p["score"] * np.float32(0.5 if t else 1.0)) for t, p in enumerate(case["preds"])]
    mean = track_eval_twin.run(preds, case["gts"], case["videos"], tubelet_score="mean")
    mx = track_eval_twin.run(preds, case["gts"], case["videos"], tubelet_score="max")
    f = np.float32
    s0 = (np.float64(f(0.6)) + np.float64(f(0.6) * f(0.5)) * 3) / 4
    assert [t[4] for t in mean["tubelets"]][0] == s0 and [t[4] for t in mx["tubelets"]] == [float(f(0.6)), float(f(0.9))]


def _xml(h, w, objs):
    s = "<annotation><size><width>%d</width><height>%d</height></size>" % (w, h)
    for name, tid, (x1, y1, x2, y2) in objs:
        s += "<object>%s<name>%s</name><bndbox><xmax>%d</xmax><xmin>%d</xmin><ymax>%d</ymax><ymin>%d</ymin></bndbox>" \
             "</object>" % ("" if tid is None else "<trackid>%d</trackid>" % tid, name, x2, x1, y2, y1)
    return s + "</annotation>"


def _write_set(tmp_path, frames):
    os.makedirs(str(tmp_path / "Anno" / "v"))
    lines = []
    for t, objs in enumerate(frames):
        (tmp_path / "Anno" / "v" / ("%06d.xml" % t)).write_text(_xml(90, 160, objs))
        lines.append("v %d %d %d" % (t + 1, t, len(frames)))
    (tmp_path / "index.txt").write_text("\n".join(lines) + "\n")
    return str(tmp_path / "index.txt"), str(tmp_path / "Anno")


def test_ground_truth_reads_track_ids_and_its_cache(tmp_path):
    a, b = vid_eval.CLASSES_MAP[3], vid_eval.CLASSES_MAP[7]
    frames = [[(a, 4, (1, 2, 30, 40)), ("n00000000", None, (0, 0, 5, 5)), (b, 0, (10, 10, 50, 60))], [],
              [(b, 0, (12, 10, 52, 60))]]
    index, anno = _write_set(tmp_path, frames)
    plain = vid_eval.VIDGroundTruth(index, anno)
    gt = vid_eval.VIDTrackGroundTruth(index, anno, cache=str(tmp_path / "c" / "gt.npz"))
    assert gt.track_ids.tolist() == [4, 0, 0] and gt.track_ids.dtype == np.int64      # the unknown wnid is skipped
    for name in ("boxes", "labels", "off", "height", "width"):
        np.testing.assert_array_equal(getattr(gt, name), getattr(plain, name))
    assert gt.labels.tolist() == [3, 7, 7] and gt.off.tolist() == [0, 2, 2, 3]
    z = np.load(str(tmp_path / "c" / "gt.npz"))
    assert sorted(z.files) == sorted(["image_set_index", "boxes", "labels", "off", "height", "width", "track_ids"])
    for f in os.listdir(anno + "/v"):
        os.remove(os.path.join(anno, "v", f))                  # the second read comes from the cache alone
    again = vid_eval.VIDTrackGroundTruth(index, anno, cache=str(tmp_path / "c" / "gt.npz"))
    assert again.track_ids.tolist() == [4, 0, 0] and again.boxes.tolist() == gt.boxes.tolist()
    assert isinstance(gt, vid_eval.VIDGroundTruth) and gt.get_groundtruth(0).get_field("labels").tolist() == [3, 7]


def test_ground_truth_without_trackid_names_the_file(tmp_path):
    a = vid_eval.CLASSES_MAP[3]
    index, anno = _write_set(tmp_path, [[(a, 1, (1, 2, 30, 40))], [(a, None, (1, 2, 30, 40))]])
    with pytest.raises(ValueError, match=r"000001\.xml.*trackid"):
        vid_eval.VIDTrackGroundTruth(index, anno)
    plain = vid_eval.VIDGroundTruth(index, anno, cache=str(tmp_path / "plain.npz"))      # needs none, as before
    assert plain.labels.tolist() == [3, 3] and not hasattr(plain, "track_ids")
    assert "track_ids" not in np.load(str(tmp_path / "plain.npz")).files
    root = __import__("xml.etree.ElementTree").etree.ElementTree.fromstring(_xml(9, 9, [(a, 1, (1, 2, 3, 4))]))
    assert sorted(vid_eval.parse_annotation(root)) == ["boxes", "im_info", "labels"]
    # a plain cache has no ids: the track GT re-reads the XML files (and fails on the same file)
    with pytest.raises(ValueError, match="trackid"):
        vid_eval.VIDTrackGroundTruth(index, anno, cache=str(tmp_path / "plain.npz"))


def _inputs(P, G, **kw):
    preds, gts = track_eval_cases._frames(P, G, **kw)
    return track_eval_twin.to_inputs(preds, gts)


def test_bad_input_raises_before_device_work():
    B, FAR = track_eval_cases.B, track_eval_cases.FAR
    ok_p, ok_g = ([B], [0.9], [1], [0]), ([B], [1], [0])
    nan, inf = float("nan"), float("inf")
    cases = [
        ([([B], [0.9], [1], [-2])], [ok_g], "below -1"),
        ([([B, FAR], [0.9, 0.8], [1, 1], [0, 0])], [ok_g], "two boxes of one tubelet in the same frame"),
        ([ok_p], [([B, FAR], [1, 1], [0, 0])], "two boxes of one GT track in the same frame"),
        ([ok_p, ([B], [0.9], [2], [0])], [ok_g, ok_g], "a tubelet with more than one label"),
        ([ok_p, ok_p], [ok_g, ([B], [2], [0])], "a GT track with more than one label"),
        ([([B], [nan], [1], [0])], [ok_g], "NaN"),
        ([([[0, 0, inf, 8]], [0.9], [1], [0])], [ok_g], "not finite"),
        ([ok_p], [([[0, nan, 8, 8]], [1], [0])], "GT box is not finite"),
        ([([B], [0.9], [-1], [0])], [ok_g], "negative class"),
        ([ok_p], [([B], [-3], [0])], "negative class"),
    ]
    for P, G, msg in cases:
        preds, gt = _inputs(P, G)
        for fn in (track_eval.run, track_eval.evaluate_tracks):
            with pytest.raises(ValueError, match="^track_eval: .*" + msg):
                fn(preds, gt, [(0, len(P))])               # device="cuda": the checks come first
    preds, gt = _inputs([ok_p, ok_p], [ok_g, ok_g])
    with pytest.raises(ValueError, match="^track_eval: 1 predictions, 2 GT frames"):
        track_eval.run(preds[:1], gt, [(0, 1)])
    with pytest.raises(ValueError, match="^track_eval: the videos cover"):
        track_eval.run(preds, gt, [(0, 1)])
    from seq_nms_twin import to_boxlists
    bare = to_boxlists(track_eval_cases._frames([ok_p, ok_p], [ok_g, ok_g])[0])
    with pytest.raises(ValueError, match="^track_eval: a prediction has no field \"track_ids\""):
        track_eval.run(bare, gt, [(0, 2)])
    plain = vid_eval.VIDGroundTruth.from_annotations([{"boxes": np.zeros((0, 4), np.float32), "labels": np.zeros(0, np.int64),
                                                       "im_info": (9, 9)}] * 2)
    with pytest.raises(ValueError, match="^track_eval: the ground truth carries no track ids"):
        track_eval.run(preds, plain, [(0, 2)])
    # a tubelet id may repeat in another video, a GT track id too
    p2, g2 = _inputs([ok_p, ok_p], [ok_g, ok_g])
    with pytest.raises(RuntimeError, match="no CPU path"):
        track_eval.run(p2, g2, [(0, 1), (1, 1)], device="cpu")
    for bad in (((0, 4),), ((5, 4),), ((1, 1025),), ((1.0, 2),), (), ((1, 2),) * 9, ((True, 2),), (1, 2)):
        with pytest.raises(ValueError, match="^track_eval: .*threshold"):
            track_eval.run(preds, gt, [(0, 2)], thresholds=bad)
    with pytest.raises(ValueError, match="tubelet_score"):
        track_eval.evaluate_tracks(preds, gt, [(0, 2)], tubelet_score="sum")
    assert track_eval.check_params() == ((1, 4), (1, 2), (3, 4)) and track_eval.check_params(((1024, 1024),)) == ((1024, 1024),)


def test_format_result_and_summary():
    nan = float("nan")
    ap = np.asarray([[nan, 1.0, 0.5, nan], [0.3, 0.25, 0.75, nan], [nan, 0.0, 0.125, nan]])
    maps, mean = track_eval.summarize(ap)
    assert maps.tolist() == [0.75, 0.5, 0.0625] and mean == (0.75 + 0.5 + 0.0625) / 3     # label 0 never counts
    text = track_eval.format_result(((1, 4), (1, 2), (3, 4)), ap, classes=["bg", "a", "b", "c"])
    assert text == ("tubelet AP | tIoU>=0.25 = 0.7500\ntubelet AP | tIoU>=0.50 = 0.5000\ntubelet AP | tIoU>=0.75 = 0.0625\n"
                    "tubelet AP | mean       = 0.4375\nCategory AP:\n"
                    "a               : 0.2500\nb               : 0.7500\nc               : nan\n")
    # the category lines are vid_eval.format_result's, for the 1/2 row
    ref = vid_eval.format_result({0: {"ap": ap[1], "map": 0.0}}, classes=["bg", "a", "b", "c"])
    assert text.split("Category AP:\n")[1] == ref.split("Category AP:\n")[1]
    assert track_eval.table_threshold(((1, 4), (3, 6))) == 1 and track_eval.table_threshold(((1, 4), (3, 4))) == 0


def test_entry_points_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "mega_hip.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in ("mega_tubelet_match", "mega_tubelet_match_workspace_bytes", "mega_tubelet_scores"):
        assert re.search(r"\b%s\s*\(" % name, decl), name + " is not declared in mega_hip.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        m = re.search(r"\b(int|size_t)\s+%s\s*\((.*?)\);" % name, decl, flags=re.S)
        params = [p.strip() for p in m.group(2).split(",")]
        assert res is {"int": _lib.c_int, "size_t": _lib.c_size_t}[m.group(1)] and len(args) == len(params)
        for a, p in zip(args, params):                        # every parameter's C type against its ctypes type
            want = _lib.c_void_p if "*" in p else {"int": _lib.c_int, "long long": _lib.c_longlong,
                                                   "size_t": _lib.c_size_t}[p.rsplit(" ", 1)[0]]
            assert a is want, (name, p)
    assert "track_eval.py" in src[src.index("Tubelet AP"):src.index("mega_tubelet_match_workspace_bytes(long")]


#        box frame rank seg ratio gbox gtrack gseg tasks offs tubelet tlen glen
_ARGS = [8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8]


def _call(lib, thr=(1, 4, 1, 2, 3, 4), T=1, F=1, C=1, R=3, M=1, Gb=1, U=1, J=1, slots=1, n_pairs=1, ws_pairs=0, ptrs=None,
          outs=(8, 8, 8, 8), ws=8, ws_bytes=1 << 20):
    import ctypes
    t = None if thr is None else ctypes.cast((ctypes.c_int * len(thr))(*thr), ctypes.c_void_p)
    return lib.mega_tubelet_match(*(list(ptrs or _ARGS) + [t, T, F, C, R, M, Gb, U, J, slots, n_pairs, ws_pairs] + list(outs) +
                                    [ws, ws_bytes, None]))


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    for i in range(len(_ARGS)):                                  # each input pointer NULL
        p = list(_ARGS)
        p[i] = None
        assert _call(lib, ptrs=p) == 1
    assert _call(lib, thr=None) == 1
    assert _call(lib, outs=(None, 8, 8, 8)) == 1 and _call(lib, outs=(8, None, 8, 8)) == 1
    assert _call(lib, outs=(8, 8, None, 8)) == 1 and _call(lib, outs=(8, 8, 8, None)) == 1     # one pair table without the other
    for name in ("T", "F", "C", "M", "Gb", "U", "J", "slots", "n_pairs", "ws_pairs"):
        assert _call(lib, **{name: -1}) == 1, name
    for name in ("F", "C", "M", "Gb", "U", "J", "slots"):        # zero with T > 0
        assert _call(lib, **{name: 0}) == 1, name
    assert _call(lib, R=0) == 1 and _call(lib, R=9, thr=(1, 2) * 9) == 1
    for thr in ((0, 4, 1, 2, 3, 4), (1, 4, 3, 2, 3, 4), (1, 4, 1, 2, 1, 1025), (1, 4, -1, 2, 3, 4), (1, 4, 1, 0, 3, 4)):
        assert _call(lib, thr=thr) == 1, thr
    assert _call(lib, M=1 << 31) == 1 and _call(lib, F=1 << 30) == 1
    assert _call(lib, ws_pairs=5000, ws=None) == 1
    # T = 0: nothing to do, not an error, nothing is touched
    assert _call(lib, T=0, F=0, C=0, M=0, Gb=0, U=0, J=0, slots=0, n_pairs=0, ptrs=[None] * 13, outs=(None,) * 4, ws=None,
                 ws_bytes=0) == 0
    # workspace: two i32 tables of ws_pairs entries, each rounded up to 256 bytes -- none when every task fits LDS
    ws = lib.mega_tubelet_match_workspace_bytes
    assert ws(0) == 0 and ws(-7) == 0
    assert ws(1) == 2 * 256 and ws(64) == 2 * 256 and ws(65) == 2 * 512
    assert ws(70000) == 2 * ((70000 * 4 + 255) // 256 * 256) == 560128
    assert _call(lib, ws_pairs=70000, ws_bytes=560127) == 3       # workspace too small
    # the score entry point
    sc = lib.mega_tubelet_scores
    assert sc(8, 8, -1, 1, 0, 8, None) == 1 and sc(8, 8, 1, -1, 0, 8, None) == 1 and sc(8, 8, 1, 1, 2, 8, None) == 1
    assert sc(None, 8, 1, 1, 0, 8, None) == 1 and sc(8, None, 1, 1, 0, 8, None) == 1 and sc(8, 8, 1, 1, 0, None, None) == 1
    assert sc(8, 8, 1, 0, 0, 8, None) == 1 and sc(None, None, 0, 0, 0, None, None) == 0


def test_lds_budget_matches_the_kernel_source():
    src = open(os.path.join(ROOT, "mega", "pytorch_amd", "csrc", "track_eval.hip")).read()
    assert int(re.search(r"TE_LDS_PAIRS\s*=\s*(\d+)", src).group(1)) == track_eval.LDS_PAIRS
    assert int(re.search(r"TE_MAX_CHUNKS\s*=\s*(\d+)", src).group(1)) * 64 == track_eval.MAX_GT_TRACKS
    assert int(re.search(r"TE_MAX_R\s*=\s*(\d+)", src).group(1)) == track_eval.MAX_THRESHOLDS
    assert 2 * 4 * track_eval.LDS_PAIRS <= 160 * 1024 // 4        # four workgroups' tables fit a CU's LDS


def _eval_vid(tmp_path, *extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_vid.py"), "--predictions", "p.pth", "--img-index",
                           "i.txt", "--anno-path", "a"] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          cwd=str(tmp_path), timeout=120)


def test_eval_vid_argument_errors(tmp_path):
    r = _eval_vid(tmp_path, "--tubelet-ap", "--box-only")
    assert r.returncode == 2 and b"--tubelet-ap" in r.stdout
    r = _eval_vid(tmp_path, "--tubelet-ap", "--tubelet-score", "sum")
    assert r.returncode == 2 and b"--tubelet-score" in r.stdout
    # predictions without track ids and no --tracks: an argument error, before any annotation is read
    from mega.pytorch_amd import inference
    from seq_nms_twin import to_boxlists
    case = CASES["perfect"]
    inference.save_predictions(to_boxlists(case["preds"]), str(tmp_path / "p.pth"))
    r = _eval_vid(tmp_path, "--tubelet-ap")
    assert r.returncode == 2 and b"track_ids" in r.stdout


def test_inference_checks_the_tubelet_score_before_the_run():
    from mega.pytorch_amd import config, inference
    cfg = config.get_cfg("R-50")
    with pytest.raises(ValueError, match="tubelet_score"):
        inference.inference(cfg, None, "nowhere", "nothing.txt", tracks={"tubelet_ap": True, "tubelet_score": "median"})
