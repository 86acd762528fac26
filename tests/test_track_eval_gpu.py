"""GPU: the tubelet-matching kernel (csrc/track_eval.hip through mega.pytorch_amd.track_eval) against the hand-computed
cases and the Python twin (tests/track_eval_twin.py) -- pair tables, match flags and matched GT tracks exactly, AP within
1e-12 -- tracks.link -> evaluate_tracks end to end, tools/eval_vid.py --tracks --tubelet-ap, and vid_eval.match_and_ap
after vid_iou moved into box_math.h."""
import os
import subprocess
import sys

import numpy as np
import pytest

import track_eval_cases
import track_eval_twin
import vid_twin
from mega.pytorch_amd import track_eval, tracks, vid_eval

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytestmark = pytest.mark.gpu
CASES = track_eval_cases.cases()


def _assert_equals_twin(got, want, thresholds=track_eval.THRESHOLDS):
    assert [(int(t["video"]), int(t["id"]), int(t["label"]), int(t["count"])) for t in got["tubelets"]] == \
        [t[:4] for t in want["tubelets"]]
    assert [float(t["score"]) for t in got["tubelets"]] == [t[4] for t in want["tubelets"]]      # the same f64
    np.testing.assert_array_equal(got["match"], want["match"])
    np.testing.assert_array_equal(got["matched_gt"], want["matched_gt"])
    np.testing.assert_array_equal(got["n_pos"], want["n_pos"])
    assert sorted(got["pairs"]) == sorted(want["pairs"])
    for key, w in want["pairs"].items():
        g = got["pairs"][key]
        assert g["tubelets"] == w["tubelets"] and g["gt"] == w["gt"], key
        np.testing.assert_array_equal(g["hits"], w["hits"])
        np.testing.assert_array_equal(g["both"], w["both"])
    assert [tuple(int(x) for x in row) for row in got["gt_table"]] == want["gt_table"]
    print("max |AP - twin|: %g" % np.nan_to_num(np.abs(got["ap"] - want["ap"])).max())
    np.testing.assert_allclose(got["ap"], want["ap"], rtol=0, atol=1e-12)      # (equal_nan: NaN where the twin has NaN)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_computed_cases(dev, name):
    case = CASES[name]
    preds, gt = track_eval_twin.to_inputs(case["preds"], case["gts"])
    got = track_eval.run(preds, gt, case["videos"], device=dev)
    track_eval_cases.check(case, got)
    _assert_equals_twin(got, track_eval_twin.run(case["preds"], case["gts"], case["videos"]))


LABELS = (1, 2, 5)
_SETS = {}


def _set(name):
    """A seeded set with the twin's answer, made once."""
    if name not in _SETS:
        base = [dict(L=40, n_gt=5, labels=LABELS, n_clutter=8) for _ in range(6)]
        spec = {
            # six videos of 40 frames, three labels; then a one-frame video, one without GT, one without tubelets
            "base": base + [dict(L=1, n_gt=2, labels=LABELS, n_clutter=2, p_drop=0.0, p_miss=0.0),
                            dict(L=5, n_gt=0, labels=LABELS, n_clutter=3),
                            dict(L=5, n_gt=3, labels=LABELS, n_clutter=0, p_miss=1.0)],
            # one task with 70 GT tracks (two chunks of lanes) whose table still fits LDS: at most 2 x 70 x 20 < 4096
            "wide": [dict(L=8, n_gt=70, labels=(3,), n_clutter=0, max_gt_len=5, p_drop=0.1, p_miss=0.75)],
            # 1,100 clutter tubelets against 70 GT tracks: the table (> 70,000 pairs) lives in the workspace
            "big": [dict(L=6, n_gt=70, labels=(3,), n_clutter=1100, max_gt_len=4, p_drop=0.1, p_miss=0.3)],
        }[name]
        preds, gts, videos = track_eval_twin.make_set({"base": 31, "wide": 32, "big": 33}[name], spec)
        _SETS[name] = (preds, gts, videos, {})
    return _SETS[name]


def _twin(name, **kw):
    preds, gts, videos, cache = _set(name)
    key = tuple(sorted(kw.items()))
    if key not in cache:
        cache[key] = track_eval_twin.run(preds, gts, videos, **kw)
    return cache[key]


@pytest.mark.parametrize("kw", [{}, {"tubelet_score": "max"}, {"thresholds": ((1, 3), (1, 1), (1, 2), (2, 3), (1, 1024))}])
def test_kernel_equals_twin_base_set(dev, kw):
    preds, gts, videos, _ = _set("base")
    bl, gt = track_eval_twin.to_inputs(preds, gts)
    got = track_eval.run(bl, gt, videos, device=dev, **kw)
    want = _twin("base", **kw)
    _assert_equals_twin(got, want)
    assert got["ws_pairs"] == 0
    assert got["match"].sum() > 10 and (got["match"][0] != got["match"][-1]).any()      # thresholds differ in what they admit
    assert len({t[4] for t in want["tubelets"]}) < len(want["tubelets"])                # tied scores occur
    vids = {int(t["video"]) for t in got["tubelets"]}
    assert 7 in vids and 8 not in vids and (got["gt_table"]["video"] == 8).any() and not (got["gt_table"]["video"] == 7).any()


def test_kernel_equals_twin_more_gt_tracks_than_lanes(dev):
    preds, gts, videos, _ = _set("wide")
    bl, gt = track_eval_twin.to_inputs(preds, gts)
    got = track_eval.run(bl, gt, videos, device=dev)
    _assert_equals_twin(got, _twin("wide"))
    (key, pair), = got["pairs"].items()
    assert len(pair["gt"]) == 70 and pair["hits"].size <= track_eval.LDS_PAIRS and got["ws_pairs"] == 0
    assert (got["matched_gt"] >= 64).any()             # a GT track of the second chunk is taken


def test_kernel_equals_twin_pair_table_in_the_workspace(dev):
    preds, gts, videos, _ = _set("big")
    bl, gt = track_eval_twin.to_inputs(preds, gts)
    got = track_eval.run(bl, gt, videos, device=dev, return_workspace=True)
    want = _twin("big")
    _assert_equals_twin(got, want)
    (key, pair), = got["pairs"].items()
    assert len(pair["gt"]) == 70 and len(pair["tubelets"]) > 1000 and pair["hits"].size > track_eval.LDS_PAIRS
    # the workspace path really ran: the workspace, preset to -1, now holds the task's two tables
    assert got["ws_pairs"] == pair["hits"].size
    ws_hits, ws_both = got["workspace"]
    np.testing.assert_array_equal(ws_hits.reshape(pair["hits"].shape), want["pairs"][key]["hits"])
    np.testing.assert_array_equal(ws_both.reshape(pair["both"].shape), want["pairs"][key]["both"])
    assert ws_both.sum() > 0 and got["match"].sum() > 0


def test_link_then_evaluate_split_track(dev, tmp_path):
    """The 9-frame GT track with the middle detection missing, linked with max_gap = 0: two tubelets of tIoU 4/9."""
    from seq_nms_twin import to_boxlists
    preds, gts, videos = track_eval_twin.split_track_case()
    _, gt = track_eval_twin.to_inputs(preds, gts)
    linked, table = tracks.link(to_boxlists(preds), videos, max_gap=0, device=dev)
    assert [o.get_field("track_ids").tolist() for o in linked] == [[0]] * 4 + [[]] + [[1]] * 4
    res = track_eval.evaluate_tracks(linked, gt, videos, output_folder=str(tmp_path), device=dev)
    np.testing.assert_allclose(res["ap"][:, 1], [1.0, 0.0, 0.0], rtol=0, atol=1e-12)
    assert res["map"].tolist() == res["ap"][:, 1].tolist() and abs(res["mean"] - 1.0 / 3.0) < 1e-12
    assert [tuple(int(x) for x in r) for r in res["gt_table"]] == [(0, 0, 1, 9, -1, 0, 0)]
    ids = [dict(p, track_id=np.asarray(o.get_field("track_ids").numpy())) for p, o in zip(preds, linked)]
    twin = track_eval_twin.run(ids, gts, videos)
    assert res["text"] == track_eval.format_result(track_eval.THRESHOLDS, twin["ap"])
    assert (tmp_path / "result_tubelets.txt").read_text() == res["text"]
    assert res["text"].startswith("tubelet AP | tIoU>=0.25 = 1.0000\ntubelet AP | tIoU>=0.50 = 0.0000\n")
    # with a gap of one frame bridged it is one tubelet of 8 of 9 frames: right at every threshold
    linked, _ = tracks.link(to_boxlists(preds), videos, max_gap=1, device=dev)
    res = track_eval.evaluate_tracks(linked, gt, videos, device=dev)
    np.testing.assert_allclose(res["ap"][:, 1], [1.0, 1.0, 1.0], rtol=0, atol=1e-12)
    assert [tuple(int(x) for x in r) for r in res["gt_table"]] == [(0, 0, 1, 9, 0, 8, 9)]


def test_eval_vid_tracks_tubelet_ap_in_a_child_process(dev, tmp_path):
    """tools/eval_vid.py --tracks --tubelet-ap on a tiny XML set: result_tubelets.txt equals evaluate_tracks' text on the
    tracks the tool linked; then --tubelet-ap alone on the predictions_tracks.pth it wrote."""
    from test_track_eval import _write_set
    from mega.pytorch_amd import inference
    from seq_nms_twin import to_boxlists
    a, b = vid_eval.CLASSES_MAP[3], vid_eval.CLASSES_MAP[7]
    T = 6
    frames = [[(a, 0, (10 + 2 * t, 10, 60 + 2 * t, 50)), (b, 1, (80, 20, 140, 80))] if t != 2 else
              [(a, 0, (14, 10, 64, 50))] for t in range(T)]
    index, anno = _write_set(tmp_path, frames)
    rng = np.random.default_rng(3)
    preds = []
    for t in range(T):
        box = [[10 + 2 * t + rng.normal(0, 1), 10, 60 + 2 * t, 50], [81, 21, 139, 79], [100, 5, 120, 30]]
        keep = [0, 1, 2] if t != 3 else [1, 2]                # label 3's detection is missing in frame 3
        preds.append({"box": np.asarray(box, np.float32)[keep], "score": np.asarray([0.9, 0.7, 0.3], np.float32)[keep],
                      "label": np.asarray([3, 7, 7])[keep], "size": (160, 90)})
    inference.save_predictions(to_boxlists(preds), str(tmp_path / "predictions.pth"))
    out = tmp_path / "cli"
    base = [sys.executable, os.path.join(ROOT, "tools", "eval_vid.py"), "--img-index", index, "--anno-path", anno,
            "--device", str(dev)]
    r = subprocess.run(base + ["--predictions", str(tmp_path / "predictions.pth"), "--output-folder", str(out), "--tracks",
                               "--tracks-max-gap", "0", "--tubelet-ap"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=dict(os.environ), timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    gt = vid_eval.VIDTrackGroundTruth(index, anno)
    linked, _ = tracks.link(to_boxlists(preds), [(0, T)], max_gap=0, device=dev)
    res = track_eval.evaluate_tracks(linked, gt, [(0, T)], device=dev)
    text = (out / "result_tubelets.txt").read_text()
    assert text == res["text"] and ("Tubelets:\n" + text) in r.stdout.decode()
    # label 3's track is split 3 + 2 of 6 frames: 1/2 and 1/3; label 7's covers 5 of its 6 frames
    np.testing.assert_allclose([res["ap"][1, 7], res["ap"][0, 3], res["ap"][1, 3], res["ap"][2, 3]], [1, 1, 1, 0], rtol=0,
                               atol=1e-12)
    out2 = tmp_path / "cli2"
    r = subprocess.run(base + ["--predictions", str(out / "predictions_tracks.pth"), "--output-folder", str(out2),
                               "--tubelet-ap", "--tubelet-score", "max"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=dict(os.environ), timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert (out2 / "result_tubelets.txt").read_text() == \
        track_eval.evaluate_tracks(linked, gt, [(0, T)], tubelet_score="max", device=dev)["text"]
    assert not (out2 / "tracks.txt").exists()


def test_vid_eval_match_and_ap_unchanged(dev):
    """vid_iou now lives in box_math.h: the detection AP's kernels still equal their twin bit for bit."""
    preds, gts, motion = vid_twin.make_frames(7)
    bl, gt = vid_twin.to_boxlists(preds, gts)
    got = vid_eval.match_and_ap(bl, gt, motion, device=dev)
    want = vid_twin.evaluate(preds, gts, motion)
    assert got["ap"].shape == (len(want), len(want[0]["ap"]))
    for ri, w in enumerate(want):
        np.testing.assert_array_equal(got["match"][ri], w["match"])
        np.testing.assert_array_equal(got["pred_ignore"][ri].view(np.uint64), w["pred_ignore"].view(np.uint64))
        np.testing.assert_array_equal(got["n_pos"][ri], w["n_pos"])
        np.testing.assert_allclose(got["ap"][ri], w["ap"], rtol=0, atol=1e-9, equal_nan=True)   # test_vid_eval_gpu's bound
