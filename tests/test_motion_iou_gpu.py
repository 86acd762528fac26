"""GPU: the motion IoU kernel (csrc/motion_iou.hip through mega.pytorch_amd.motion_iou) against the Python twin
(tests/motion_iou_twin.py), bit for bit -- values as int64, counts -- on the shared cases; the workspace path;
evaluate_detections on the derived table; tools/eval_vid.py --motion-iou derive --save-motion-iou; inference's request
forms; tools/make_motion_iou.py --compare; run-to-run identity.  No tolerance anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import motion_iou_cases
import motion_iou_twin
from mega.pytorch_amd import flat, motion_iou, ops, vid_eval

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytestmark = pytest.mark.gpu
CASES = motion_iou_cases.cases()
_TWIN = {}


def _twin(name):
    """The twin's answer of a shared case, computed once."""
    if name not in _TWIN:
        gt, case = CASES[name]["gt"], CASES[name]
        _TWIN[name] = motion_iou_twin.run(gt.boxes, gt.off, gt.track_ids, case["videos"], case["window"])
    return _TWIN[name]


def _assert_bits(got, want):
    (v, c), (tv, tc) = got, want
    assert v.dtype == np.float64 and c.dtype == np.int32 and v.shape == tv.shape and c.shape == tc.shape
    np.testing.assert_array_equal(c, tc)
    np.testing.assert_array_equal(v.view(np.int64), tv.view(np.int64))


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_twin(dev, name):
    case = CASES[name]
    got = motion_iou.run(case["gt"], case["videos"], case["window"], device=dev)
    _assert_bits(got, _twin(name))
    table = motion_iou.derive(case["gt"], case["videos"], case["window"], device=dev)
    want = motion_iou_twin.per_frame(_twin(name)[0], case["gt"].off)
    assert len(table) == len(want) == len(case["gt"])
    for a, b in zip(table, want):
        assert a.dtype == np.float64 and a.view(np.int64).tolist() == b.view(np.int64).tolist()


def test_the_130_box_frame_runs_in_the_workspace(dev):
    """ops.motion_iou on case (f) with the workspace handed back: preset to -1, it now holds the pair IoUs of the 130-box
    frame (three boxes with four neighbours each), and nothing of the 3-box frames, which fit LDS."""
    case = CASES["f_130_boxes"]
    gt = case["gt"]
    _, parts, max_gt = motion_iou._pack(gt, case["videos"], case["window"])
    assert max_gt == 130 and max_gt * 2 * case["window"] > motion_iou.LDS_PAIRS
    t = flat.upload(parts, dev)
    with torch.cuda.device(dev):
        v, c, ws = ops.motion_iou(t["box"], t["track"], t["off"], t["v0"], t["v1"], case["window"], max_gt,
                                  return_workspace=True)
    _assert_bits((v.cpu().numpy(), c.cpu().numpy()), _twin("f_130_boxes"))
    ws = ws.cpu().numpy()
    s, e = int(gt.off[2]), int(gt.off[3])
    assert ws.shape == (len(gt.boxes), 20) and (ws[:s] == -1).all() and (ws[e:] == -1).all()
    found = ws[s:e] != -1
    assert found.sum(1).tolist() == _twin("f_130_boxes")[1][s:e].tolist() and found.sum() == 12
    # the slots are in offset order -W .. -1, +1 .. +W: the neighbours at d = -2, -1, +1, +2 are slots 8 .. 11
    assert np.nonzero(found[64])[0].tolist() == [8, 9, 10, 11]
    want = [motion_iou_twin.pair_iou(gt.boxes[s + 64], gt.boxes[gt.off[f] + 1]) for f in (0, 1, 3, 4)]
    assert ws[s + 64, 8:12].view(np.float32).tolist() == want
    # without a frame that large there is no workspace at all
    small = CASES["g_random"]
    _, parts, max_gt = motion_iou._pack(small["gt"], small["videos"], small["window"])
    t = flat.upload(parts, dev)
    with torch.cuda.device(dev):
        assert ops.motion_iou(t["box"], t["track"], t["off"], t["v0"], t["v1"], small["window"], max_gt,
                              return_workspace=True)[2] is None


def test_two_runs_are_bit_identical(dev):
    case = CASES["g_random"]
    a = motion_iou.run(case["gt"], case["videos"], case["window"], device=dev)
    b = motion_iou.run(case["gt"], case["videos"], case["window"], device=dev)
    _assert_bits(a, b)
    assert a[1].max() >= 10 and len(set(a[0].tolist())) > 100          # neighbours on both sides; no trivial table


def _detections(gt, seed):
    """Jittered copies of the GT boxes (some dropped, some mislabelled) plus clutter, as seq_nms_twin frame dicts."""
    rng = np.random.default_rng(seed)
    out = []
    for f in range(len(gt)):
        s, e = gt.off[f], gt.off[f + 1]
        keep = rng.random(e - s) < 0.85
        box = gt.boxes[s:e][keep] + rng.normal(0, 2.0, (int(keep.sum()), 4)).astype(np.float32)
        lab = gt.labels[s:e][keep].copy()
        lab[rng.random(len(lab)) < 0.1] = 1
        clutter = np.asarray([[100, 5, 150, 40], [3, 150, 40, 190]], np.float32)
        out.append({"box": np.concatenate([box, clutter]).astype(np.float32),
                    "score": rng.uniform(0.05, 1.0, len(lab) + 2).astype(np.float32),
                    "label": np.concatenate([lab, [2, 3]]).astype(np.int64), "size": (200, 200)})
    return out


def test_evaluate_detections_on_the_derived_table(dev):
    from seq_nms_twin import to_boxlists
    case = motion_iou_cases.motion_ranges_set()
    gt = case["gt"]
    tv, _ = motion_iou_twin.run(gt.boxes, gt.off, gt.track_ids, case["videos"], case["window"])
    twin_table = motion_iou_twin.per_frame(tv, gt.off)
    table = motion_iou.derive(gt, case["videos"], case["window"], device=dev)
    preds = to_boxlists(_detections(gt, 5))
    got = vid_eval.evaluate_detections(preds, gt, motion_iou=table, device=dev)
    want = vid_eval.evaluate_detections(preds, gt, motion_iou=twin_table, device=dev)
    assert sorted(got) == sorted(want) == [0, 1, 2, 3]
    for r in range(4):
        assert got[r]["ap"].view(np.int64).tolist() == want[r]["ap"].view(np.int64).tolist()
        assert np.float64(got[r]["map"]).view(np.int64) == np.float64(want[r]["map"]).view(np.int64)
    # the positives of each range are the GT boxes whose twin value lies in it; every range holds one
    n_pos = vid_eval.match_and_ap(preds, gt, table, device=dev)["n_pos"]
    in_range = [int(((tv >= lo) & (tv <= hi)).sum()) for lo, hi in vid_eval.MOTION_RANGES]
    assert n_pos.sum(1).tolist() == in_range and in_range[0] == len(tv) and min(in_range) >= 1
    assert len({round(float(got[r]["map"]), 12) for r in range(4)}) > 1 and not np.isnan([got[r]["map"] for r in range(4)]).any()


def _write_videos(tmp_path, videos):
    """videos: {name: frames}, a frame a list of (wnid, track id, box) -> (index file, annotation directory)."""
    from test_track_eval import _xml
    lines, n = [], 0
    for name, frames in videos.items():
        os.makedirs(str(tmp_path / "Anno" / name))
        for t, objs in enumerate(frames):
            (tmp_path / "Anno" / name / ("%06d.xml" % t)).write_text(_xml(200, 200, objs))
            n += 1
            lines.append("%s %d %d %d" % (name, n, t, len(frames)))
    (tmp_path / "index.txt").write_text("\n".join(lines) + "\n")
    return str(tmp_path / "index.txt"), str(tmp_path / "Anno")


def test_eval_vid_derives_and_saves_the_table_in_a_child_process(dev, tmp_path):
    """tools/eval_vid.py --motion-iou derive --save-motion-iou on a small XML tree: a four-range result.txt, and a .mat
    whose reload reproduces it."""
    from mega.pytorch_amd import inference
    from seq_nms_twin import to_boxlists
    case = motion_iou_cases.motion_ranges_set()
    gt0 = case["gt"]
    wnid = vid_eval.CLASSES_MAP
    videos = {"va": [], "vb": []}
    for (start, length), name in zip(case["videos"], videos):
        for f in range(start, start + length):
            videos[name].append([(wnid[int(gt0.labels[i])], int(gt0.track_ids[i]), tuple(int(x) for x in gt0.boxes[i]))
                                 for i in range(gt0.off[f], gt0.off[f + 1])])
    index, anno = _write_videos(tmp_path, videos)
    gt = vid_eval.VIDTrackGroundTruth(index, anno)
    np.testing.assert_array_equal(gt.boxes, gt0.boxes)
    np.testing.assert_array_equal(gt.track_ids, gt0.track_ids)
    preds = to_boxlists(_detections(gt0, 6))
    inference.save_predictions(preds, str(tmp_path / "predictions.pth"))
    out, mat = tmp_path / "cli", tmp_path / "derived.mat"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_vid.py"), "--predictions",
                        str(tmp_path / "predictions.pth"), "--img-index", index, "--anno-path", anno, "--device", str(dev),
                        "--output-folder", str(out), "--motion-iou", "derive", "--motion-window", "10",
                        "--save-motion-iou", str(mat)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=dict(os.environ), timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    text = (out / "result.txt").read_text()
    assert [l.split("=")[1].strip() for l in text.splitlines()[:4]] == ["all", "fast", "medium", "slow"]
    assert text in r.stdout.decode()
    # the saved table is the twin's, bit for bit, and evaluating with it reproduces result.txt
    back = vid_eval.load_motion_iou(str(mat))
    tv, _ = motion_iou_twin.run(gt0.boxes, gt0.off, gt0.track_ids, case["videos"], 10)
    for a, b in zip(back, motion_iou_twin.per_frame(tv, gt0.off)):
        assert a.view(np.int64).tolist() == b.view(np.int64).tolist()
    vid_eval.evaluate_detections(preds, gt, motion_iou=back, output_folder=str(tmp_path / "again"), device=dev)
    assert (tmp_path / "again" / "result.txt").read_text() == text
    # what inference(motion_iou=...) does with its argument on the same tree: the request forms derive, a path loads
    for request, w in (("derive", 10), ({"derive": True, "window": 2}, 2)):
        table, tgt = motion_iou.resolve(request, index, anno, device=dev)
        tw, _ = motion_iou_twin.run(gt0.boxes, gt0.off, gt0.track_ids, case["videos"], w)
        assert isinstance(tgt, vid_eval.VIDTrackGroundTruth) and len(table) == len(gt0)
        for a, b in zip(table, motion_iou_twin.per_frame(tw, gt0.off)):
            assert a.view(np.int64).tolist() == b.view(np.int64).tolist()
    table, tgt = motion_iou.resolve(str(mat), index, anno, device=dev)
    assert tgt is None and [m.tolist() for m in table] == [m.tolist() for m in back]
    assert motion_iou.resolve(back, index, anno, device=dev) == (back, None)


def test_make_motion_iou_writes_and_compares(dev, tmp_path, capsys):
    """tools/make_motion_iou.py on a two-video XML tree: the .mat holds the twin's table; --compare against a copy with
    one planted value reports that one entry."""
    import json
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_motion_iou
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    a, b = vid_eval.CLASSES_MAP[3], vid_eval.CLASSES_MAP[7]
    videos = {"va": [[(a, 0, (10 + 3 * t, 10, 60 + 3 * t, 50)), (b, 1, (80, 20, 140, 80))] if t != 2 else [] for t in range(5)],
              "vb": [[(a, 0, (20, 30, 90, 120))], [(a, 0, (60, 30, 130, 120))]]}
    index, anno = _write_videos(tmp_path, videos)
    gt = vid_eval.VIDTrackGroundTruth(index, anno)
    tv, tc = motion_iou_twin.run(gt.boxes, gt.off, gt.track_ids, [(0, 5), (5, 2)], 3)
    want = motion_iou_twin.per_frame(tv, gt.off)
    planted = [m.copy() for m in want]
    assert 0.9 < planted[0][1] <= 1.0
    planted[0][1] = 0.5                  # slow -> fast
    motion_iou.save_mat(str(tmp_path / "ref.mat"), planted, off=gt.off)
    capsys.readouterr()
    assert make_motion_iou.main(["--img-index", index, "--anno-path", anno, "--out", str(tmp_path / "m.mat"), "--window", "3",
                                 "--compare", str(tmp_path / "ref.mat"), "--device", str(dev)]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    for x, y in zip(vid_eval.load_motion_iou(str(tmp_path / "m.mat")), want):
        assert x.view(np.int64).tolist() == y.view(np.int64).tolist()
    assert (res["frames"], res["gt_boxes"], res["window"], res["lone_boxes"]) == (7, 10, 3, int((tc == 0).sum()))
    assert res["compare"] == {"frames": 7, "entries": 11, "count_mismatch": [], "max_abs_diff": float(want[0][1]) - 0.5,
                              "median_abs_diff": 0.0, "range_changed": 1.0 / 11.0}
