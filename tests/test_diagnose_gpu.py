"""GPU: the detection error diagnosis (csrc/diagnose.hip, mega/pytorch_amd/diagnose.py) against the Python twin
(tests/diagnose_twin.py) on every case of tests/diagnose_cases.py: kinds, attributed boxes and per-GT detections equal, the
IoU bit for bit, the tables equal, AP and dAP at the tolerance tests/test_vid_eval_gpu.py uses for the AP against vid_twin
(atol 1e-12 without motion ranges); the matching against ops.vid_eval_match, stale output bytes, the motion cross-
tabulation, the text file and inference(..., diagnose=True)."""
import os

import numpy as np
import pytest
import torch

import diagnose_cases
import diagnose_twin
import vid_twin
from mega.pytorch_amd import diagnose, ops, vid_eval

pytestmark = pytest.mark.gpu
AP_ATOL = 1e-12
HAND = diagnose_cases.hand_cases()


def _sets():
    sets = {name: (c["preds"], c["gts"]) for name, c in HAND.items()}
    sets["random"] = diagnose_cases.random_frames(diagnose_twin.frame_iou)[:2]
    sets["size"] = diagnose_cases.size_frames(diagnose_twin.frame_iou)
    return sets


SETS = _sets()
_TWIN = {}


def _twin(name, **kw):
    key = (name, tuple(sorted((k, repr(v)) for k, v in kw.items())))
    if key not in _TWIN:
        _TWIN[key] = diagnose_twin.run(*SETS[name], **kw)
    return _TWIN[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _check(got, want):
    np.testing.assert_array_equal(got["det_kind"], want["det_kind"])
    np.testing.assert_array_equal(got["det_gt"], want["det_gt"])
    np.testing.assert_array_equal(got["gt_det"], want["gt_det"])
    np.testing.assert_array_equal(got["gt_state"], want["gt_state"])
    np.testing.assert_array_equal(_bits(got["det_iou"]), _bits(want["det_iou"]))
    assert got["det_kind"].dtype == np.uint8 and got["det_gt"].dtype == np.int32 and got["gt_det"].dtype == np.int32
    for k in ("kind_counts", "kind_counts_thr", "kind_counts_by_label", "kind_counts_thr_by_label", "gt_state_counts",
              "gt_state_counts_by_label", "confusion"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    if want["motion"] is None:
        assert got["motion"] is None
    else:
        for k in ("gt_state_counts", "kind_counts"):
            np.testing.assert_array_equal(got["motion"][k], want["motion"][k], err_msg=k)
    print("map", got["map"], want["map"])
    np.testing.assert_allclose(got["ap"], want["ap"], rtol=0, atol=AP_ATOL, equal_nan=True)
    np.testing.assert_allclose(got["map"], want["map"], rtol=0, atol=AP_ATOL, equal_nan=True)
    for k in diagnose.FIXES:
        print("dap", k, got["dap"][k], want["dap"][k])
        np.testing.assert_allclose(got["dap"][k], want["dap"][k], rtol=0, atol=AP_ATOL, equal_nan=True, err_msg=k)
        np.testing.assert_allclose(got["dap_by_class"][k], want["dap_by_class"][k], rtol=0, atol=AP_ATOL, equal_nan=True,
                                   err_msg=k)


@pytest.mark.parametrize("name", sorted(SETS))
def test_every_case_equals_the_twin(dev, name):
    bl, gt = vid_twin.to_boxlists(*SETS[name])
    got = diagnose.evaluate_errors(bl, gt, device=dev)
    _check(got, _twin(name))
    if name in HAND:                                   # and the hand-written expectations themselves
        assert got["det_kind"].tolist() == HAND[name]["kind"] and got["det_gt"].tolist() == HAND[name]["gt"]
        assert got["gt_det"].tolist() == [list(r) for r in HAND[name]["gt_det"]]


@pytest.mark.parametrize("name", ["random", "size"])
def test_other_thresholds_equal_the_twin(dev, name):
    bl, gt = vid_twin.to_boxlists(*SETS[name])
    got = diagnose.evaluate_errors(bl, gt, score_thresh=0.625, bg_thresh=0.25, device=dev)
    _check(got, _twin(name, score_thresh=0.625, bg_thresh=0.25))
    assert (got["det_kind"] != _twin(name)["det_kind"]).any()      # the background threshold moved some detections


def _merged():
    preds = SETS["random"][0] + SETS["size"][0] + HAND["rescale"]["preds"]
    gts = SETS["random"][1] + SETS["size"][1] + HAND["rescale"]["gts"]
    return preds, gts


def test_tp_is_the_evaluations_match_and_the_base_row_its_ap(dev):
    preds, gts = _merged()
    bl, gt = vid_twin.to_boxlists(preds, gts)
    st = diagnose._run(bl, gt, None, 0.1, dev)
    t, meta = st["t"], st["meta"]
    ranges = torch.tensor([[0.0, 1.0, 0.0]], dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        match = ops.vid_eval_match(t["det_box"], t["det_label"], t["det_off"], st["order"], t["ratio"], t["gt_box"],
                                   t["gt_label"], None, t["gt_off"], ranges, meta["C"], meta["max_gt"])[0]
    kind = st["out"]["det_kind"]
    assert torch.equal(kind == 0, match[0] == 1) and int((kind == 0).sum()) > 100
    got = diagnose.evaluate_errors(bl, gt, device=dev)
    ref = vid_eval.match_and_ap(bl, gt, None, device=dev)
    np.testing.assert_array_equal(got["ap"], ref["ap"][0])          # the same kernel on the same rows: the same bits
    np.testing.assert_array_equal(got["det_kind"] == 0, ref["match"][0] == 1)
    res = vid_eval.evaluate_detections(bl, gt, device=dev)
    assert got["map"] == res[0]["map"] or (np.isnan(got["map"]) and np.isnan(res[0]["map"]))


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_every_output_element_is_written(dev, fill):
    preds, gts = _merged()
    bl, gt = vid_twin.to_boxlists(preds, gts)
    st = diagnose._run(bl, gt, None, 0.1, dev)
    t, meta = st["t"], st["meta"]
    N, G = meta["N"], t["gt_label"].shape[0]
    out = (torch.empty(N, dtype=torch.uint8, device=dev), torch.empty(N, dtype=torch.int32, device=dev),
           torch.empty(N, dtype=torch.float32, device=dev), torch.empty((3, G), dtype=torch.int32, device=dev))
    for o in out:
        o.view(torch.uint8).fill_(fill)
    with torch.cuda.device(dev):
        got = ops.diagnose_match(t["det_box"], t["det_label"], t["score"], t["det_off"], st["order"], t["ratio"],
                                 t["gt_box"], t["gt_label"], t["gt_off"], meta["C"], meta["max_gt"], 0.1, out=out)
    assert all(a is b for a, b in zip(got, out))
    for a, b in zip(got, (st["out"][k] for k in ("det_kind", "det_gt", "det_iou", "gt_det"))):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))            # the same bytes as into fresh tensors
    want = diagnose_twin.classify(preds, gts)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a.cpu().numpy().view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def test_motion_cross_tabulation(dev):
    # the small table: 0.7 counts as fast and as medium; the second frame has no list and falls in no range
    p, g = diagnose_cases.frame([(diagnose_cases.NEAR, 0.9, 1)], [(diagnose_cases.A, 1), (diagnose_cases.FAR, 1)])
    bl, gt = vid_twin.to_boxlists([p, p], [g, g])
    motion = [[0.7, 0.95], []]
    got = diagnose.evaluate_errors(bl, gt, motion_iou=motion, device=dev)
    assert got["motion"]["gt_state_counts"].tolist() == [[0, 1, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]]
    assert got["motion"]["kind_counts"].tolist() == [[0, 1, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0]]
    _check(got, diagnose_twin.run([p, p], [g, g], motion=motion))
    # the random frames with a table that hits 0.7 and 0.9 and leaves frames without a list
    motion = diagnose_cases.motion_table(SETS["random"][1])
    assert any(len(m) == 0 for m in motion) and any(0.7 in m for m in motion) and any(0.9 in m for m in motion)
    bl, gt = vid_twin.to_boxlists(*SETS["random"])
    got = diagnose.evaluate_errors(bl, gt, motion_iou=motion, device=dev)
    want = _twin("random", motion=motion)
    _check(got, want)
    assert got["text"] == want["text"] and "motion=  fast" in got["text"]


def test_result_file_equals_the_twins_text(dev, tmp_path):
    bl, gt = vid_twin.to_boxlists(*SETS["random"])
    got = diagnose.evaluate_errors(bl, gt, output_folder=str(tmp_path / "out"), device=dev)
    text = (tmp_path / "out" / "result_diagnosis.txt").read_text()
    assert text == got["text"] == _twin("random")["text"]
    assert text.startswith("mAP = ") and text.count("\n") == 10 and "motion" not in text
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["result_diagnosis.txt"]


def _xml(h, w, objs):
    s = "<annotation><size><width>%d</width><height>%d</height></size>" % (w, h)
    for name, (x1, y1, x2, y2) in objs:
        s += ("<object><name>%s</name><bndbox><xmax>%d</xmax><xmin>%d</xmin><ymax>%d</ymax><ymin>%d</ymin></bndbox>"
              "</object>" % (name, x2, x1, y2, y1))
    return s + "</annotation>"


def test_inference_writes_the_diagnosis_and_leaves_result_txt(dev, tmp_path):
    """The tiny synthetic loop of tests/test_vid_eval_gpu.py: image files -> inference(..., anno_path=..., diagnose=True)
    -> result_diagnosis.txt == the twin's text on the returned predictions; result.txt is the evaluation's, as without."""
    from PIL import Image
    from mega.pytorch_amd import config, inference, modeling, synth
    T, H0, W0 = 12, 90, 160
    clip0 = synth.make_clip(T, H0, W0, seed=8).numpy()
    os.makedirs(str(tmp_path / "Data" / "v"))
    os.makedirs(str(tmp_path / "Anno" / "v"))
    rng = np.random.default_rng(5)
    lines, motion = [], []
    for t in range(T):
        Image.fromarray(clip0[t]).save(str(tmp_path / "Data" / "v" / ("%06d.JPEG" % t)), format="PNG")
        lines.append("v %d %d %d" % (t + 1, t, T))
        g = int(rng.integers(0, 5))
        objs = []
        for _ in range(g):
            x1, y1 = int(rng.integers(0, 120)), int(rng.integers(0, 60))
            objs.append((vid_eval.CLASSES_MAP[int(rng.integers(1, 31))],
                         (x1, y1, x1 + int(rng.integers(8, 60)), y1 + int(rng.integers(8, 40)))))
        (tmp_path / "Anno" / "v" / ("%06d.xml" % t)).write_text(_xml(H0, W0, objs))
        motion.append(np.asarray(rng.choice([0.2, 0.7, 0.8, 0.95], g), np.float64) if g else np.zeros(1))
    (tmp_path / "index.txt").write_text("\n".join(lines) + "\n")
    cfg = config.get_cfg("R-50")
    cfg.MODEL.DEVICE = str(dev)
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 180, 320
    model = modeling.build_detection_model(cfg)
    model.load_state_dict(synth.make_state_dict(blocks=(3, 4, 6), reduce_channel=True, global_res_stage=0, seed=1))
    model.to(dev)
    out = tmp_path / "out"
    preds = inference.inference(cfg, model, str(tmp_path / "Data"), str(tmp_path / "index.txt"), output_folder=str(out),
                                steps_per_batch=4, anno_path=str(tmp_path / "Anno"), motion_iou=motion,
                                diagnose={"score_thresh": 0.05})
    assert len(preds) == T and sum(len(p) for p in preds) > 0
    gt = vid_eval.VIDGroundTruth(str(tmp_path / "index.txt"), str(tmp_path / "Anno"))
    tp, tg = vid_twin.from_boxlists(preds, gt)
    want = vid_twin.evaluate(tp, tg, [list(m) for m in motion])
    assert (out / "result.txt").read_text() == vid_eval.format_result({i: {"ap": w["ap"], "map": w["map"]}
                                                                      for i, w in enumerate(want)})
    twin = diagnose_twin.run(tp, tg, motion=[list(m) for m in motion], score_thresh=0.05)
    assert (out / "result_diagnosis.txt").read_text() == twin["text"]
    assert twin["kind_counts"].sum() == sum(len(p) for p in preds)
    assert sorted(os.listdir(str(out))) == ["predictions.pth", "result.txt", "result_diagnosis.txt"]
