"""GPU: the VID evaluation kernels (csrc/vid_eval.hip) against the numpy twin (tests/vid_twin.py) and the reference's
recorded outputs (tests/golden/ref_vid_eval.npz), and the evaluation at the end of inference() / tools/eval_vid.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import vid_twin
from mega.pytorch_amd import vid_eval

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytestmark = pytest.mark.gpu


def _check_against_twin(preds, gts, motion, dev):
    bl, gt = vid_twin.to_boxlists(preds, gts)
    got = vid_eval.match_and_ap(bl, gt, motion, device=dev)
    want = vid_twin.evaluate(preds, gts, motion)
    assert got["ap"].shape == (len(want), len(want[0]["ap"]))
    for ri, w in enumerate(want):
        np.testing.assert_array_equal(got["match"][ri], w["match"])
        np.testing.assert_array_equal(got["pred_ignore"][ri], w["pred_ignore"])
        np.testing.assert_array_equal(got["n_pos"][ri], w["n_pos"])
        np.testing.assert_allclose(got["ap"][ri], w["ap"], rtol=0, atol=1e-12 if motion is None else 1e-9, equal_nan=True)
    return got, want


@pytest.mark.parametrize("motion", [True, False])
def test_kernels_equal_twin_with_ties_and_large_frames(dev, motion):
    preds, gts, mot = vid_twin.make_frames(7, F=60, tie_scores=True, motion=motion)
    # frames with more than 64 GT boxes (several chunks of lanes) and more than 1024 predictions
    p2, g2, m2 = vid_twin.make_frames(8, F=3, max_det=1600, min_det=1100, max_gt=150, min_gt=70, tie_scores=True,
                                      motion=motion, special=False)
    preds, gts = preds + p2, gts + g2
    mot = mot + m2 if motion else None
    assert max(len(g["label"]) for g in gts) > 64 and max(len(p["score"]) for p in preds) > 1024
    assert any(len(np.unique(p["score"])) < len(p["score"]) for p in preds)       # ties within frames
    _check_against_twin(preds, gts, mot, dev)


def test_kernels_equal_twin_on_distinct_scores(dev):
    preds, gts, mot = vid_twin.make_frames(11, F=120)
    _check_against_twin(preds, gts, mot, dev)


def _golden(z):
    sys.path.insert(0, HERE)
    from test_vid_eval import golden_frames
    return golden_frames(z)


@pytest.mark.parametrize("case", ["motion", "nomotion"])
def test_golden_through_evaluate_detections(dev, tmp_path, case):
    z = np.load(os.path.join(HERE, "golden", "ref_vid_eval.npz"))
    preds, gts, motion = _golden(z)
    bl, gt = vid_twin.to_boxlists(preds, gts)
    mot = [np.asarray(m, np.float64) for m in motion] if case == "motion" else None
    res = vid_eval.evaluate_detections(bl, gt, motion_iou=mot, output_folder=str(tmp_path), device=dev)
    R = 4 if case == "motion" else 1
    assert sorted(res.keys()) == list(range(R))
    ref = {}
    for ri in range(R):
        want = z["%s_r%d_ap" % (case, ri)]
        np.testing.assert_allclose(res[ri]["ap"], want, rtol=0, atol=1e-12 if case == "nomotion" else 1e-9, equal_nan=True)
        ref[ri] = {"ap": want, "map": np.nanmean(want)}
    text = (tmp_path / "result.txt").read_text()
    assert text == vid_eval.format_result(ref)
    assert text.startswith("AP50 | motion=   all = ") and "Category AP:\n" in text


def test_large_set_equals_twin(dev):
    """~20k frames x 300 detections, one range (the twin's Python loops bound the size)."""
    rng = np.random.default_rng(3)
    F, D = 20000, 300
    preds, gts = [], []
    for f in range(F):
        H, W = 375, 500
        g = int(rng.integers(0, 6))
        gl = rng.integers(1, 31, g)
        x1, y1 = rng.uniform(0, 350, g), rng.uniform(0, 250, g)
        gb = np.round(np.stack([x1, y1, x1 + rng.uniform(10, 140, g), y1 + rng.uniform(10, 120, g)], 1)).astype(np.float32)
        n = D
        src = rng.integers(0, max(g, 1), n)
        jit = gb[src] + rng.normal(0, 8, (n, 4)) if g else rng.uniform(0, 400, (n, 4))
        box = np.sort(np.asarray(jit, np.float32).reshape(n, 2, 2), axis=1).reshape(n, 4)
        box = np.clip(box, 0, 499).astype(np.float32)
        lab = np.where(rng.random(n) < 0.5, gl[src] if g else rng.integers(1, 31, n), rng.integers(1, 31, n))
        preds.append({"box": box * np.float32(1.6), "score": rng.random(n).astype(np.float32), "label": lab,
                      "size": (800, 600)})
        gts.append({"box": gb.reshape(-1, 4), "label": gl, "im_info": (H, W)})
    bl, gt = vid_twin.to_boxlists(preds, gts)
    got = vid_eval.match_and_ap(bl, gt, None, device=dev)
    want = vid_twin.evaluate(preds, gts, None)[0]
    np.testing.assert_array_equal(got["match"][0], want["match"])
    np.testing.assert_array_equal(got["pred_ignore"][0], want["pred_ignore"])
    np.testing.assert_array_equal(got["n_pos"][0], want["n_pos"])
    np.testing.assert_allclose(got["ap"][0], want["ap"], rtol=0, atol=1e-12, equal_nan=True)


def _xml(h, w, objs):
    s = "<annotation><size><width>%d</width><height>%d</height></size>" % (w, h)
    for name, (x1, y1, x2, y2) in objs:
        s += ("<object><name>%s</name><bndbox><xmax>%d</xmax><xmin>%d</xmin><ymax>%d</ymax><ymin>%d</ymin></bndbox>"
              "</object>" % (name, x2, x1, y2, y1))
    return s + "</annotation>"


def test_inference_with_annotations_writes_result_and_cli_agrees(dev, tmp_path):
    """image files -> inference(..., anno_path=..., motion_iou=...) -> result.txt == the twin's evaluation of the returned
    predictions; tools/eval_vid.py on the saved predictions.pth writes the same result.txt."""
    from PIL import Image
    import scipy.io as sio
    from mega.pytorch_amd import config, inference, modeling, synth
    T, H0, W0 = 12, 90, 160
    clip0 = synth.make_clip(T, H0, W0, seed=8).numpy()
    os.makedirs(str(tmp_path / "Data" / "v"))
    os.makedirs(str(tmp_path / "Anno" / "v"))
    rng = np.random.default_rng(5)
    lines, motion = [], np.empty((T, 1), dtype=object)
    for t in range(T):
        Image.fromarray(clip0[t]).save(str(tmp_path / "Data" / "v" / ("%06d.JPEG" % t)), format="PNG")
        lines.append("v %d %d %d" % (t + 1, t, T))
        g = int(rng.integers(0, 5))
        objs = []
        for _ in range(g):
            x1, y1 = int(rng.integers(0, 120)), int(rng.integers(0, 60))
            objs.append((vid_eval.CLASSES_MAP[int(rng.integers(1, 31))],
                         (x1, y1, x1 + int(rng.integers(8, 60)), y1 + int(rng.integers(8, 40)))))
        objs.append(("n00000000", (1, 1, 20, 20)))          # unknown wnid: dropped
        (tmp_path / "Anno" / "v" / ("%06d.xml" % t)).write_text(_xml(H0, W0, objs))
        motion[t, 0] = rng.uniform(0, 1, (g, 1)) if g else np.zeros((1, 0))
    (tmp_path / "index.txt").write_text("\n".join(lines) + "\n")
    sio.savemat(str(tmp_path / "motion.mat"), {"motion_iou": motion})
    cfg = config.get_cfg("R-50")
    cfg.MODEL.DEVICE = str(dev)
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 180, 320
    model = modeling.build_detection_model(cfg)
    model.load_state_dict(synth.make_state_dict(blocks=(3, 4, 6), reduce_channel=True, global_res_stage=0, seed=1))
    model.to(dev)
    out = tmp_path / "out"
    preds = inference.inference(cfg, model, str(tmp_path / "Data"), str(tmp_path / "index.txt"), output_folder=str(out),
                                steps_per_batch=4, anno_path=str(tmp_path / "Anno"), motion_iou=str(tmp_path / "motion.mat"))
    assert len(preds) == T and sum(len(p) for p in preds) > 0
    text = (out / "result.txt").read_text()
    gt = vid_eval.VIDGroundTruth(str(tmp_path / "index.txt"), str(tmp_path / "Anno"))
    mot = vid_eval.load_motion_iou(str(tmp_path / "motion.mat"))
    tp, tg = vid_twin.from_boxlists(preds, gt)
    want = vid_twin.evaluate(tp, tg, mot)
    assert text == vid_eval.format_result({i: {"ap": w["ap"], "map": w["map"]} for i, w in enumerate(want)})
    # the command-line tool on the saved predictions.pth
    cli_out = tmp_path / "cli"
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_vid.py"), "--predictions",
                        str(out / "predictions.pth"), "--img-index", str(tmp_path / "index.txt"), "--anno-path",
                        str(tmp_path / "Anno"), "--motion-iou", str(tmp_path / "motion.mat"), "--output-folder",
                        str(cli_out), "--device", str(dev)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert (cli_out / "result.txt").read_text() == text
