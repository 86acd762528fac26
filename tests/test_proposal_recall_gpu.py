"""GPU: the proposal-recall kernel (csrc/proposal_recall.hip) against its numpy twin bit for bit, the reference's fixture
through vid_eval.evaluate_proposals and tools/eval_vid.py --box-only, and MODEL.RPN_ONLY through the clip engines and
inference()."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import proposal_recall_twin as twin
from mega.pytorch_amd import vid_eval

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_proposal_recall.npz")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _kernel(preds, gts, limits, dev):
    bl, gt = twin.to_boxlists(preds, gts)
    ov, pr = vid_eval.match_proposals(bl, gt, limits, dev)
    return ov.cpu().numpy(), pr.cpu().numpy()


def _check_against_twin(preds, gts, limits, dev):
    ov, pr = _kernel(preds, gts, limits, dev)
    assert ov.dtype == np.float32 and pr.dtype == np.int32 and ov.shape == pr.shape == (len(limits), sum(len(g["box"]) for g in gts))
    for li, lim in enumerate(limits):
        wov, wpr = twin.match(preds, gts, lim)
        np.testing.assert_array_equal(_bits(ov[li]), _bits(wov), err_msg="gt_overlap, limit %d" % lim)
        np.testing.assert_array_equal(pr[li], wpr, err_msg="gt_prop, limit %d" % lim)
    return ov, pr


def test_kernel_equals_twin_with_tied_objectness_and_tied_ious(dev):
    preds, gts = twin.make_frames(11, F=60, ties=True)
    assert any(len(np.unique(p["obj"])) < len(p["obj"]) for p in preds)
    assert any(len(p["box"]) and len(np.unique(p["box"], axis=0)) < len(p["box"]) for p in preds)
    ov, pr = _check_against_twin(preds, gts, [300], dev)
    assert (pr >= 0).sum() > 100


def _large_frames(seed):
    """3 frames with 70-150 GT boxes (more than one chunk of 64 lanes) and 1100-1600 proposals (more than the 1024 a
    wave holds: the limit cuts them), on a coarse grid so that IoUs tie."""
    rng = np.random.default_rng(seed)
    preds, gts = [], []
    for g, n in ((70, 1100), (129, 1600), (150, 1300)):
        x1, y1 = rng.integers(0, 500, g), rng.integers(0, 300, g)
        gb = np.stack([x1, y1, x1 + rng.integers(8, 140, g), y1 + rng.integers(8, 120, g)], 1).astype(np.float32)
        src = gb[rng.integers(0, g, n)] + np.round(rng.normal(0, 4, (n, 4))).astype(np.float32)
        box = (np.maximum(src, 0) * np.float32([1.25, 1.5, 1.25, 1.5])).astype(np.float32)
        obj = (rng.integers(0, 4000, n) / 4000.0).astype(np.float32)
        preds.append({"box": box, "obj": obj, "size": (800, 600)})
        gts.append({"box": gb, "im_info": (400, 640)})
    return preds, gts


def test_kernel_equals_twin_on_large_frames(dev):
    preds, gts = _large_frames(5)
    ov, pr = _check_against_twin(preds, gts, [300, 1024], dev)
    assert pr[0].max() < 300 and 300 <= pr[1].max() < 1024


def test_kernel_equals_twin_on_edge_frames(dev):
    A, B = np.float32([[10, 10, 50, 40]]), np.float32([[12, 8, 48, 44]])
    none = np.zeros((0, 4), np.float32)
    preds = [{"box": none, "obj": np.zeros(0, np.float32), "size": (100, 80)},                       # P = 0
             {"box": np.concatenate([A, B]), "obj": np.float32([0.3, 0.6]), "size": (100, 80)},        # G = 0
             {"box": B, "obj": np.float32([0.5]), "size": (100, 80)},                                  # P = G = 1
             {"box": np.concatenate([B, A]), "obj": np.float32([0.5, 0.5]), "size": (200, 40)},        # G > P, unequal ratios
             {"box": none, "obj": np.zeros(0, np.float32), "size": (100, 80)}]                         # P = G = 0
    gts = [{"box": np.concatenate([A, B]), "im_info": (80, 100)}, {"box": none, "im_info": (80, 100)},
           {"box": A, "im_info": (80, 100)}, {"box": np.concatenate([A, B, A, A + 30]), "im_info": (80, 100)},
           {"box": none, "im_info": (80, 100)}]
    ov, pr = _check_against_twin(preds, gts, [300], dev)
    assert pr[0].tolist() == [-1, -1, 0] + pr[0][3:].tolist() and sorted(pr[0][3:].tolist()) == [-1, -1, 0, 1]
    assert ov[0, 2] > 0.7 and ov[0, :2].tolist() == [0.0, 0.0]
    # no proposals at all, and no GT boxes at all
    ov, pr = _check_against_twin([preds[0], preds[4]], [gts[0], gts[4]], [300], dev)
    assert ov.tolist() == [[0.0, 0.0]] and pr.tolist() == [[-1, -1]]
    ov, pr = _check_against_twin(preds[1:2], gts[1:2], [300, 10], dev)
    assert ov.shape == (2, 0)


def test_four_limit_launch_equals_four_single_limit_launches(dev):
    preds, gts = twin.make_frames(21, F=30, max_prop=400, ties=True)
    limits = [10, 50, 100, 300]
    ov, pr = _check_against_twin(preds, gts, limits, dev)
    for li, lim in enumerate(limits):
        ov1, pr1 = _kernel(preds, gts, [lim], dev)
        np.testing.assert_array_equal(_bits(ov1[0]), _bits(ov[li]))
        np.testing.assert_array_equal(pr1[0], pr[li])
    assert not np.array_equal(pr[0], pr[3])


def test_golden_through_evaluate_proposals(dev, tmp_path):
    z = np.load(GOLDEN, allow_pickle=False)
    preds, gts = twin.from_fixture(z)
    bl, gt = twin.to_boxlists(preds, gts)
    res = vid_eval.evaluate_proposals(bl, gt, output_folder=str(tmp_path), device=dev)
    assert (tmp_path / "proposal_result.txt").read_bytes() == str(z["ref_text"]).encode()
    assert not (tmp_path / "proposal_recall_table.txt").exists()
    assert res["recall"].dtype == np.float32 and _bits(res["recall"]) == _bits(z["ref_recall"])
    assert res["num_pos"] == int(z["ref_num_pos"])
    has_prop = np.repeat(np.diff(z["pred_off"]) > 0, np.diff(z["gt_off"]))
    np.testing.assert_array_equal(_bits(np.sort(res["gt_overlaps"][has_prop])), _bits(z["ref_gt_overlaps_sorted"]))
    wov, wpr = twin.match(preds, gts, 300)
    np.testing.assert_array_equal(res["gt_prop"], wpr)
    # the table: every limit in one launch; its (300, 0.5) cell is the reference's recall
    res = vid_eval.evaluate_proposals(bl, gt, limits=(10, 50, 100, 300), output_folder=str(tmp_path), device=dev)
    assert res["table"].shape == (4, 10) and res["ar"].shape == (4,) and res["table"].dtype == np.float32
    assert _bits(res["table"][3, 0]) == _bits(z["ref_recall"])
    for li, lim in enumerate(res["limits"]):
        w = twin.match(preds, gts, lim)[0]
        for ti, t in enumerate(res["iou_thresholds"]):
            assert _bits(res["table"][li, ti]) == _bits(twin.recall(w, t)), (lim, t)
    np.testing.assert_array_equal(res["ar"], res["table"].mean(axis=1, dtype=np.float32))
    assert (np.diff(res["table"], axis=1) <= 0).all()
    assert (tmp_path / "proposal_recall_table.txt").read_text() == vid_eval.format_recall_table(
        res["limits"], res["iou_thresholds"], res["table"], res["ar"], res["num_pos"])
    # another threshold and limit
    res = vid_eval.evaluate_proposals(bl, gt, iou_thresh=0.7, limit=20, device=dev)
    assert _bits(res["recall"]) == _bits(twin.recall(twin.match(preds, gts, 20)[0], 0.7))


def _xml(h, w, boxes):
    s = "<annotation><size><width>%d</width><height>%d</height></size>" % (w, h)
    for x1, y1, x2, y2 in boxes:
        s += ("<object><name>n02084071</name><bndbox><xmax>%d</xmax><xmin>%d</xmin><ymax>%d</ymax><ymin>%d</ymin></bndbox>"
              "</object>" % (x2, x1, y2, y1))
    return s + "</annotation>"


def _write_annotations(tmp_path, T, H0, W0, seed=5):
    rng = np.random.default_rng(seed)
    os.makedirs(str(tmp_path / "Anno" / "v"))
    lines = []
    for t in range(T):
        lines.append("v %d %d %d" % (t + 1, t, T))
        boxes = []
        for _ in range(int(rng.integers(0, 5))):
            x1, y1 = int(rng.integers(0, W0 * 3 // 4)), int(rng.integers(0, H0 * 2 // 3))
            boxes.append((x1, y1, x1 + int(rng.integers(8, W0 // 3)), y1 + int(rng.integers(8, H0 // 3))))
        (tmp_path / "Anno" / "v" / ("%06d.xml" % t)).write_text(_xml(H0, W0, boxes))
    (tmp_path / "index.txt").write_text("\n".join(lines) + "\n")


def test_eval_vid_tool_box_only(dev, tmp_path):
    from mega.pytorch_amd import inference
    T = 12
    _write_annotations(tmp_path, T, 90, 160)
    preds, _ = twin.make_frames(9, F=T, special=False)
    for p in preds:
        p["size"] = (320, 180)
        p["box"] = p["box"] * np.float32(0.25)
    gt = vid_eval.VIDGroundTruth(str(tmp_path / "index.txt"), str(tmp_path / "Anno"))
    gts = [{"box": gt.boxes[gt.off[i]:gt.off[i + 1]], "im_info": (90, 160)} for i in range(T)]
    bl, _ = twin.to_boxlists(preds, gts)
    os.makedirs(str(tmp_path / "out"))
    inference.save_predictions(bl, str(tmp_path / "out" / "predictions.pth"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_vid.py"), "--box-only", "--limit", "25",
                        "--recall-table", "--predictions", str(tmp_path / "out" / "predictions.pth"), "--img-index",
                        str(tmp_path / "index.txt"), "--anno-path", str(tmp_path / "Anno"), "--device", str(dev)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ), timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    want = twin.result_text(twin.recall(twin.match(preds, gts, 25)[0]))
    assert (tmp_path / "out" / "proposal_result.txt").read_text() == want
    assert want + "\n" in r.stdout.decode() and "Proposal recall, %d GT boxes" % len(gt.boxes) in r.stdout.decode()
    assert (tmp_path / "out" / "proposal_recall_table.txt").exists()


# ------------------------------------------------------------------------------------------------ MODEL.RPN_ONLY
def _rpn_only_model(dev, method, sd, dtype, strict=True):
    from mega.pytorch_amd import config, modeling
    import mega.pytorch_amd.fgfa  # noqa: F401
    import mega.pytorch_amd.rdn  # noqa: F401
    cfg = config.get_cfg("R-50", method)
    cfg.DTYPE = dtype
    cfg.MODEL.DEVICE = str(dev)
    cfg.MODEL.RPN_ONLY = True
    cfg.NMS_STRICT_GT = True
    m = modeling.build_detection_model(cfg)
    m.load_state_dict(sd, strict=strict)
    m.to(dev)
    return m


def _assert_same_proposals(a, b, tag):
    assert sorted(a.fields()) == sorted(b.fields()) == ["objectness"], tag
    assert a.size == b.size and len(a) == len(b) > 0, (tag, len(a), len(b))
    assert torch.equal(a.bbox.cpu(), b.bbox.cpu()) and torch.equal(a.get_field("objectness").cpu(),
                                                                   b.get_field("objectness").cpu()), tag


@pytest.mark.parametrize("method,dtype,batch_head", [("base", "float32", True), ("base", "bfloat16", False),
                                                     ("dff", "bfloat16", True), ("dff", "float32", False),
                                                     ("fgfa", "bfloat16", True), ("fgfa", "float32", False)])
def test_rpn_only_engine_equals_model(dev, method, dtype, batch_head):
    """the two-graph engines stop after the proposal selection: boxes, objectness and counts of every frame are the bits of
    model.forward (the reference call convention) frame by frame."""
    from mega.pytorch_amd import fgfa as fgfa_mod, inference, synth
    L = {"base": 15, "dff": 24, "fgfa": 24}[method]
    if method == "dff":
        sd = synth.make_dff_state_dict(seed=3)
    else:
        sd = synth.make_fgfa_state_dict(seed=3)
        if method == "base":
            sd = {k: v for k, v in sd.items() if not k.startswith(("flownet.", "embednet."))}
    frames = synth.preprocess_cpu(synth.make_clip(L, 120, 200, seed=7)).to(dev)
    m1, m2 = _rpn_only_model(dev, method, sd, dtype), _rpn_only_model(dev, method, sd, dtype)
    if method == "base":
        eng = fgfa_mod.BaseClipEngine(m2, group=6, batch_head=batch_head)
    elif method == "dff":
        eng = fgfa_mod.DffClipEngine(m2, interval=10, lookahead=2, batch_head=batch_head)
    else:
        eng = fgfa_mod.FgfaClipEngine(m2, lookahead=6, group=2, batch_head=batch_head)
    cut = {"base": 12, "dff": 20, "fgfa": 13}[method]      # (DffClipEngine.run starts on a key frame)
    got = eng.run(frames, first=0, last=cut) + eng.run(frames, first=cut, last=L)      # eager, captured and replayed groups
    assert len(got) == L and eng.replays > 0
    for idx in range(L):
        ref = m1(inference.frame_feed(m1.cfg, frames, idx))[0]
        _assert_same_proposals(ref, got[idx], (method, idx))
        assert got[idx].size == (200, 120)


def test_rpn_only_inference_for_every_method(dev, tmp_path):
    """inference() with MODEL.RPN_ONLY from image files: predictions.pth holds the proposals, proposal_result.txt their
    recall; mega and rdn (through BaseClipEngine) give the bits of the base detector with the same backbone / RPN weights
    (built without the one-frame detectors' split-K of the RPN conv, which MEGA's frame stage never uses) and of their own
    forward()."""
    from PIL import Image
    from mega.pytorch_amd import inference, synth
    T, H0, W0 = 12, 90, 160
    clip0 = synth.make_clip(T, H0, W0, seed=8).numpy()
    os.makedirs(str(tmp_path / "Data" / "v"))
    for t in range(T):
        Image.fromarray(clip0[t]).save(str(tmp_path / "Data" / "v" / ("%06d.JPEG" % t)), format="PNG")
    _write_annotations(tmp_path, T, H0, W0)
    gt = vid_eval.VIDGroundTruth(str(tmp_path / "index.txt"), str(tmp_path / "Anno"))
    sd = synth.make_state_dict(blocks=(3, 4, 6), reduce_channel=True, global_res_stage=0, seed=1)
    shared = {k: v for k, v in sd.items() if k.startswith(("backbone.", "rpn."))}
    results = {}
    for method in ("mega", "rdn", "base"):
        if method == "mega":
            model = _rpn_only_model(dev, method, sd, "bfloat16")
        else:
            model = _rpn_only_model(dev, method, shared, "bfloat16", strict=False)
            model.rpn.head.conv_ksplit = None
        model.cfg.INPUT.MIN_SIZE_TEST, model.cfg.INPUT.MAX_SIZE_TEST = 180, 320
        out = tmp_path / ("out_" + method)
        preds = inference.inference(model.cfg, model, str(tmp_path / "Data"), str(tmp_path / "index.txt"),
                                    output_folder=str(out), anno_path=str(tmp_path / "Anno"), engine_kwargs={"group": 5})
        assert len(preds) == T and all(p.size == (320, 180) for p in preds)
        back = inference.load_predictions(str(out / "predictions.pth"))
        for a, b in zip(back, preds):
            _assert_same_proposals(a, b, method)
        tp = [{"box": p.bbox.numpy(), "obj": p.get_field("objectness").numpy(), "size": p.size} for p in preds]
        tg = [{"box": gt.boxes[gt.off[i]:gt.off[i + 1]], "im_info": (H0, W0)} for i in range(T)]
        assert (out / "proposal_result.txt").read_text() == twin.result_text(twin.recall(twin.match(tp, tg, 300)[0]))
        assert not (out / "result.txt").exists()
        results[method] = preds
        if method != "base":      # the detector's own forward on the resident frames
            src = inference.feed.FrameSource(os.path.join(str(tmp_path / "Data"), "%s.JPEG"), "v/%06d", T, dev,
                                             min_size=180, max_size=320)
            frames = inference.resident_video(src, model.cfg)
            src.close()
            for idx in (0, 7):
                own = model({"cur": frames[idx], "frame_category": 1})[0]
                _assert_same_proposals(own, preds[idx], (method, "forward", idx))
    for method in ("mega", "rdn"):
        for idx, (a, b) in enumerate(zip(results[method], results["base"])):
            _assert_same_proposals(a, b, (method, "vs base", idx))
