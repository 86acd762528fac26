"""CPU: the VID proposal recall's definition (tests/proposal_recall_twin.py) against the reference's own results
(tests/golden/ref_proposal_recall.npz, written by the unmodified do_vid_evaluation(box_only=True)), its tie rules, the host-side
errors of vid_eval.evaluate_proposals, and MODEL.RPN_ONLY through the config, the detectors (on the CPU twins) and
inference()'s argument checks.  The kernel itself is tested in test_proposal_recall_gpu.py."""
import os
import types

import numpy as np
import pytest
import torch

import cpu_ops
import proposal_recall_twin as twin
from mega.pytorch_amd import config, inference, modeling, synth, vid_eval
from mega.pytorch_amd.structures import BoxList

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_proposal_recall.npz")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_twin_equals_reference_fixture():
    z = np.load(GOLDEN, allow_pickle=False)
    preds, gts = twin.from_fixture(z)
    per_frame = [twin.match_frame(p, g, 300)[0] for p, g in zip(preds, gts)]
    # the reference collects the overlaps of the frames that have both GT boxes and proposals (vid_eval.py:88-92), sorted
    got = np.sort(np.concatenate([o for o, p in zip(per_frame, preds) if len(p["obj"])]))
    want = z["ref_gt_overlaps_sorted"]
    assert got.shape == want.shape
    np.testing.assert_array_equal(_bits(got), _bits(want))
    ov = np.concatenate(per_frame)
    assert len(ov) == int(z["ref_num_pos"])                 # num_pos counts every GT box
    rec = twin.recall(ov)
    assert rec.dtype == np.float32 and _bits(rec) == _bits(z["ref_recall"])
    assert twin.result_text(rec) == str(z["ref_text"])
    # the cases the fixture is there for
    n = np.diff(z["pred_off"])
    g = np.diff(z["gt_off"])
    assert ((g == 0) & (n > 0)).any() and ((n == 0) & (g > 0)).any() and ((g > n) & (n > 0)).any() and (n > 300).any()


def _frame(boxes, obj, gt, size=(100, 100)):
    return ({"box": np.asarray(boxes, np.float32).reshape(-1, 4), "obj": np.asarray(obj, np.float32), "size": size},
            {"box": np.asarray(gt, np.float32).reshape(-1, 4), "im_info": (size[1], size[0])})


def test_tie_rules_on_hand_made_cases():
    A, B = [0, 0, 9, 9], [50, 50, 59, 59]
    # 2 x 2, every IoU equal (two identical proposals, two identical GT boxes): round 1 takes GT 0 with proposal 0
    p, g = _frame([A, A], [0.9, 0.8], [A, A])
    ov, pr = twin.match_frame(p, g, 300)
    assert ov.tolist() == [1.0, 1.0] and pr.tolist() == [0, 1]
    # equal IoUs in one column: the lower proposal position, i.e. the higher objectness, wins; GT 1 gets what is left
    p, g = _frame([A, A], [0.2, 0.7], [A, B])
    ov, pr = twin.match_frame(p, g, 300)
    assert ov.tolist() == [1.0, 0.0] and pr.tolist() == [0, 1]          # positions in objectness order
    # tied objectness keeps ascending position
    p, g = _frame([B, A], [0.5, 0.5], [A])
    ov, pr = twin.match_frame(p, g, 300)
    assert ov.tolist() == [1.0] and pr.tolist() == [1]
    # 3 x 2: the global maximum goes first, even when it takes a lower GT's best proposal
    C = [0, 0, 9, 4]                                                    # IoU(A, C) = 0.5
    p, g = _frame([A, C, B], [0.9, 0.8, 0.7], [C, A])
    ov, pr = twin.match_frame(p, g, 300)
    assert ov.tolist() == [1.0, 1.0] and pr.tolist() == [1, 0]
    p, g = _frame([A, B, B], [0.9, 0.8, 0.7], [C, A])                   # A goes to GT 1 (IoU 1), GT 0 is left with IoU 0
    ov, pr = twin.match_frame(p, g, 300)
    assert ov.tolist() == [0.0, 1.0] and pr.tolist() == [1, 0]
    # the limit cuts in objectness order; more GT boxes than proposals leaves the rest at 0 / -1
    p, g = _frame([A, B], [0.1, 0.9], [A, B])
    ov, pr = twin.match_frame(p, g, 1)
    assert ov.tolist() == [0.0, 1.0] and pr.tolist() == [-1, 0]
    assert np.isnan(twin.recall(np.zeros(0, np.float32)))


def _boxlists(with_objectness=True):
    preds, gts = twin.make_frames(3, F=4, special=False)
    bl, gt = twin.to_boxlists(preds, gts)
    if not with_objectness:
        for b in bl:
            b.extra_fields.pop("objectness")
            b.add_field("scores", torch.zeros(len(b)))
    return bl, gt


def test_host_side_errors():
    bl, gt = _boxlists()
    with pytest.raises(RuntimeError, match=r"runs on a HIP device \(no CPU path\)"):
        vid_eval.evaluate_proposals(bl, gt, device="cpu")
    with pytest.raises(ValueError, match="limit 1025"):
        vid_eval.evaluate_proposals(bl, gt, limit=1025)
    with pytest.raises(ValueError, match="limit 2000"):
        vid_eval.evaluate_proposals(bl, gt, limits=(10, 2000))
    with pytest.raises(ValueError, match="thresholds must be > 0"):
        vid_eval.evaluate_proposals(bl, gt, iou_thresh=0.0)
    with pytest.raises(ValueError, match="thresholds must be > 0"):
        vid_eval.evaluate_proposals(bl, gt, iou_thresholds=(0.5, -0.1))
    with pytest.raises(ValueError, match="objectness"):
        vid_eval.evaluate_proposals(_boxlists(False)[0], gt)
    bl[1].bbox[0, 0] = float("inf")
    with pytest.raises(ValueError, match="not finite"):
        vid_eval.evaluate_proposals(bl, gt)
    bl, gt = _boxlists()
    bl[1].get_field("objectness")[0] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        vid_eval.evaluate_proposals(bl, gt)
    bl, gt = _boxlists()
    with pytest.raises(ValueError, match="need to be same"):
        vid_eval.evaluate_proposals(bl[:-1], gt)


def test_box_only_of_evaluate_detections_points_to_evaluate_proposals():
    bl, gt = _boxlists()
    with pytest.raises(NotImplementedError, match="evaluate_proposals"):
        vid_eval.evaluate_detections(bl, gt, box_only=True)


def test_recall_table_text():
    t = vid_eval.format_recall_table([10, 300], [0.5, 0.75], np.float32([[0.25, 0.125], [1.0, 0.5]]),
                                     np.float32([0.1875, 0.75]), 8)
    assert t == ("Proposal recall, 8 GT boxes\n"
                 " limit     AR  @0.50  @0.75\n"
                 "    10 0.1875 0.2500 0.1250\n"
                 "   300 0.7500 1.0000 0.5000\n")
    assert vid_eval.PROPOSAL_LIMITS == (10, 50, 100, 300)
    assert vid_eval.PROPOSAL_IOU_THRESHOLDS == (0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95)


def test_config_has_rpn_only_off():
    for method in ("mega", "rdn", "fgfa", "dff", "base"):
        cfg = config.get_cfg("R-50", method)
        assert cfg.MODEL.RPN_ONLY is False
        assert modeling.rpn_only(cfg) is False


def test_inference_refuses_rpn_only_with_seq_nms_or_bbox_aug(tmp_path):
    cfg = config.get_cfg("R-50", "base")
    cfg.MODEL.RPN_ONLY = True
    model = types.SimpleNamespace(cfg=cfg)
    with pytest.raises(ValueError, match="Seq-NMS"):
        inference.inference(cfg, model, str(tmp_path), str(tmp_path / "index.txt"), device="cpu", seq_nms=True)
    with pytest.raises(ValueError, match="Seq-NMS"):
        inference.inference(cfg, model, str(tmp_path), str(tmp_path / "index.txt"), device="cpu", seq_nms={"link_iou": 0.5})
    cfg.TEST.BBOX_AUG.ENABLED = True
    cfg.TEST.BBOX_AUG.H_FLIP = True
    with pytest.raises(ValueError, match="BBOX_AUG"):
        inference.inference(cfg, model, str(tmp_path), str(tmp_path / "index.txt"), device="cpu")


def _assert_is_own_rpn(out, model, frame):
    il_feats = model.backbone(frame[None])
    want = model.rpn(frame[None], il_feats, None)[0][0]
    assert isinstance(out, list) and len(out) == 1 and isinstance(out[0], BoxList)
    got = out[0]
    assert sorted(got.fields()) == ["objectness"] and got.size == want.size == (frame.shape[2], frame.shape[1])
    assert len(got) == len(want) > 0
    assert torch.equal(got.bbox, want.bbox) and torch.equal(got.get_field("objectness"), want.get_field("objectness"))
    obj = got.get_field("objectness")
    assert bool((obj[:-1] >= obj[1:]).all())          # the keep order is descending objectness already (rpn.py:193-196)


def test_rpn_only_base_forward_is_the_models_own_rpn(monkeypatch):
    cpu_ops.install(monkeypatch)
    cfg = config.get_cfg("R-50", "base")
    cfg.MODEL.DEVICE = "cpu"
    cfg.MODEL.RPN_ONLY = True
    cfg.MODEL.RPN.POST_NMS_TOP_N_TEST = 40
    sd = {k: v for k, v in synth.make_fgfa_state_dict(seed=3).items() if not k.startswith(("flownet.", "embednet."))}
    model = modeling.build_detection_model(cfg)
    model.load_state_dict(sd)          # strict: roi_heads is still built
    frames = synth.preprocess_cpu(synth.make_clip(1, 64, 96, seed=6))
    with torch.no_grad():
        _assert_is_own_rpn(model(frames[0]), model, frames[0])


def test_rpn_only_dff_forward_and_engine_return_proposals(monkeypatch):
    from mega.pytorch_amd import fgfa as fgfa_mod
    cpu_ops.install(monkeypatch)
    cfg = config.get_cfg("R-50", "dff")
    cfg.MODEL.DEVICE = "cpu"
    cfg.MODEL.RPN_ONLY = True
    cfg.MODEL.RPN.POST_NMS_TOP_N_TEST = 40
    model = modeling.build_detection_model(cfg)
    model.load_state_dict(synth.make_dff_state_dict(seed=3))
    frames = synth.preprocess_cpu(synth.make_clip(3, 64, 96, seed=6))
    with torch.no_grad():
        ref = [model(inference.frame_feed(cfg, frames, i))[0] for i in range(3)]
        got = fgfa_mod.DffClipEngine(model, interval=10, lookahead=2, graphs=False).run(frames)
    assert len(got) == 3
    for r, g in zip(ref, got):
        assert sorted(r.fields()) == sorted(g.fields()) == ["objectness"] and g.size == (96, 64)
        # (the twins' GEMMs are not batch-invariant to the last bit; the GPU test asks for equal bits)
        assert abs(len(r) - len(g)) <= 2 and len(g) > 0
        n = min(len(r), len(g), 5)
        assert (r.bbox[:n] - g.bbox[:n]).abs().max() < 0.05


def test_rpn_only_mega_forward_needs_the_key_frame_only(monkeypatch):
    cpu_ops.install(monkeypatch)
    cfg = config.get_cfg("R-50", "mega")
    cfg.MODEL.DEVICE = "cpu"
    cfg.MODEL.RPN_ONLY = True
    cfg.MODEL.RPN.POST_NMS_TOP_N_TEST = 80
    model = modeling.build_detection_model(cfg)
    model.load_state_dict(synth.make_state_dict(blocks=(3, 4, 6), reduce_channel=True, global_res_stage=0, seed=1))
    frames = synth.preprocess_cpu(synth.make_clip(1, 64, 96, seed=6))
    with torch.no_grad():
        out = model({"cur": frames[0], "frame_category": 1})          # no window, no reference frames
        _assert_is_own_rpn(out, model, frames[0])
