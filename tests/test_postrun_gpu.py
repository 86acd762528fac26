"""GPU: one inference() run with every stage of the chain after the detections on (mega/pytorch_amd/postrun.py), and
tools/eval_vid.py with the same options on its predictions.pth: the two folders hold the same files, and each file is the
direct call of its stage's module on the stage's input.  No tolerance anywhere."""
import importlib.util
import os

import pytest
import torch

from mega.pytorch_amd import diagnose, motion_iou, seq_nms, track_eval, tracks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
TEXTS = ("result.txt", "result_diagnosis.txt", "result_seq_nms.txt", "tracks.txt", "result_tracks.txt", "result_tubelets.txt")
LISTS = ("predictions.pth", "predictions_seq_nms.pth", "predictions_tracks.pth")


def _assert_same_lists(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.size == w.size and g.mode == w.mode and sorted(g.fields()) == sorted(w.fields())
        assert g.bbox.dtype == w.bbox.dtype and torch.equal(g.bbox.cpu(), w.bbox.cpu())
        for k in w.fields():
            assert g.get_field(k).dtype == w.get_field(k).dtype and torch.equal(g.get_field(k).cpu(), w.get_field(k).cpu()), k


def test_inference_and_the_tool_run_the_same_chain(dev, tmp_path, capsys):
    from PIL import Image
    from mega.pytorch_amd import config, inference, modeling, synth, vid_eval
    from test_track_eval import _xml
    T, H0, W0 = 12, 90, 160
    clip0 = synth.make_clip(T, H0, W0, seed=8).numpy()
    os.makedirs(str(tmp_path / "Data" / "v"))
    os.makedirs(str(tmp_path / "Anno" / "v"))
    lines = []
    for t in range(T):
        Image.fromarray(clip0[t]).save(str(tmp_path / "Data" / "v" / ("%06d.JPEG" % t)), format="PNG")
        lines.append("v %d %d %d" % (t + 1, t, T))
        objs = [(vid_eval.CLASSES_MAP[3], 0, (10 + 2 * t, 10, 60 + 2 * t, 50)), (vid_eval.CLASSES_MAP[7], 1, (80, 20, 140, 80))]
        (tmp_path / "Anno" / "v" / ("%06d.xml" % t)).write_text(_xml(H0, W0, objs))
    index, anno = str(tmp_path / "index.txt"), str(tmp_path / "Anno")
    (tmp_path / "index.txt").write_text("\n".join(lines) + "\n")
    cfg = config.get_cfg("R-50")
    cfg.MODEL.DEVICE = str(dev)
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 180, 320
    model = modeling.build_detection_model(cfg)
    model.load_state_dict(synth.make_state_dict(blocks=(3, 4, 6), reduce_channel=True, global_res_stage=0, seed=1))
    model.to(dev)
    lib, cli = tmp_path / "lib", tmp_path / "cli"
    link_kw = {"score_thresh": 0.0, "link_iou": 0.3, "max_gap": 2, "rescore": "avg"}
    returned = inference.inference(cfg, model, str(tmp_path / "Data"), index, output_folder=str(lib), steps_per_batch=4,
                                   anno_path=anno, seq_nms=True, diagnose=True, motion_iou="derive",
                                   tracks=dict(link_kw, fill=True, smooth=1, tubelet_ap=True))
    spec = importlib.util.spec_from_file_location("eval_vid_tool", os.path.join(ROOT, "tools", "eval_vid.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    capsys.readouterr()
    assert tool.main(["--predictions", str(lib / "predictions.pth"), "--img-index", index, "--anno-path", anno,
                      "--output-folder", str(cli), "--device", str(dev), "--seq-nms", "--tracks", "--tracks-score-thresh", "0",
                      "--tracks-link-iou", "0.3", "--tracks-max-gap", "2", "--tracks-rescore", "avg", "--tracks-fill",
                      "--tracks-smooth", "1", "--tubelet-ap", "--diagnose", "--motion-iou", "derive"]) == 0
    printed = capsys.readouterr().out
    # the two front ends wrote the same
    assert sorted(os.listdir(str(lib))) == sorted(TEXTS + LISTS)
    assert sorted(os.listdir(str(cli))) == sorted(TEXTS + LISTS[1:])
    text = {}
    for name in TEXTS:
        text[name] = (lib / name).read_bytes()
        assert (cli / name).read_bytes() == text[name] != b"", name
    saved = {name: inference.load_predictions(str(lib / name)) for name in LISTS}
    for name in LISTS[1:]:
        _assert_same_lists(inference.load_predictions(str(cli / name)), saved[name])
    # and each file is its stage's own call on the stage's input
    raw, videos = saved["predictions.pth"], [(0, T)]
    rescored = seq_nms.seq_nms(raw, videos, device=dev)
    _assert_same_lists(saved["predictions_seq_nms.pth"], rescored)
    _assert_same_lists(returned, rescored)                       # inference() returns the rescored list
    linked, table = tracks.link(rescored, videos, device=dev, **link_kw)
    assert text["tracks.txt"].decode() == tracks.format_table(table) and len(table) > 0
    refined, info = tracks.refine(linked, videos, fill=True, smooth=1, device=dev)
    print("boxes: %d raw, %d kept by Seq-NMS; %d tracks, %d boxes filled"
          % (sum(len(p) for p in raw), sum(len(p) for p in rescored), len(table), info["filled"]))
    _assert_same_lists(saved["predictions_tracks.pth"], refined)
    assert all(sorted(p.fields()) == ["filled", "labels", "scores", "track_ids"] for p in refined)
    gt = vid_eval.VIDTrackGroundTruth(index, anno)
    motion = motion_iou.derive(gt, videos, motion_iou.WINDOW, device=dev)

    def ap_text(preds):
        return vid_eval.format_result(vid_eval.evaluate_detections(preds, gt, motion_iou=motion, device=dev)).encode()
    assert text["result.txt"] == ap_text(raw)
    assert [l.split("=")[1].strip() for l in text["result.txt"].decode().splitlines()[:4]] == ["all", "fast", "medium", "slow"]
    assert text["result_seq_nms.txt"] == ap_text(rescored) and text["result_tracks.txt"] == ap_text(refined)
    assert text["result_diagnosis.txt"] == diagnose.evaluate_errors(raw, gt, motion_iou=motion, device=dev)["text"].encode()
    assert text["result_tubelets.txt"] == track_eval.evaluate_tracks(refined, gt, videos, device=dev)["text"].encode()
    # what the tool printed: every text under its header, in the chain's order
    assert printed == "".join([text["result.txt"].decode(), "Diagnosis:\n", text["result_diagnosis.txt"].decode(), "Seq-NMS:\n",
                               text["result_seq_nms.txt"].decode(), "Tracks: %d\n" % len(table),
                               "Filled boxes: %d\n" % info["filled"], "Tracks, rescored and refined:\n",
                               text["result_tracks.txt"].decode(), "Tubelets:\n", text["result_tubelets.txt"].decode()])
