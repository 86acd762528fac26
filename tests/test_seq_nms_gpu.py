"""GPU: the Seq-NMS kernel (csrc/seq_nms.hip through mega.pytorch_amd.seq_nms) against the hand-computed cases, the numpy
twin (tests/seq_nms_twin.py) bit for bit, greedy NMS on one-frame videos, and Seq-NMS at the end of inference() /
tools/eval_vid.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seq_nms_cases
import seq_nms_twin
import vid_twin
from mega.pytorch_amd import ops, seq_nms, vid_eval

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
pytestmark = pytest.mark.gpu


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _check(frames, videos, dev, **kw):
    """seq_nms.run (flat) and seq_nms.seq_nms (list[BoxList]) == the twin: keep mask and f32 score bits of every box."""
    preds = seq_nms_twin.to_boxlists(frames)
    r = seq_nms.run(preds, videos, device=dev, **kw)
    keep, new, iters = seq_nms_twin.seq_nms(frames, videos, **kw)
    wk = np.concatenate(keep) if keep else np.zeros(0, bool)
    ws = np.concatenate(new) if new else np.zeros(0, np.float32)
    np.testing.assert_array_equal(r["keep"], wk)
    np.testing.assert_array_equal(_bits(r["scores"][wk]), _bits(ws[wk]))
    out = seq_nms.seq_nms(preds, videos, device=dev, **kw)
    assert len(out) == len(preds)
    for p, o, k, s in zip(preds, out, keep, new):
        assert o.size == p.size and o.mode == p.mode and len(o) == int(k.sum())
        np.testing.assert_array_equal(o.bbox.numpy(), p.bbox.numpy()[k])
        np.testing.assert_array_equal(o.get_field("labels").numpy(), p.get_field("labels").numpy()[k])
        np.testing.assert_array_equal(_bits(o.get_field("scores").numpy()), _bits(s[k]))
    return r, iters


@pytest.mark.parametrize("name", sorted(seq_nms_cases.cases()))
def test_hand_computed_cases(dev, name):
    frames, videos, kw, keep, scores = seq_nms_cases.cases()[name]
    out = seq_nms.seq_nms(seq_nms_twin.to_boxlists(frames), videos, device=dev, **kw)
    assert [len(o) for o in out] == [sum(k) for k in keep]
    for o, e in zip(out, scores):
        np.testing.assert_array_equal(_bits(o.get_field("scores").numpy()), _bits(e))
    _check(frames, videos, dev, **kw)


@pytest.mark.parametrize("kw", [{}, {"rescore": "max"}, {"link_iou": 0.3, "nms_iou": 0.5},
                                {"link_iou": 0.7, "nms_iou": 0.1, "rescore": "max"}, {"link_iou": 0.0, "nms_iou": 1.0}])
def test_kernel_equals_twin_many_videos(dev, kw):
    """30 classes, scores on a coarse grid (ties), exact-threshold IoUs, empty frames, an empty and one-frame videos."""
    frames, videos = seq_nms_twin.make_videos(21, n_videos=14, max_len=30, tracks=6, clutter=12)
    f1, v1 = seq_nms_twin.make_videos(22, lengths=[1, 1, 1], tracks=5, clutter=20)
    videos += [(s + len(frames), n) for s, n in v1]
    frames += f1
    assert any(n == 0 for _, n in videos) and any(n == 1 for _, n in videos)
    assert any(len(f["score"]) == 0 for f in frames)
    _check(frames, videos, dev, **kw)


def test_kernel_equals_twin_frames_over_1024_boxes_of_one_class(dev):
    rng = np.random.default_rng(4)
    frames = []
    for t in range(2):
        n = 1100 + 37 * t
        xy = rng.uniform(0, 1200, (n, 2))
        wh = rng.uniform(5, 60, (n, 2))
        box = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        frames.append({"box": box, "score": (rng.integers(1, 20, n) / 16.0).astype(np.float32),
                       "label": np.full(n, 7, np.int64)})
    _, iters = _check(frames, [(0, 2)], dev)
    assert max(iters.values()) > 1024


def test_kernel_equals_twin_long_video_track(dev):
    """3,200 frames, one track spanning the video (rescored as one path) plus sparse clutter."""
    rng = np.random.default_rng(5)
    L = 3200
    frames = []
    for t in range(L):
        b = [[100 + 0.02 * t + rng.normal(0, 0.5), 80 + rng.normal(0, 0.5), 180 + 0.02 * t, 160]]
        s, lab = [rng.uniform(0.3, 0.9) if t % 50 else 0.01], [3]
        if t % 97 == 5:
            b.append([400, 300, 430, 330])
            s.append(0.6)
            lab.append(3)
        if t % 211 == 7:
            b.append([100 + 0.02 * t, 80, 180 + 0.02 * t, 110])     # IoU ~0.38 with the track: suppressed, not linked
            s.append(0.95)
            lab.append(3)
        frames.append({"box": np.asarray(b, np.float32), "score": np.asarray(s, np.float32),
                       "label": np.asarray(lab, np.int64)})
    r, iters = _check(frames, [(0, L)], dev)
    first = np.cumsum([0] + [len(f["score"]) for f in frames])[:-1]
    assert r["keep"][first].all() and len(np.unique(r["scores"][first])) == 1      # one path over all frames


def test_one_frame_videos_equal_greedy_nms(dev):
    """Independent cross-check: a one-frame video == ops.nms(..., strict_gt=True) per class (distinct scores, IoUs away
    from the threshold)."""
    rng = np.random.default_rng(9)
    frames = []
    pool = rng.permutation(100000)[:40 * 200] / 100000.0 + 1e-4
    for f in range(40):
        n = 200
        xy = np.round(rng.uniform(0, 300, (n, 2)))
        wh = np.round(rng.uniform(10, 80, (n, 2)))
        frames.append({"box": np.concatenate([xy, xy + wh], 1).astype(np.float32),
                       "score": pool[f * n:(f + 1) * n].astype(np.float32), "label": rng.integers(1, 6, n)})
    preds = seq_nms_twin.to_boxlists(frames)
    r = seq_nms.run(preds, [(f, 1) for f in range(len(frames))], device=dev)
    off = np.cumsum([0] + [len(f["score"]) for f in frames])
    checked = 0
    for f, fr in enumerate(frames):
        want = np.zeros(len(fr["score"]), bool)
        for c in np.unique(fr["label"]):
            idx = np.nonzero(fr["label"] == c)[0]
            iou = vid_twin.iou_f32(fr["box"][idx], fr["box"][idx])
            if np.any(np.abs(iou[~np.eye(len(idx), dtype=bool)] - 0.3) < 1e-3):
                continue                                 # keep the cross-check away from the threshold
            k = ops.nms(torch.from_numpy(fr["box"][idx]).to(dev), torch.from_numpy(fr["score"][idx]).to(dev), 0.3,
                        strict_gt=True).cpu().numpy()
            want[idx[k]] = True
            np.testing.assert_array_equal(r["keep"][off[f]:off[f + 1]][idx], want[idx])
            checked += 1
        got_s = r["scores"][off[f]:off[f + 1]]
        np.testing.assert_array_equal(got_s[r["keep"][off[f]:off[f + 1]]],
                                      fr["score"][r["keep"][off[f]:off[f + 1]]])     # one-box paths keep their score
    assert checked > 100


def test_deterministic(dev):
    frames, videos = seq_nms_twin.make_videos(31, n_videos=10, max_len=50, tracks=8, clutter=30)
    preds = seq_nms_twin.to_boxlists(frames)
    a = seq_nms.run(preds, videos, device=dev)
    b = seq_nms.run(preds, videos, device=dev)
    np.testing.assert_array_equal(a["keep"], b["keep"])
    np.testing.assert_array_equal(_bits(a["scores"]), _bits(b["scores"]))


def test_mid_size_set_matches_twin_on_sampled_videos(dev):
    """~24k frames x 300 detections (the bench tool's generator) on the GPU; the twin checks the shortest videos."""
    import bench_seq_nms
    s = bench_seq_nms.make_set(videos=80, frames=24000, dets=300, seed=2,
                               lengths=bench_seq_nms.video_lengths(80, 24000, np.random.default_rng(2), longest=2000))
    preds = bench_seq_nms.to_boxlists(s)
    r = seq_nms.run(preds, s["videos"], device=dev, with_stats=True)
    assert len(r["tasks"]) > 80 * 20 and r["stats"][:, 0].max() > 1000
    D = s["dets"]
    for start, n in sorted(s["videos"], key=lambda v: v[1])[:3]:
        frames = bench_seq_nms.to_frames(s, start, start + n)
        keep, new, _ = seq_nms_twin.seq_nms(frames, [(0, n)])
        wk, ws = np.concatenate(keep), np.concatenate(new)
        np.testing.assert_array_equal(r["keep"][start * D:(start + n) * D], wk)
        np.testing.assert_array_equal(_bits(r["scores"][start * D:(start + n) * D][wk]), _bits(ws[wk]))


def _ap_set(seed=12, n_videos=8, L=30):
    """GT tracks; predictions: the tracks jittered, with score dips, plus temporally isolated false positives whose
    scores lie between the dips and the track scores."""
    rng = np.random.default_rng(seed)
    preds, gts, videos = [], [], []
    for v in range(n_videos):
        videos.append((len(preds), L))
        K = 3
        xy = rng.uniform(0, 300, (K, 2))
        wh = rng.uniform(40, 120, (K, 2))
        cls = rng.integers(1, 31, K)
        for t in range(L):
            gb = np.round(np.concatenate([xy + t, xy + t + wh], 1)).astype(np.float32)
            box = gb + rng.normal(0, 1.0, gb.shape).astype(np.float32)
            sc = np.where(rng.random(K) < 0.3, rng.uniform(0.05, 0.15, K), rng.uniform(0.7, 0.95, K))
            nfp = 2
            fxy = rng.uniform(0, 500, (nfp, 2))
            fb = np.concatenate([fxy, fxy + rng.uniform(20, 60, (nfp, 2))], 1)
            preds.append({"box": np.concatenate([box, fb]).astype(np.float32),
                          "score": np.concatenate([sc, rng.uniform(0.3, 0.5, nfp)]).astype(np.float32),
                          "label": np.concatenate([cls, rng.integers(1, 31, nfp)]), "size": (640, 480)})
            gts.append({"box": gb, "label": cls.astype(np.int64), "im_info": (480, 640)})
    return preds, gts, videos


def test_seq_nms_raises_ap50_on_tracks_with_dips(dev):
    preds, gts, videos = _ap_set()
    bl, gt = vid_twin.to_boxlists(preds, gts)
    raw_map = vid_twin.evaluate(preds, gts)[0]["map"]
    keep, new, _ = seq_nms_twin.seq_nms(preds, videos)
    tw = [{"box": p["box"][k], "score": s[k], "label": p["label"][k], "size": p["size"]} for p, k, s in
          zip(preds, keep, new)]
    twin_map = vid_twin.evaluate(tw, gts)[0]["map"]
    assert twin_map > raw_map + 0.05, (raw_map, twin_map)         # the twin predicts the rise
    out = seq_nms.seq_nms(bl, videos, device=dev)
    res = vid_eval.evaluate_detections(out, gt, device=dev)
    assert abs(res[0]["map"] - twin_map) < 1e-12
    assert res[0]["map"] > vid_eval.evaluate_detections(bl, gt, device=dev)[0]["map"] + 0.05


def test_inference_with_seq_nms_writes_rescored_outputs_and_cli_agrees(dev, tmp_path):
    """image files -> inference(..., seq_nms=True, anno_path=...): predictions.pth stays raw, predictions_seq_nms.pth and
    result_seq_nms.txt equal the twin's Seq-NMS + vid_twin.evaluate; tools/eval_vid.py --seq-nms writes the same."""
    from PIL import Image
    from mega.pytorch_amd import config, inference, modeling, synth
    from test_vid_eval_gpu import _xml
    T, H0, W0 = 12, 90, 160
    clip0 = synth.make_clip(T, H0, W0, seed=8).numpy()
    os.makedirs(str(tmp_path / "Data" / "v"))
    os.makedirs(str(tmp_path / "Anno" / "v"))
    rng = np.random.default_rng(5)
    lines = []
    for t in range(T):
        Image.fromarray(clip0[t]).save(str(tmp_path / "Data" / "v" / ("%06d.JPEG" % t)), format="PNG")
        lines.append("v %d %d %d" % (t + 1, t, T))
        objs = []
        for _ in range(int(rng.integers(0, 5))):
            x1, y1 = int(rng.integers(0, 120)), int(rng.integers(0, 60))
            objs.append((vid_eval.CLASSES_MAP[int(rng.integers(1, 31))],
                         (x1, y1, x1 + int(rng.integers(8, 60)), y1 + int(rng.integers(8, 40)))))
        (tmp_path / "Anno" / "v" / ("%06d.xml" % t)).write_text(_xml(H0, W0, objs))
    (tmp_path / "index.txt").write_text("\n".join(lines) + "\n")
    cfg = config.get_cfg("R-50")
    cfg.MODEL.DEVICE = str(dev)
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 180, 320
    model = modeling.build_detection_model(cfg)
    model.load_state_dict(synth.make_state_dict(blocks=(3, 4, 6), reduce_channel=True, global_res_stage=0, seed=1))
    model.to(dev)
    out = tmp_path / "out"
    rescored = inference.inference(cfg, model, str(tmp_path / "Data"), str(tmp_path / "index.txt"),
                                   output_folder=str(out), steps_per_batch=4, anno_path=str(tmp_path / "Anno"),
                                   seq_nms=True)
    raw = inference.load_predictions(str(out / "predictions.pth"))
    assert len(raw) == T and sum(len(p) for p in raw) > 0
    gt = vid_eval.VIDGroundTruth(str(tmp_path / "index.txt"), str(tmp_path / "Anno"))
    tp, tg = vid_twin.from_boxlists(raw, gt)
    assert (out / "result.txt").read_text() == vid_eval.format_result(
        {i: {"ap": w["ap"], "map": w["map"]} for i, w in enumerate(vid_twin.evaluate(tp, tg))})
    keep, new, _ = seq_nms_twin.seq_nms(tp, [(0, T)])
    saved = inference.load_predictions(str(out / "predictions_seq_nms.pth"))
    assert sum(len(p) for p in saved) < sum(len(p) for p in raw)
    for r, s, p, k, v in zip(rescored, saved, raw, keep, new):
        for x in (r, s):
            np.testing.assert_array_equal(x.bbox.cpu().numpy(), p.bbox.cpu().numpy()[k])
            np.testing.assert_array_equal(_bits(x.get_field("scores").cpu().numpy()), _bits(v[k]))
    tw = [{"box": p["box"][k], "score": v[k], "label": p["label"][k], "size": p["size"]} for p, k, v in zip(tp, keep, new)]
    text = (out / "result_seq_nms.txt").read_text()
    assert text == vid_eval.format_result({i: {"ap": w["ap"], "map": w["map"]} for i, w in enumerate(vid_twin.evaluate(tw, tg))})
    cli_out = tmp_path / "cli"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_vid.py"), "--predictions",
                        str(out / "predictions.pth"), "--img-index", str(tmp_path / "index.txt"), "--anno-path",
                        str(tmp_path / "Anno"), "--output-folder", str(cli_out), "--device", str(dev), "--seq-nms"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ), timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert (cli_out / "result_seq_nms.txt").read_text() == text
    assert (cli_out / "result.txt").read_text() == (out / "result.txt").read_text()
