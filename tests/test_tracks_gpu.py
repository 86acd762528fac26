"""GPU: the track-linking kernel (csrc/tracks.hip through mega.pytorch_amd.tracks) against the hand-computed cases and the
numpy twin (tests/tracks_twin.py) -- ids exactly, scores as f32 bits, the table row for row -- and track linking at the
end of inference() / tools/eval_vid.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seq_nms_twin
import tracks_cases
import tracks_twin
import vid_twin
from mega.pytorch_amd import tracks, vid_eval

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytestmark = pytest.mark.gpu


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _rows(table):
    return [(int(r["video"]), int(r["id"]), int(r["label"]), int(r["first"]), int(r["last"]), int(r["count"]),
             float(r["mean"])) for r in table]


def _cat(parts, dtype):
    return np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)


def _check(frames, videos, dev, **kw):
    """tracks.run (flat) and tracks.link (list[BoxList]) == the twin: the id and the f32 score bits of every box, the
    table row for row (the mean as the same f64)."""
    ids, new, table = tracks_twin.link(frames, videos, **kw)
    preds = tracks_twin.to_boxlists(frames)
    r = tracks.run(preds, videos, device=dev, **kw)
    np.testing.assert_array_equal(r["track_ids"], _cat(ids, np.int64))
    np.testing.assert_array_equal(_bits(r["scores"]), _bits(_cat(new, np.float32)))
    assert _rows(r["table"]) == table
    out, tab = tracks.link(preds, videos, device=dev, **kw)
    assert len(out) == len(preds) and _rows(tab) == table
    for p, o, i, s in zip(preds, out, ids, new):
        assert o.size == p.size and o.mode == p.mode and len(o) == len(p)
        assert sorted(o.fields()) == sorted(p.fields() + ["track_ids"])
        assert o.get_field("track_ids").dtype == torch.int64
        np.testing.assert_array_equal(o.bbox.numpy(), p.bbox.numpy())
        np.testing.assert_array_equal(o.get_field("labels").numpy(), p.get_field("labels").numpy())
        np.testing.assert_array_equal(o.get_field("track_ids").numpy(), i)
        np.testing.assert_array_equal(_bits(o.get_field("scores").numpy()), _bits(s))
    return r, (ids, new, table)


@pytest.mark.parametrize("name", sorted(tracks_cases.cases()))
def test_hand_computed_cases(dev, name):
    frames, videos, kw, ids, scores, table = tracks_cases.cases()[name]
    out, tab = tracks.link(tracks_twin.to_boxlists(frames), videos, device=dev, **kw)
    assert [o.get_field("track_ids").tolist() for o in out] == ids
    for o, e in zip(out, scores):
        np.testing.assert_array_equal(_bits(o.get_field("scores").numpy()), _bits(e))
    if table is not None:
        assert _rows(tab) == table
    r = tracks.run(tracks_twin.to_boxlists(frames), videos, device=dev, **kw)
    assert r["track_ids"].tolist() == [i for f in ids for i in f]
    np.testing.assert_array_equal(_bits(r["scores"]), _bits(_cat([np.asarray(e, np.float32) for e in scores], np.float32)))
    _check(frames, videos, dev, **kw)


def test_minus_zero_score_keeps_its_bits(dev):
    """-0.0 counts as +0.0 in the candidate order; an unlinked box's score field stays bit for bit."""
    f = tracks_cases._frame
    frames = [f([tracks_cases.BOX], [0.9], [1]), f([[0, 0, 9, 7], tracks_cases.BOX], [0.0, -0.0], [1, 1])]
    out, _ = tracks.link(tracks_twin.to_boxlists(frames), [(0, 2)], score_thresh=0.0, min_len=2, rescore="max", device=dev)
    assert [o.get_field("track_ids").tolist() for o in out] == [[0], [0, -1]]
    np.testing.assert_array_equal(_bits(out[1].get_field("scores").numpy()), _bits(np.asarray([0.9, -0.0], np.float32)))


_MANY = []


def _many_videos():
    """30 classes, scores on a coarse grid (ties), exact-threshold IoUs, empty frames, an empty and one-frame videos."""
    if not _MANY:
        frames, videos = seq_nms_twin.make_videos(21, n_videos=14, max_len=30, tracks=6, clutter=12)
        f1, v1 = seq_nms_twin.make_videos(22, lengths=[1, 1, 1], tracks=5, clutter=20)
        videos = videos + [(s + len(frames), n) for s, n in v1]
        frames = frames + f1
        assert any(n == 0 for _, n in videos) and any(n == 1 for _, n in videos)
        assert any(len(f["score"]) == 0 for f in frames)
        _MANY.append((frames, videos))
    return _MANY[0]


@pytest.mark.parametrize("kw", [{}, {"score_thresh": 0.0}, {"link_iou": 0.0, "rescore": "avg"},
                                {"link_iou": 1.0, "rescore": "max"}, {"max_gap": 0, "min_len": 3, "rescore": "avg"},
                                {"max_gap": 3, "min_len": 3, "rescore": "max", "score_thresh": 0.125},
                                {"max_gap": 1, "link_iou": 0.3, "min_len": 2, "rescore": "avg"}])
def test_kernel_equals_twin_many_videos(dev, kw):
    frames, videos = _many_videos()
    r, _ = _check(frames, videos, dev, **kw)
    if kw.get("link_iou") != 1.0:
        assert r["table"]["count"].max() > 1          # something links


def test_kernel_equals_twin_more_boxes_and_open_tracks_than_threads(dev):
    """Two frames of ~1,100 boxes of one class: more candidates per frame, and after frame 0 more open tracks, than a
    workgroup has threads and than the table's part in LDS holds."""
    rng = np.random.default_rng(4)
    n = 1100
    xy = rng.uniform(0, 1200, (n, 2))
    wh = rng.uniform(5, 60, (n, 2))
    box0 = np.concatenate([xy, xy + wh], 1)
    xy1 = rng.uniform(0, 1200, (37, 2))
    box1 = np.concatenate([box0 + rng.normal(0, 1.0, box0.shape), np.concatenate([xy1, xy1 + rng.uniform(5, 60, (37, 2))], 1)])
    frames = [{"box": b.astype(np.float32), "score": (rng.integers(1, 20, len(b)) / 16.0).astype(np.float32),
               "label": np.full(len(b), 7, np.int64)} for b in (box0, box1[rng.permutation(len(box1))])]
    r, (ids, _, table) = _check(frames, [(0, 2)], dev, link_iou=0.3)
    assert sum(1 for row in table if row[5] == 2) > 900 and len(table) > 1100


def test_long_video_track_is_one_id(dev):
    """3,200 frames, one track spanning the video plus sparse clutter: the spanning track is a single id of 3,200 boxes."""
    rng = np.random.default_rng(5)
    L = 3200
    frames = []
    for t in range(L):
        b = [[100 + 0.02 * t + rng.normal(0, 0.5), 80 + rng.normal(0, 0.5), 180 + 0.02 * t, 160]]
        s, lab = [rng.uniform(0.3, 0.9) if t % 50 else 0.06], [3]
        if t % 97 == 5:
            b.append([400, 300, 430, 330])
            s.append(0.6)
            lab.append(3)
        if t % 211 == 7:
            b.append([100 + 0.02 * t, 80, 180 + 0.02 * t, 110])     # IoU ~0.38 with the track: a track of its own
            s.append(0.95)
            lab.append(3)
        frames.append({"box": np.asarray(b, np.float32), "score": np.asarray(s, np.float32),
                       "label": np.asarray(lab, np.int64)})
    r, _ = _check(frames, [(0, L)], dev, rescore="avg")
    first = np.cumsum([0] + [len(f["score"]) for f in frames])[:-1]
    assert (r["track_ids"][first] == 0).all() and len(np.unique(r["scores"][first])) == 1
    assert _rows(r["table"])[0][:6] == (0, 0, 3, 0, L - 1, L)


def test_tracks_that_close_and_reopen_exercise_compaction(dev):
    """Objects that appear for 1 .. 5 frames, vanish for as long and come back, out of phase with each other and with
    long-lived tracks between them in the table: a reappearance after more than max_gap frames is a new id, and closing
    some entries must not disturb the others."""
    rng = np.random.default_rng(8)
    L, K = 60, 40
    base = np.stack([np.arange(K) % 8 * 70.0, np.arange(K) // 8 * 70.0], 1)
    frames = []
    for t in range(L):
        b, s = [], []
        for k in range(K):
            period = 1 + k % 5
            if k % 4 == 0 or (t // period) % 2 == 0:             # every fourth object never vanishes
                xy = base[k] + rng.normal(0, 0.7, 2)
                b.append([xy[0], xy[1], xy[0] + 50, xy[1] + 50])
                s.append(rng.integers(2, 16) / 16.0)
        frames.append({"box": np.asarray(b, np.float32).reshape(-1, 4), "score": np.asarray(s, np.float32),
                       "label": np.full(len(s), 2, np.int64)})
    for gap in (0, 1, 2):
        r, (_, _, table) = _check(frames, [(0, L)], dev, max_gap=gap, rescore="avg")
        assert sum(1 for row in table if row[5] == L) == K // 4
    assert len(table) < len(_check(frames, [(0, L)], dev, max_gap=0)[1][2])       # a longer gap bridges more


def _maps(dev, preds, gts, videos, **kw):
    """(the twin's map, its table) after the device result has been shown equal to the twin's."""
    bl, gt = vid_twin.to_boxlists(preds, gts)
    _, new, table = tracks_twin.link(preds, videos, **kw)
    twin_map = vid_twin.evaluate(tracks_twin.rescored(preds, new), gts)[0]["map"]
    return bl, gt, twin_map, table


def test_rescoring_by_tracks_raises_ap50_on_tracks_with_dips(dev):
    preds, gts, videos = tracks_twin.ap_set()
    raw_map = vid_twin.evaluate(preds, gts)[0]["map"]
    bl, gt, twin_map, table = _maps(dev, preds, gts, videos, rescore="avg")
    assert twin_map > raw_map + 0.05, (raw_map, twin_map)         # the twin predicts the rise
    assert sum(1 for row in table if row[5] >= 20) == 24          # every GT track is recovered
    out, tab = tracks.link(bl, videos, rescore="avg", device=dev)
    assert _rows(tab) == table
    res = vid_eval.evaluate_detections(out, gt, device=dev)
    assert abs(res[0]["map"] - twin_map) < 1e-12
    assert res[0]["map"] > vid_eval.evaluate_detections(bl, gt, device=dev)[0]["map"] + 0.05


def test_max_gap_bridges_missing_detections(dev):
    preds, gts, videos = tracks_twin.ap_gap_set()
    raw_map = vid_twin.evaluate(preds, gts)[0]["map"]
    bl, gt, map0, table0 = _maps(dev, preds, gts, videos, max_gap=0, min_len=5, rescore="avg")
    _, _, map1, table1 = _maps(dev, preds, gts, videos, max_gap=1, min_len=5, rescore="avg")
    assert len(table1) == len(videos) * 3 and len(table0) > len(table1)
    assert map1 > map0 > raw_map, (raw_map, map0, map1)
    for gap, twin_map, table in ((0, map0, table0), (1, map1, table1)):
        out, tab = tracks.link(bl, videos, max_gap=gap, min_len=5, rescore="avg", device=dev)
        assert _rows(tab) == table
        assert abs(vid_eval.evaluate_detections(out, gt, device=dev)[0]["map"] - twin_map) < 1e-12


def test_deterministic(dev):
    frames, videos = _many_videos()
    preds = tracks_twin.to_boxlists(frames)
    a = tracks.run(preds, videos, rescore="avg", device=dev)
    b = tracks.run(preds, videos, rescore="avg", device=dev)
    np.testing.assert_array_equal(a["track_ids"], b["track_ids"])
    np.testing.assert_array_equal(_bits(a["scores"]), _bits(b["scores"]))


def test_inference_with_tracks_writes_outputs_and_cli_agrees(dev, tmp_path):
    """image files -> inference(..., tracks={...}, anno_path=...): predictions.pth and result.txt stay raw;
    predictions_tracks.pth, tracks.txt and result_tracks.txt equal the twin's linking + vid_twin.evaluate;
    tools/eval_vid.py --tracks writes the same."""
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
    kw = {"score_thresh": 0.0, "link_iou": 0.3, "max_gap": 2, "min_len": 1, "rescore": "avg"}
    ret = inference.inference(cfg, model, str(tmp_path / "Data"), str(tmp_path / "index.txt"), output_folder=str(out),
                              steps_per_batch=4, anno_path=str(tmp_path / "Anno"), tracks=kw)
    raw = inference.load_predictions(str(out / "predictions.pth"))
    assert len(raw) == T and sum(len(p) for p in raw) > 0
    for a, c in zip(raw, ret):                        # predictions.pth and the return value: the raw detections
        assert a.fields() == c.fields() and "track_ids" not in a.fields()
        np.testing.assert_array_equal(a.bbox.numpy(), c.bbox.cpu().numpy())
        np.testing.assert_array_equal(_bits(a.get_field("scores").numpy()), _bits(c.get_field("scores").cpu().numpy()))
    gt = vid_eval.VIDGroundTruth(str(tmp_path / "index.txt"), str(tmp_path / "Anno"))
    tp, tg = vid_twin.from_boxlists(raw, gt)
    assert (out / "result.txt").read_text() == vid_eval.format_result(
        {i: {"ap": w["ap"], "map": w["map"]} for i, w in enumerate(vid_twin.evaluate(tp, tg))})
    ids, new, table = tracks_twin.link(tp, [(0, T)], **kw)
    print("tracks: %d, of more than one box: %d" % (len(table), sum(1 for r in table if r[5] > 1)))
    assert len(table) > 0
    saved = inference.load_predictions(str(out / "predictions_tracks.pth"))
    for s, p, i, v in zip(saved, raw, ids, new):
        assert sorted(s.fields()) == sorted(p.fields() + ["track_ids"])
        np.testing.assert_array_equal(s.bbox.numpy(), p.bbox.numpy())
        np.testing.assert_array_equal(s.get_field("track_ids").numpy(), i)
        np.testing.assert_array_equal(_bits(s.get_field("scores").numpy()), _bits(v))
    want_tracks = "".join("{:d} {:d} {} {:d} {:d} {:d} {:.6f}\n".format(r[0], r[1], vid_eval.CLASSES[r[2]], *r[3:])
                          for r in table)
    assert (out / "tracks.txt").read_text() == want_tracks
    text = (out / "result_tracks.txt").read_text()
    assert text == vid_eval.format_result({i: {"ap": w["ap"], "map": w["map"]} for i, w in
                                           enumerate(vid_twin.evaluate(tracks_twin.rescored(tp, new), tg))})
    # the saved file unpickles as the reference's BoxList with the extra field
    shadow = type("BoxList", (object,), {"__module__": inference._REF_MODULE})
    with inference._reference_boxlist_module(shadow):
        obj = torch.load(str(out / "predictions_tracks.pth"), map_location="cpu", weights_only=False)
    assert type(obj[0]).__module__ == inference._REF_MODULE and "track_ids" in obj[0].extra_fields
    cli_out = tmp_path / "cli"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_vid.py"), "--predictions",
                        str(out / "predictions.pth"), "--img-index", str(tmp_path / "index.txt"), "--anno-path",
                        str(tmp_path / "Anno"), "--output-folder", str(cli_out), "--device", str(dev), "--tracks",
                        "--tracks-score-thresh", "0", "--tracks-link-iou", "0.3", "--tracks-max-gap", "2",
                        "--tracks-rescore", "avg"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ), timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert (cli_out / "result_tracks.txt").read_text() == text
    assert (cli_out / "tracks.txt").read_text() == want_tracks
    assert (cli_out / "result.txt").read_text() == (out / "result.txt").read_text()
    for s, c in zip(saved, inference.load_predictions(str(cli_out / "predictions_tracks.pth"))):
        np.testing.assert_array_equal(s.get_field("track_ids").numpy(), c.get_field("track_ids").numpy())
        np.testing.assert_array_equal(_bits(s.get_field("scores").numpy()), _bits(c.get_field("scores").numpy()))
