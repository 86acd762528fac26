"""GPU: the track-refinement kernel (csrc/track_refine.hip through mega.pytorch_amd.tracks.refine / refine_run) against the
hand-computed cases and the numpy twin (tests/track_refine_twin.py) -- boxes and scores as f32 bits, labels, ids, "filled"
and the per-frame order exactly -- at the kernel's wave, tile and halo boundaries, under stale memory, and at the end of
inference()."""
import os

import numpy as np
import pytest
import torch

import poison
import seq_nms_twin
import track_eval_twin
import track_refine_cases
import track_refine_twin
from test_track_refine import assert_frames_equal
from mega.pytorch_amd import ops, track_eval, tracks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
CASES = track_refine_cases.cases()


def _check(frames, videos, dev, **kw):
    """tracks.refine (list[BoxList]) and tracks.refine_run (flat) == the twin, bit for bit; -> (refined frames, info)."""
    want, info = track_refine_twin.refine(frames, videos, **kw)
    preds = track_refine_twin.to_boxlists(frames)
    out, got_info = tracks.refine(preds, videos, device=dev, **kw)
    assert got_info == info and len(out) == len(preds)
    for p, o in zip(preds, out):
        assert o.size == p.size and o.mode == p.mode
        assert sorted(o.fields()) == sorted(set(p.fields()) | {"filled"})
        assert o.bbox.dtype == torch.float32 and o.get_field("filled").dtype == torch.uint8
        assert o.get_field("track_ids").dtype == torch.int64 and o.get_field("scores").dtype == torch.float32
    assert_frames_equal(track_refine_twin.from_boxlists(out), want)
    r = tracks.refine_run(preds, videos, device=dev, **kw)
    n_in = [len(f["score"]) for f in frames]
    cat = np.concatenate
    assert r["tracks"] == info["tracks"] and r["boxes"].shape == (sum(n_in), 4)
    assert r["boxes"].view(np.uint32).tolist() == cat([w["box"][:n] for w, n in zip(want, n_in)]).view(np.uint32).tolist()
    assert r["fill_box"].view(np.uint32).tolist() == cat([w["box"][n:] for w, n in zip(want, n_in)]).view(np.uint32).tolist()
    assert r["fill_score"].view(np.uint32).tolist() == cat([w["score"][n:] for w, n in zip(want, n_in)]).view(np.uint32).tolist()
    assert r["fill_frame"].tolist() == [t for t, (w, n) in enumerate(zip(want, n_in)) for _ in range(len(w["score"]) - n)]
    assert r["fill_id"].tolist() == cat([w["track"][n:] for w, n in zip(want, n_in)]).tolist()
    assert r["fill_label"].tolist() == cat([w["label"][n:] for w, n in zip(want, n_in)]).tolist()
    return want, info


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_computed_cases(dev, name):
    frames, videos, kw, want, info = CASES[name]
    out, got_info = tracks.refine(track_refine_twin.to_boxlists(frames), videos, device=dev, **kw)
    assert_frames_equal(track_refine_twin.from_boxlists(out), want)
    assert got_info == info
    _check(frames, videos, dev, **kw)
    # refining the refined list with smooth = 0 adds nothing and changes no bit
    again, info2 = tracks.refine(out, videos, fill=kw.get("fill", True), device=dev)
    assert_frames_equal(track_refine_twin.from_boxlists(again), track_refine_twin.from_boxlists(out))
    assert info2 == {"tracks": info["tracks"], "filled": 0}


def _single_track(slots, fill, seed):
    """One track (id 5, label 2) of `slots` output slots: with fill its first and last frames are slots - 1 apart and about
    half the frames between hold a box; without fill it has `slots` boxes, 1 .. 3 frames apart."""
    rng = np.random.default_rng(seed)
    if fill:
        has = rng.random(slots) < 0.5
        has[0] = has[-1] = True
    else:
        has = np.zeros(3 * slots, bool)
        has[np.cumsum(rng.integers(1, 4, slots)) - 1] = True
        has = has[:int(np.nonzero(has)[0][-1]) + 1]
    frames = []
    for t, h in enumerate(has):
        xy = rng.uniform(0, 300, 2) + 0.37 * t
        b = [[xy[0], xy[1], xy[0] + rng.uniform(20, 90), xy[1] + rng.uniform(20, 90)]] if h else []
        frames.append(track_refine_cases._frame(b, [rng.uniform(0.1, 1.0)] if h else [], [2] if h else [], [5] if h else []))
    return frames


@pytest.mark.parametrize("slots", [1, 2, 63, 64, 65, 255, 256, 257, 600])
def test_single_track_at_wave_and_tile_boundaries(dev, slots):
    """One wave, one tile, one slot more; 600 slots are three tiles, so a halo of 64 crosses two tile boundaries; r = 64 is
    larger than the short tracks."""
    for fill in (True, False):
        frames = _single_track(slots, fill, seed=slots)
        for r in (0, 1, 2, 64):
            want, info = _check(frames, [(0, len(frames))], dev, fill=fill, smooth=r, fill_scale=0.75)
            assert sum(len(w["score"]) for w in want) == slots and info["tracks"] == 1


def _packed_tracks(lengths, stride, seed):
    """len(lengths) tracks in one video, all starting in frame 0, track k with a box in every stride-th frame of its
    lengths[k] frames and in its last one; track k's coordinates lie around 1000 k, so a box averaged or interpolated with a
    neighbouring track's shows."""
    rng = np.random.default_rng(seed)
    T = max(lengths)
    frames = []
    for t in range(T):
        b, s, lab, ids = [], [], [], []
        for k in reversed(range(len(lengths))):               # (higher ids first within a frame: the order is the input's)
            if t < lengths[k] and (t % stride == 0 or t == lengths[k] - 1):
                x, y = 1000.0 * k + 0.5 * t + rng.normal(0, 1), 1000.0 * k + rng.normal(0, 1)
                b.append([x, y, x + 40, y + 30])
                s.append(rng.uniform(0.1, 1.0))
                lab.append(k + 1)
                ids.append(k)
        frames.append(track_refine_cases._frame(b, s, lab, ids))
    return frames


@pytest.mark.parametrize("lengths", [(100, 30, 5, 200), (250, 10, 300), (256, 256), (300, 1, 1, 70)])
def test_neighbouring_tracks_share_tiles_and_halos(dev, lengths):
    """A track ends and the next begins inside one tile (offsets 100, 130, 135), across a tile boundary (250 .. 260), exactly
    on one (256), and inside one halo: the windows take only their own track's slots."""
    for stride, fill in ((3, True), (1, True), (2, False)):
        frames = _packed_tracks(lengths, stride, seed=sum(lengths))
        for r in (1, 64):
            want, info = _check(frames, [(0, len(frames))], dev, fill=fill, smooth=r)
            assert info["tracks"] == len(lengths)
            for w in want:                                    # nothing leaked: every box still lies around its own 1000 k
                k = np.asarray(w["track"], np.float32)
                assert (np.abs(w["box"][:, 0] - 1000 * k) < 300).all() and (np.abs(w["box"][:, 1] - 1000 * k) < 50).all()


def test_many_one_box_tracks_per_tile(dev):
    """300 one-box tracks in one frame and 300 two-box tracks with a gap in the frames around it: more tracks than a tile has
    slots, every window cut to a single slot or to three."""
    rng = np.random.default_rng(9)
    n = 300
    xy = rng.uniform(0, 2000, (n, 2))
    box = np.concatenate([xy, xy + rng.uniform(10, 50, (n, 2))], 1)
    sc, lab = rng.uniform(0.1, 1, n), rng.integers(1, 5, n)
    fr = track_refine_cases._frame
    frames = [fr(box + 3, sc, lab, np.arange(n) + n), fr(box[::-1], sc[::-1], lab[::-1], np.arange(n)[::-1]),
              fr(box + 8, sc, lab, np.arange(n) + n)]
    for r in (0, 2):
        want, info = _check(frames, [(0, 3)], dev, smooth=r)
        assert info == {"tracks": 2 * n, "filled": n}
        assert want[1]["track"][n:].tolist() == list(range(n, 2 * n))         # the filled boxes by ascending id
        assert (want[1]["box"][:n] == frames[1]["box"]).all()                 # one-box tracks: unchanged


_RANDOM = []


def _random_case(dev):
    """3 videos of 40, 1 and 25 frames, at most 20 boxes a frame, 4 classes, linked by tracks.link(max_gap=2)."""
    if not _RANDOM:
        frames, videos = seq_nms_twin.make_videos(31, lengths=[40, 1, 25], classes=4, tracks=5, clutter=8)
        assert max(len(f["score"]) for f in frames) <= 20 and [n for _, n in videos] == [40, 1, 25]
        linked, table = tracks.link(seq_nms_twin.to_boxlists(frames), videos, max_gap=2, score_thresh=0.1, device=dev)
        assert (table["last"] - table["first"] + 1 > table["count"]).sum() >= 3          # tracks with gaps to fill
        _RANDOM.append((track_refine_twin.from_boxlists(linked), videos))
    return _RANDOM[0]


@pytest.mark.parametrize("kw", [{}, {"smooth": 2}, {"fill": False, "smooth": 3}, {"smooth": 64, "fill_scale": 0.5}])
def test_kernel_equals_twin_on_linked_random_videos(dev, kw):
    frames, videos = _random_case(dev)
    want, info = _check(frames, videos, dev, **kw)
    assert info["tracks"] > 10 and (info["filled"] > 0) == kw.get("fill", True)


def test_nothing_to_refine(dev):
    assert tracks.refine([], [], device=dev) == ([], {"tracks": 0, "filled": 0})
    empty = [track_refine_cases.EMPTY] * 3
    want, info = _check(empty, [(0, 2), (2, 1)], dev, smooth=2)
    assert info == {"tracks": 0, "filled": 0} and all(len(w["score"]) == 0 for w in want)
    # the entry point itself with K = 0 and S = 0: no launch, empty outputs
    z = torch.zeros(1, dtype=torch.int64, device=dev)
    out = ops.refine_tracks(torch.zeros((0, 4), device=dev), torch.zeros(0, device=dev),
                            torch.zeros(0, dtype=torch.int32, device=dev), z, z, 0, True, 1, 1.0)
    assert [tuple(o.shape) for o in out] == [(0, 4), (0,), (0,), (0,), (0,), (0,)]


def _flat(r):
    return {k: r[k] for k in ("boxes", "fill_box", "fill_score", "fill_frame", "fill_label", "fill_id", "tracks")}


@pytest.mark.parametrize("mode", poison.MODES)
def test_result_does_not_depend_on_stale_output_bytes(dev, mode):
    """The random case under poisoned allocations: every output element is written by the kernel, so 0x00, 0xFF or the bytes
    of a larger problem in its output arrays change no bit."""
    frames, videos = _random_case(dev)
    preds = track_refine_twin.to_boxlists(frames)
    kw = {"smooth": 2, "fill_scale": 0.5}
    clean = _flat(tracks.refine_run(preds, videos, device=dev, **kw))
    mods = (ops, tracks)
    if mode != "replay":
        with poison.poisoned(mode, mods) as p:
            got = _flat(tracks.refine_run(preds, videos, device=dev, **kw))
        assert p.count >= 6
    else:
        big = track_refine_twin.to_boxlists(_packed_tracks((250, 10, 300), 3, seed=1))
        with poison.poisoned("zeros", mods) as p:
            tracks.refine_run(big, [(0, len(big))], device=dev, smooth=64)
        with poison.poisoned("replay", mods, slab_bytes=2 * p.nbytes + (1 << 20), device=dev) as p:
            tracks.refine_run(big, [(0, len(big))], device=dev, smooth=64)
            p.reset()
            got = _flat(tracks.refine_run(preds, videos, device=dev, **kw))
    for k, v in clean.items():
        if isinstance(v, np.ndarray):
            assert got[k].dtype == v.dtype and got[k].tobytes() == v.tobytes(), k
        else:
            assert got[k] == v, k


def test_filling_lifts_the_tubelet_ap_at_three_quarters(dev):
    """A 9-frame GT track moving 2 px a frame, detected in the even frames only (score 0.9) and linked with max_gap = 1: the
    tubelet has 5 of the 9 frames, tIoU 5/9 < 3/4: AP 0 at the last threshold.  Filled, it has all 9, and the midpoints of an
    integer lattice are exact, so every frame IoU is 1: AP 1."""
    gts = [track_eval_twin._gt([[2 * t, 4, 2 * t + 20, 30]], [1], [0], (48, 64)) for t in range(9)]
    preds = [track_eval_twin._pred([[2 * t, 4, 2 * t + 20, 30]] if t % 2 == 0 else [], [0.9] * (1 - t % 2), [1] * (1 - t % 2),
                                   [-1] * (1 - t % 2), (64, 48)) for t in range(9)]
    _, gt = track_eval_twin.to_inputs(preds, gts)
    linked, table = tracks.link(seq_nms_twin.to_boxlists(preds), [(0, 9)], max_gap=1, device=dev)
    assert len(table) == 1 and int(table["count"][0]) == 5
    assert track_eval.THRESHOLDS[2] == (3, 4)
    before = track_eval.evaluate_tracks(linked, gt, [(0, 9)], device=dev)
    np.testing.assert_allclose(before["ap"][:, 1], [1.0, 1.0, 0.0], rtol=0, atol=1e-12)
    refined, info = tracks.refine(linked, [(0, 9)], fill=True, device=dev)
    assert info == {"tracks": 1, "filled": 4}
    for t, p in enumerate(refined):
        assert p.bbox.tolist() == [[2 * t, 4, 2 * t + 20, 30]] and p.get_field("filled").tolist() == [t % 2]
    after = track_eval.evaluate_tracks(refined, gt, [(0, 9)], device=dev)
    np.testing.assert_allclose(after["ap"][:, 1], [1.0, 1.0, 1.0], rtol=0, atol=1e-12)
    assert [int(x) for x in after["gt_table"][0]][3:] == [9, 0, 9, 9]


def test_inference_with_refinement_writes_the_refined_list(dev, tmp_path):
    """inference(..., tracks={"fill": True, "smooth": 1, "tubelet_ap": True}): predictions_tracks.pth is tracks.refine of the
    linked detections (field "filled"), result_tracks.txt and result_tubelets.txt are written, tracks.txt stays the linker's
    and predictions.pth the raw list.  With the new keys absent or off the run writes what tracks={} writes, byte for byte."""
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
    (tmp_path / "index.txt").write_text("\n".join(lines) + "\n")
    cfg = config.get_cfg("R-50")
    cfg.MODEL.DEVICE = str(dev)
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 180, 320
    model = modeling.build_detection_model(cfg)
    model.load_state_dict(synth.make_state_dict(blocks=(3, 4, 6), reduce_channel=True, global_res_stage=0, seed=1))
    model.to(dev)
    link_kw = {"score_thresh": 0.0, "link_iou": 0.3, "max_gap": 2}

    def run(name, **extra):
        out = tmp_path / name
        inference.inference(cfg, model, str(tmp_path / "Data"), str(tmp_path / "index.txt"), output_folder=str(out),
                            steps_per_batch=4, anno_path=str(tmp_path / "Anno"), tracks=dict(link_kw, **extra))
        return out
    a = run("refined", fill=True, smooth=1, tubelet_ap=True)
    b = run("plain")
    c = run("off", fill=False, smooth=0, fill_scale=0.5)
    raw = inference.load_predictions(str(a / "predictions.pth"))
    assert all("track_ids" not in p.fields() and "filled" not in p.fields() for p in raw)
    assert (a / "predictions.pth").read_bytes() == (b / "predictions.pth").read_bytes()
    assert (b / "predictions_tracks.pth").read_bytes() == (c / "predictions_tracks.pth").read_bytes()
    assert (a / "tracks.txt").read_text() == (b / "tracks.txt").read_text() != ""
    assert not (b / "result_tracks.txt").exists() and not (c / "result_tracks.txt").exists()
    plain = inference.load_predictions(str(b / "predictions_tracks.pth"))
    assert all("filled" not in p.fields() and "track_ids" in p.fields() for p in plain)
    want, info = tracks.refine(plain, [(0, T)], fill=True, smooth=1, device=dev)
    print("tracks: %d, filled boxes: %d" % (info["tracks"], info["filled"]))
    saved = inference.load_predictions(str(a / "predictions_tracks.pth"))
    assert all(p.get_field("filled").dtype == torch.uint8 for p in saved)
    assert_frames_equal(track_refine_twin.from_boxlists(saved), track_refine_twin.from_boxlists(want))
    twin, _ = track_refine_twin.refine(track_refine_twin.from_boxlists(plain), [(0, T)], fill=True, smooth=1)
    assert_frames_equal(track_refine_twin.from_boxlists(saved), twin)
    gt = vid_eval.VIDTrackGroundTruth(str(tmp_path / "index.txt"), str(tmp_path / "Anno"))
    assert (a / "result_tracks.txt").read_text() == vid_eval.format_result(vid_eval.evaluate_detections(saved, gt, device=dev))
    assert (a / "result_tubelets.txt").read_text() == track_eval.evaluate_tracks(saved, gt, [(0, T)], device=dev)["text"]
    # tools/eval_vid.py --tracks --tracks-fill --tracks-smooth 1 on the raw predictions writes the same files
    import importlib.util
    spec = importlib.util.spec_from_file_location("eval_vid_tool", os.path.join(ROOT, "tools", "eval_vid.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    cli = tmp_path / "cli"
    assert tool.main(["--predictions", str(a / "predictions.pth"), "--img-index", str(tmp_path / "index.txt"), "--anno-path",
                      str(tmp_path / "Anno"), "--output-folder", str(cli), "--device", str(dev), "--tracks",
                      "--tracks-score-thresh", "0", "--tracks-link-iou", "0.3", "--tracks-max-gap", "2", "--tracks-fill",
                      "--tracks-smooth", "1", "--tubelet-ap"]) == 0
    assert_frames_equal(track_refine_twin.from_boxlists(inference.load_predictions(str(cli / "predictions_tracks.pth"))), twin)
    for name in ("result_tracks.txt", "result_tubelets.txt", "tracks.txt", "result.txt"):
        assert (cli / name).read_text() == (a / name).read_text(), name
