"""CPU: track refinement (mega/pytorch_amd/tracks.py, refine) -- hand-computed answers through the numpy twin
(tests/track_refine_twin.py), the host checks of tracks.refine, the new C-ABI entry points' declaration and argument checks
(no GPU needed) and the command line's option check."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import track_refine_cases
import track_refine_twin
from mega.pytorch_amd import _lib, tracks
from mega.pytorch_amd.structures import BoxList

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = track_refine_cases.cases()
f32 = np.float32


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def assert_frames_equal(got, want):
    """box and score as f32 bits, label / track / filled exactly, frame by frame in order"""
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        assert _bits(np.asarray(g["box"], f32).reshape(-1, 4)) == _bits(np.asarray(w["box"], f32).reshape(-1, 4)), t
        assert _bits(g["score"]) == _bits(w["score"]), t
        for k in ("label", "track", "filled"):
            assert np.asarray(g[k]).tolist() == np.asarray(w[k]).tolist(), (t, k)


def test_hand_computed_values():
    """A few of the expected numbers, derived again here without the twin or the cases' helpers."""
    w13 = f32(1) / f32(3)
    assert w13 == track_refine_cases.W13 and f32(2) / f32(3) == track_refine_cases.W23
    want = CASES["gap_1_and_gap_3"][3]
    assert want[1]["box"].tolist() == [[0.5, 1.5, 10.5, 11.5]] and want[1]["filled"].tolist() == [1]
    # frame 3 of b = (1, 3, 11, 13) -> c = (2, 5, 13, 20), f - fa = 1 of 3: b + (c - b) * w, one f32 operation at a time
    assert want[3]["box"][0].tolist() == [f32(1) + f32(f32(1) * w13), f32(3) + f32(f32(2) * w13), f32(11) + f32(f32(2) * w13),
                                          f32(13) + f32(f32(7) * w13)]
    assert want[3]["score"].tolist() == [f32(0.5)] and CASES["fill_scale_half"][3][3]["score"].tolist() == [f32(0.25)]
    r1 = CASES["smooth_r1_ends"][3]
    assert r1[0]["box"][0].tolist() == [1.5, 101.5, 201.5, 301.5] and r1[4]["box"][0][0] == f32(14)
    assert r1[1]["box"][0][0] == f32((np.float64(0) + np.float64(3) + np.float64(4)) / np.float64(3))
    assert CASES["smooth_r_larger_than_track"][3][2]["box"][0].tolist() == [7, 107, 207, 307]
    gap = CASES["fill_off_r2_across_a_gap"][3]
    assert [g["box"][0][0] for g in gap if len(g["box"])] == [3.0, 5.0, 7.5, 30.0]
    one = CASES["one_box_track"][3][0]["box"]
    assert np.signbit(one[0][0]) and one[0][0] == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_reproduces_hand_computed_cases(name):
    frames, videos, kw, want, info = CASES[name]
    got, got_info = track_refine_twin.refine(frames, videos, **kw)
    assert_frames_equal(got, want)
    assert got_info == info


@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_is_idempotent(name):
    """Refining a refined list with smooth = 0 adds nothing and changes no bit."""
    frames, videos, kw, _, info = CASES[name]
    once, _ = track_refine_twin.refine(frames, videos, **kw)
    twice, info2 = track_refine_twin.refine(once, videos, fill=kw.get("fill", True))
    assert_frames_equal(twice, once)
    assert info2 == {"tracks": info["tracks"], "filled": 0}


def test_twin_output_order_and_dtypes():
    frames, videos, kw, want, _ = CASES["two_classes_interleaved"]
    got, _ = track_refine_twin.refine(frames, videos, **kw)
    assert got[1]["track"].tolist() == [0, 1] and got[1]["label"].tolist() == [1, 2]       # filled boxes by ascending id
    assert got[0]["track"].tolist() == [1, 0]                                              # input boxes in input order
    for g in got:
        assert g["box"].dtype == np.float32 and g["box"].shape[1] == 4 and g["score"].dtype == np.float32
        assert g["label"].dtype == np.int64 and g["track"].dtype == np.int64 and g["filled"].dtype == np.uint8
    bl = track_refine_twin.to_boxlists(got)
    assert bl[1].get_field("track_ids").dtype == torch.int64 and bl[1].get_field("filled").dtype == torch.uint8
    back = track_refine_twin.from_boxlists(bl)
    assert_frames_equal(back, got)


def _bl(boxes, scores, labels, ids, size=(20, 20), **extra):
    b = BoxList(torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4), size)
    b.add_field("scores", torch.tensor(scores, dtype=torch.float32))
    b.add_field("labels", torch.tensor(labels, dtype=torch.int64))
    if ids is not None:
        b.add_field("track_ids", torch.tensor(ids, dtype=torch.int64))
    for k, v in extra.items():
        b.add_field(k, torch.tensor(v))
    return b


def test_bad_input_raises_before_device_work():
    ok = [_bl([[0, 0, 9, 9]], [0.5], [1], [0])]
    B = [0, 0, 9, 9]
    cases = [
        ([_bl([B], [0.5], [1], None)], [(0, 1)], {}, "track_ids"),
        ([_bl([B], [0.5], [1], [-2])], [(0, 1)], {}, "below -1"),
        ([_bl([B, B], [0.5, 0.5], [1, 1], [3, 3])], [(0, 1)], {}, "same frame"),
        ([_bl([B], [0.5], [1], [0]), _bl([B], [0.5], [2], [0])], [(0, 2)], {}, "more than one label"),
        ([_bl([[0, 0, float("inf"), 9]], [0.5], [1], [0])], [(0, 1)], {}, "not finite"),
        ([_bl([B], [float("nan")], [1], [0])], [(0, 1)], {}, "negative or NaN"),
        ([_bl([B], [-0.5], [1], [0])], [(0, 1)], {}, "negative or NaN"),
        ([_bl([B], [0.5], [-1], [0])], [(0, 1)], {}, "negative class"),
        ([_bl([B], [0.5], [1], [0]), _bl([B], [0.5], [1], [0], size=(30, 20))], [(0, 2)], {}, "size or mode"),
        ([_bl([B], [0.5], [1], [0], objectness=[0.5])], [(0, 1)], {}, "objectness"),
        (ok, [(0, 2)], {}, "cover"),
        (ok, [(1, 1)], {}, "partition"),
        (ok, [(0, 1)], {"smooth": -1}, "smooth"),
        (ok, [(0, 1)], {"smooth": 65}, "smooth"),
        (ok, [(0, 1)], {"smooth": 1.0}, "smooth"),
        (ok, [(0, 1)], {"smooth": True}, "smooth"),
        (ok, [(0, 1)], {"fill": 1}, "fill"),
        (ok, [(0, 1)], {"fill_scale": 0.0}, "fill_scale"),
        (ok, [(0, 1)], {"fill_scale": 1.5}, "fill_scale"),
        (ok, [(0, 1)], {"fill_scale": float("nan")}, "fill_scale"),
        (ok, [(0, 1)], {"fill_scale": 1e-60}, "fill_scale"),            # 0 in f32
        (ok, [(0, 1)], {"fill_scale": "x"}, "fill_scale"),
    ]
    for preds, videos, kw, msg in cases:
        for fn in (tracks.refine, tracks.refine_run):
            with pytest.raises(ValueError, match=msg) as e:
                fn(preds, videos, **kw)              # device="cuda": the checks come first
            assert str(e.value).startswith("tracks:"), str(e.value)
    # the same two tracks in different videos are no duplicate and may differ in label
    two = [_bl([B], [0.5], [1], [0]), _bl([B], [0.5], [2], [0])]
    assert tracks._refine_pack(two, [(0, 1), (1, 1)], True)["K"] == 2
    # a field a filled box has no value for is fine as long as nothing is filled
    assert tracks._refine_pack([_bl([B], [0.5], [1], [0], objectness=[0.5])], [(0, 1)], False)["K"] == 1
    assert tracks.check_refine_params() == (True, 0, 1.0)
    assert tracks.check_refine_params(False, np.int64(64), 0.1) == (False, 64, float(np.float32(0.1)))


def test_slot_counts_are_known_on_the_host():
    """The output size (checked against 2^31 - 1 before any device work) follows from the members' frames alone: with fill a
    track's slots are last - first + 1, without it its member count."""
    first, empty = _bl([[0, 0, 9, 9]], [0.5], [1], [0]), _bl([], [], [], [])
    n = 40
    preds = [first] + [empty] * (n - 2) + [first]
    pk = tracks._refine_pack(preds, [(0, n)], True)
    assert (pk["K"], pk["M"], pk["S"], pk["n_new"]) == (1, 2, n, n - 2)
    assert pk["m_off"].tolist() == [0, 2] and pk["o_off"].tolist() == [0, n]
    pk = tracks._refine_pack(preds, [(0, n)], False)
    assert (pk["S"], pk["n_new"], pk["o_off"].tolist()) == (2, 0, [0, 2])


def test_cpu_device_is_a_runtime_error():
    ok = [_bl([[0, 0, 9, 9]], [0.5], [1], [0])]
    with pytest.raises(RuntimeError, match="no CPU path"):
        tracks.refine(ok, [(0, 1)], device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        tracks.refine_run([], [], device="cpu")


def test_pack_orders_members_by_video_track_and_frame():
    frames, videos, _, _, _ = CASES["empty_video_between"]
    pk = tracks._refine_pack(track_refine_twin.to_boxlists(frames), videos, True)
    assert (pk["K"], pk["M"], pk["S"]) == (2, 4, 8)
    assert pk["frame"].tolist() == [0, 2, 5, 9] and pk["m_off"].tolist() == [0, 2, 4] and pk["o_off"].tolist() == [0, 3, 8]
    frames, videos, _, _, _ = CASES["two_classes_interleaved"]
    pk = tracks._refine_pack(track_refine_twin.to_boxlists(frames), videos, True)
    assert pk["order"].tolist() == [1, 3, 0, 2] and pk["track_id"].tolist() == [0, 1] and pk["track_label"].tolist() == [1, 2]


def test_entry_points_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "mega_hip.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in ("mega_refine_tracks", "mega_refine_tracks_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, decl), name + " is not declared in mega_hip.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["mega_refine_tracks"]
    m = re.search(r"int\s+mega_refine_tracks\s*\((.*?)\);", decl, flags=re.S)
    assert res is _lib.c_int and len(args) == len(m.group(1).split(",")) == 20
    assert _lib.SIGNATURES["mega_refine_tracks_workspace_bytes"] == (_lib.c_size_t, [_lib.c_longlong, _lib.c_int])
    assert "tracks.py" in src[src.index("Refining linked tracks"):src.index("mega_refine_tracks_workspace_bytes(long")]
    from mega.pytorch_amd import build
    assert build.SOURCES["track_refine.hip"] == ["-ffp-contract=off"]


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    #       box score frame m_off o_off K  M  S  fill r  scale  out x 6           ws bytes stream
    args = [8, 8, 8, 8, 8, 1, 2, 3, 1, 1, 1.0, 8, 8, 8, 8, 8, 8, 8, 0, None]
    for i in (0, 1, 2, 3, 4, 11, 12, 13, 14, 15, 16):      # each required pointer NULL with non-zero sizes
        a = list(args)
        a[i] = None
        assert lib.mega_refine_tracks(*a) == 1, i
    for i in (5, 6, 7, 8, 9):                              # K, M, S, fill, r negative
        a = list(args)
        a[i] = -1
        assert lib.mega_refine_tracks(*a) == 1, i
    for i, v in ((9, 65), (8, 2), (10, 0.0), (10, 1.5), (10, -1.0), (10, float("nan")), (6, 1 << 31), (7, 1 << 31),
                 (5, 0), (6, 0)):                          # r, fill, fill_scale, sizes past an i32 index, slots of no track
        a = list(args)
        a[i] = v
        assert lib.mega_refine_tracks(*a) == 1, (i, v)
    # no slot: nothing to launch, not an error, nothing is touched (K = 0; and K tracks whose slot count is 0)
    assert lib.mega_refine_tracks(None, None, None, None, None, 0, 0, 0, 1, 0, 1.0, None, None, None, None, None, None,
                                  None, 0, None) == 0
    assert lib.mega_refine_tracks(None, None, None, 8, 8, 1, 0, 0, 0, 64, 0.5, None, None, None, None, None, None, None, 0,
                                  None) == 0
    # the fused kernel keeps a tile and its halos in LDS: no workspace at any size
    for S, r in ((0, 0), (1, 0), (1 << 20, 64), ((1 << 31) - 1, 64)):
        assert lib.mega_refine_tracks_workspace_bytes(S, r) == 0


@pytest.mark.parametrize("flag", [["--tracks-fill"], ["--tracks-smooth", "2"], ["--tracks-fill-scale", "0.5"]])
def test_eval_vid_rejects_refinement_flags_without_tracks(tmp_path, flag):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_vid.py"), "--predictions", "p.pth",
                        "--img-index", "i.txt", "--anno-path", "a"] + flag,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 2 and flag[0].encode() in r.stdout and b"--tracks" in r.stdout


def test_inference_checks_refinement_parameters_before_the_run():
    from mega.pytorch_amd import config, inference
    cfg = config.get_cfg("R-50")
    for bad, msg in (({"smooth": 65}, "smooth"), ({"fill": "yes"}, "fill"), ({"fill_scale": 2.0}, "fill_scale"),
                     ({"smooth": 1, "link_iou": 2.0}, "link_iou")):
        with pytest.raises(ValueError, match="tracks: .*" + msg):
            inference.inference(cfg, None, "nowhere", "nothing.txt", tracks=bad)
