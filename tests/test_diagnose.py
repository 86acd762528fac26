"""CPU: the detection error diagnosis (mega/pytorch_amd/diagnose.py) -- the cases meet the conditions they are built for,
the Python twin (tests/diagnose_twin.py) reproduces the hand-written expectations and keeps its invariants, faults planted
in the twin are caught by the cases, every host check, the C-ABI entry point's declaration and argument checks (no GPU
needed) and the command line's and inference()'s option checks."""
import ast
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import diagnose_cases
import diagnose_twin
import vid_twin
from mega.pytorch_amd import _lib, diagnose, vid_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = diagnose_cases.hand_cases()


@pytest.fixture(scope="module")
def random_set():
    return diagnose_cases.random_frames(diagnose_twin.frame_iou)


@pytest.fixture(scope="module")
def size_set():
    return diagnose_cases.size_frames(diagnose_twin.frame_iou)


def _iou(det, gt, size=(200, 200)):
    p, g = diagnose_cases.frame([(det, 0.5, 1)], [(gt, 1)], size=size)
    return diagnose_twin.frame_iou(p, g)[0, 0]


def test_exact_cases_equal_the_f32_thresholds():
    f = np.float32
    for det, gt, want in diagnose_cases.exact_ious():
        assert _iou(det, gt) == want and _iou(det, gt).dtype == np.float32
    assert _iou(diagnose_cases.HALF, diagnose_cases.A) == f(0.5) and _iou(diagnose_cases.TENTH, diagnose_cases.A) == f(0.1)
    # written out without the twin: +1 on x2 / y2, then the +1 convention
    a = [f(0), f(0), f(18) + f(1), f(18) + f(1)]
    area_a = (a[2] - a[0] + f(1)) * (a[3] - a[1] + f(1))
    assert area_a == f(400)
    for y2, want in ((f(8), f(0.5)), (f(0), f(0.1))):
        d = [f(0), f(0), f(18) + f(1), y2 + f(1)]
        area_d = (d[2] - d[0] + f(1)) * (d[3] - d[1] + f(1))
        inter = (min(a[2], d[2]) - f(0) + f(1)) * (min(a[3], d[3]) - f(0) + f(1))
        assert inter / ((area_d + area_a) - inter) == want
    # one lattice step below each threshold, outside the margin
    assert f(0.5) - _iou(diagnose_cases.BELOW_HALF, diagnose_cases.A) > 1e-3
    assert f(0.1) - _iou(diagnose_cases.BELOW_TENTH, diagnose_cases.A) > 1e-3
    assert _iou(diagnose_cases.BELOW_TENTH, diagnose_cases.A) > f(0.09)
    # the rescale case reaches the same lattice
    assert _iou([0, 0, 9, 2], diagnose_cases.A, size=(100, 50)) == f(0.5)
    assert _iou([0, 0, 9, 0], diagnose_cases.A, size=(100, 50)) == f(0.1)
    # (half of a 10 x 10 box is not IoU 0.5 here: with vid_iou's +1 on both sides the side terms are 11 and 6)
    assert _iou([0, 0, 9, 4], [0, 0, 9, 9]) == f(66) / f(121)


def test_cases_keep_the_margin_and_the_redraw_cap(random_set, size_set):
    preds, gts, drawn, redrawn = random_set
    assert len(preds) == 250 and drawn == 250 + redrawn
    assert redrawn <= 0.02 * drawn, (redrawn, drawn)
    sets = [(c["preds"], c["gts"]) for c in HAND.values()] + [(preds, gts), size_set]
    exact = 0
    for ps, gs in sets:
        for p, g in zip(ps, gs):
            if len(p["score"]) and len(g["label"]):
                iou = diagnose_twin.frame_iou(p, g)
                assert not diagnose_cases.near_threshold(iou)
                exact += int(((iou == np.float32(0.5)) | (iou == np.float32(0.1))).sum())
    assert exact > 0
    assert all(len(p["score"]) == 12 and len(g["label"]) == 4 for p, g in zip(preds, gts))
    assert all(p["box"].min() >= 0 and p["box"].max() <= 79 and (p["box"] == np.round(p["box"])).all() for p in preds)
    sp, sg = size_set
    assert [len(g["label"]) for g in sg] == [65, 0, 65] and [len(p["score"]) for p in sp] == [130, 130, 0]


@pytest.mark.parametrize("name", sorted(HAND))
def test_twin_reproduces_the_hand_written_expectations(name):
    c = HAND[name]
    r = diagnose_twin.run(c["preds"], c["gts"])
    assert r["det_kind"].tolist() == c["kind"]
    assert r["det_gt"].tolist() == c["gt"]
    assert r["gt_det"].tolist() == [list(row) for row in c["gt_det"]]
    assert r["gt_state"].tolist() == c["state"]
    bkg = np.asarray(c["kind"]) == diagnose_twin.BKG
    assert (r["det_iou"][bkg] == 0).all() and (r["det_iou"][~bkg] > 0).all()


def _invariants(preds, gts, r):
    N, G = len(r["det_kind"]), r["gt_det"].shape[1]
    want = vid_twin.evaluate(preds, gts, None)[0]
    np.testing.assert_array_equal(r["det_kind"] == 0, want["match"] == 1)        # kind 0 <=> the evaluation's match
    assert r["kind_counts"].sum() == N and (r["det_kind"] <= 5).all()           # the kinds partition N
    assert r["kind_counts_by_label"].sum() == N and r["gt_state_counts"].sum() == G
    tp_gt = r["det_gt"][r["det_kind"] == 0]
    assert len(np.unique(tp_gt)) == len(tp_gt)                                   # every DETECTED box has exactly one TP
    np.testing.assert_array_equal(np.sort(tp_gt), np.nonzero(r["gt_state"] == 0)[0])
    for g in np.nonzero(r["gt_state"] == 0)[0]:
        d = r["gt_det"][0, g]
        assert r["det_kind"][d] == 0 and r["det_gt"][d] == g
    assert ((r["det_gt"] < 0) == (r["det_kind"] == 5)).all()
    ap = want["ap"]
    np.testing.assert_allclose(r["ap"][:len(ap)], ap, rtol=0, atol=1e-12, equal_nan=True)


def test_twin_invariants(random_set, size_set):
    for preds, gts in [(c["preds"], c["gts"]) for c in HAND.values() if sum(len(g["label"]) for g in c["gts"])] + \
            [random_set[:2], size_set]:
        _invariants(preds, gts, diagnose_twin.run(preds, gts))
    r = diagnose_twin.run(*random_set[:2])
    assert (r["kind_counts"] > 0).all() and (r["gt_state_counts"] > 0).all()    # the random set shows every kind and state
    assert r["confusion"].sum() == r["kind_counts_thr"][3] and r["confusion"].trace() == 0
    r = diagnose_twin.run(*size_set)
    assert r["gt_det"][0, 64] == 129                         # the box beyond the first 64 lanes is taken by its own detection


@pytest.mark.parametrize("name", sorted(n for n in HAND if HAND[n]["dap_nonneg"]))
def test_no_repair_lowers_the_map_on_the_hand_cases(name):
    """Ignoring false positives, turning one into a true positive on an undetected box, or dropping missed boxes from
    n_pos never lowers a class's AP; on the hand cases no class loses its last positive, so the mAP cannot drop."""
    c = HAND[name]
    r = diagnose_twin.run(c["preds"], c["gts"])
    for k in diagnose_twin.FIXES:
        assert r["dap"][k] >= -1e-12, (k, r["dap"][k])


def test_oracle_rows_on_a_hand_case():
    c = HAND["two_loc_equal_score"]
    r = diagnose_twin.run(c["preds"], c["gts"])
    lab, match, pign, n_pos = r["rows"]["loc"]
    assert match.tolist() == [0, 1, 0] and pign.tolist() == [1, 0, 1]            # the best LOC detection becomes the match
    assert r["map"] == 0 and abs(r["dap"]["loc"] - 1.0) < 1e-12 and r["dap"]["miss"] == 0 and r["dap"]["cls"] == 0
    c = HAND["thresholds_other_label"]
    r = diagnose_twin.run(c["preds"], c["gts"])
    lab, match, pign, n_pos = r["rows"]["cls"]
    assert lab.tolist() == [1, 2, 2, 2] and match.tolist() == [1, 0, 0, 0] and pign.tolist() == [0, 0, 0, 0]
    assert r["rows"]["miss"][3].tolist() == [0, 1, 0] and n_pos.tolist() == [0, 4, 0]
    # only class 1 has GT boxes (label 0 is empty, label 2 only predicted): its AP goes from 0 to 1 / 4
    assert r["map"] == 0 and abs(r["dap"]["cls"] - 0.25) < 1e-12 and np.isnan(r["ap"][0]) and np.isnan(r["ap"][2])


@pytest.mark.parametrize("fault", ["cls_first", "strict", "tie_high"])
def test_planted_faults_are_caught_by_the_hand_cases(fault):
    caught = []
    for name, c in HAND.items():
        r = diagnose_twin.run(c["preds"], c["gts"], fault=fault)
        if (r["det_kind"].tolist() != c["kind"] or r["det_gt"].tolist() != c["gt"] or
                r["gt_det"].tolist() != [list(row) for row in c["gt_det"]]):
            caught.append(name)
    want = {"cls_first": {"dupe_before_cls", "loc_before_cls"}, "strict": {"thresholds_same_label", "thresholds_other_label"},
            "tie_high": {"equal_iou_lower_index", "equal_iou_lower_index_loc"}}[fault]
    assert want <= set(caught), caught


def test_planted_faults_are_caught_by_the_random_frames(random_set):
    preds, gts = random_set[:2]
    good = diagnose_twin.classify(preds, gts)
    for fault in ("cls_first", "strict"):
        bad = diagnose_twin.classify(preds, gts, fault=fault)
        assert any((a != b).any() for a, b in zip(good, bad)), fault


def test_motion_cross_tabulation_counts_a_boundary_in_both_ranges():
    p, g = diagnose_cases.frame([(diagnose_cases.NEAR, 0.9, 1)], [(diagnose_cases.A, 1), (diagnose_cases.FAR, 1)])
    r = diagnose_twin.run([p, p], [g, g], motion=[[0.7, 0.95], []])
    # box 0 (0.7) is fast and medium, box 1 slow; the second frame has no list: in no range
    assert r["motion"]["gt_state_counts"].tolist() == [[0, 1, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]]
    assert r["motion"]["kind_counts"].tolist() == [[0, 1, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0]]
    host = diagnose.tables(r["det_kind"], r["det_gt"], np.asarray([1, 1]), np.float32([0.9, 0.9]), r["gt_det"],
                           np.asarray([1, 1, 1, 1]), 2, 0.5, np.asarray([0.7, 0.95, np.nan, np.nan]))
    for k in ("gt_state_counts", "kind_counts"):
        assert host["motion"][k].tolist() == r["motion"][k].tolist()


def test_host_tables_and_text_equal_the_twins(random_set):
    preds, gts = random_set[:2]
    motion = diagnose_cases.motion_table(gts)
    r = diagnose_twin.run(preds, gts, motion=motion, score_thresh=0.625)
    labels = np.concatenate([p["label"] for p in preds])
    score = np.concatenate([p["score"] for p in preds])
    gl = np.concatenate([g["label"] for g in gts])
    mot = np.concatenate([np.asarray(m if len(m) else [np.nan] * len(g["label"]), np.float64)
                          for m, g in zip(motion, gts)])
    assert any(len(m) == 0 for m in motion) and (mot == 0.7).any()
    host = diagnose.tables(r["det_kind"], r["det_gt"], labels, score, r["gt_det"], gl, 4, 0.625, mot)
    for k, v in host.items():
        if k == "motion":
            for kk in v:
                np.testing.assert_array_equal(v[kk], r["motion"][kk])
        else:
            np.testing.assert_array_equal(v, r[k])
    assert (score == np.float32(0.625)).any() and r["kind_counts_thr"].sum() == (score >= np.float32(0.625)).sum()
    np.testing.assert_array_equal(diagnose.gt_states(r["gt_det"]), r["gt_state"])
    res = dict(r, **host)
    assert diagnose.format_result(res) == r["text"]
    lines = r["text"].splitlines()
    assert lines[0].startswith("mAP = ") and [l.split()[1] for l in lines[1:7]] == list(diagnose.FIXES)
    assert len(lines) == 1 + 6 + 3 + 6 and lines[8].startswith("kinds | score>=0.62")
    assert diagnose.KINDS == diagnose_twin.KINDS and diagnose.GT_STATES == diagnose_twin.GT_STATES


def test_summarize_forms_the_differences():
    nan = float("nan")
    ap6 = np.asarray([[nan, 0.5, 0.0], [nan, 0.75, 0.0], [nan, 0.5, 0.5], [nan, 0.5, 0.0], [nan, 1.0, 0.0], [nan, 0.5, nan]])
    m, dap, by = diagnose.summarize(ap6, np.asarray([nan, 0.5, 1.0]))
    assert m == 0.25 and dap == {"dupe": 0.125, "loc": 0.25, "cls": 0.5, "both": 0.0, "bkg": 0.25, "miss": 0.25}
    assert by["bkg"][1] == 0.5 and np.isnan(by["miss"][2]) and np.isnan(by["dupe"][0])


def test_check_params():
    assert diagnose.check_params() == (0.5, 0.1) and diagnose.check_params(0, 0.25) == (0.0, 0.25)
    for bad in (0.0, 0.5, -0.1, 0.7, float("nan"), 1e-50, "0.1", None, True):
        with pytest.raises(ValueError, match="^diagnose: bg_thresh"):
            diagnose.check_params(bg_thresh=bad)
    for bad in (float("nan"), "x", None, False):
        with pytest.raises(ValueError, match="^diagnose: score_thresh"):
            diagnose.check_params(score_thresh=bad)
    assert diagnose.check_params(bg_thresh=0.49999997) == (0.5, 0.49999997)
    with pytest.raises(ValueError, match="^diagnose: bg_thresh"):
        diagnose.check_params(bg_thresh=0.49999999)          # 0.5 as an f32


def test_bad_input_raises_before_device_work():
    c = HAND["detected_with_loc_and_cls"]
    bl, gt = vid_twin.to_boxlists(c["preds"], c["gts"])
    for fn in (diagnose.run, diagnose.evaluate_errors):
        with pytest.raises(ValueError, match="^diagnose: no predictions"):
            fn([], gt)
        with pytest.raises(ValueError, match="^diagnose: Length of gt and pred lists"):
            fn(bl + bl, gt)
        with pytest.raises(ValueError, match="^diagnose: bg_thresh"):
            fn(bl, gt, bg_thresh=0.5)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(bl, gt, device="cpu")
    for field, value, msg in (("box", np.inf, "a prediction box is not finite"), ("score", np.nan, "score is NaN"),
                              ("label", -1, "negative class label")):
        p = {k: np.array(v) if isinstance(v, np.ndarray) else v for k, v in c["preds"][0].items()}
        p[field].reshape(-1)[0] = value
        bad, _ = vid_twin.to_boxlists([p], c["gts"])
        with pytest.raises(ValueError, match="^diagnose: .*" + msg):
            diagnose.evaluate_errors(bad, gt)
    with pytest.raises(ValueError, match="^diagnose: the motion IoU list covers 0 frames"):
        diagnose.evaluate_errors(bl, gt, motion_iou=[])
    with pytest.raises(ValueError, match="^diagnose: score_thresh"):
        diagnose.evaluate_errors(bl, gt, score_thresh=float("nan"))


def test_entry_point_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "mega_hip.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    name = "mega_diagnose_match"
    assert len(re.findall(r"\b%s\s*\(" % name, decl)) == 1, "declared once in mega_hip.h"
    assert hasattr(lib, name) and name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    m = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, decl, flags=re.S)
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert res is _lib.c_int and len(args) == len(params) == 20
    for a, p in zip(args, params):
        want = _lib.c_void_p if "*" in p else {"int": _lib.c_int, "long long": _lib.c_longlong,
                                               "float": _lib.c_float}[p.rsplit(" ", 1)[0]]
        assert a is want, p
    assert _lib.PARAMS[name] == ("det_box", "det_label", "det_score", "det_off", "order", "ratio", "gt_box", "gt_label",
                                 "gt_off", "F", "C", "N", "G", "max_gt", "bg_thresh", "det_kind", "det_gt", "det_iou",
                                 "gt_det", "stream")
    assert "diagnose.py" in src[src.index("Detection error diagnosis"):src.index("int mega_diagnose_match(")]
    from mega.pytorch_amd import build
    assert build.SOURCES["diagnose.hip"] == ["-ffp-contract=off"]
    assert "mega_diagnose_match_workspace_bytes" not in src


def _call(lib, ins=None, F=1, C=2, N=1, G=1, max_gt=1, bg=0.1, outs=(8, 8, 8, 8)):
    return lib.mega_diagnose_match(*(list(ins or [8] * 9) + [F, C, N, G, max_gt, bg] + list(outs) + [None]))


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()
    for i in range(9):                                           # each input pointer NULL with non-zero sizes
        p = [8] * 9
        p[i] = None
        assert _call(lib, ins=p) == 1, i
    for i in range(4):                                           # each output pointer NULL
        o = [8] * 4
        o[i] = None
        assert _call(lib, outs=o) == 1, i
    for name in ("F", "N", "G", "max_gt"):
        assert _call(lib, **{name: -1}) == 1, name
    assert _call(lib, C=0) == 1 and _call(lib, C=-3) == 1
    assert _call(lib, max_gt=4097) == 1 and _call(lib, max_gt=vid_eval.MAX_GT_PER_FRAME + 1) == 1
    for bg in (0.0, 0.5, -0.1, 0.75, float("nan"), float("inf")):
        assert _call(lib, bg=bg) == 1, bg
    assert _call(lib, N=1 << 31) == 1
    assert _call(lib, F=0) == 1                                  # boxes without a frame
    # no frame, no boxes: nothing to do, nothing is touched
    assert _call(lib, ins=[None] * 9, F=0, N=0, G=0, max_gt=0, outs=(None,) * 4) == 0
    src = open(os.path.join(ROOT, "mega", "pytorch_amd", "csrc", "diagnose.hip")).read()
    assert int(re.search(r"DG_MAX_CHUNKS\s*=\s*(\d+)", src).group(1)) * 64 == vid_eval.MAX_GT_PER_FRAME


def test_the_wrapper_takes_no_workspace():
    path = os.path.join(ROOT, "mega", "pytorch_amd", "ops.py")
    src = open(path).read()
    fn = [n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef) and n.name == "diagnose_match"]
    assert len(fn) == 1
    seg = ast.get_source_segment(src, fn[0])
    assert "_ws(" not in seg and '"mega_diagnose_match"' in seg and 'prof=("diagnose_match",)' in seg


def test_eval_vid_lists_the_flags_and_checks_them(tmp_path):
    tool = os.path.join(ROOT, "tools", "eval_vid.py")
    r = subprocess.run([sys.executable, tool, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0
    for flag in (b"--diagnose", b"--diagnose-score-thresh", b"--diagnose-bg-thresh"):
        assert flag in r.stdout, flag
    base = [sys.executable, tool, "--predictions", "p.pth", "--img-index", "i.txt", "--anno-path", "a"]
    for extra, msg in ((["--diagnose", "--box-only"], b"--diagnose applies to detections"),
                       (["--diagnose-bg-thresh", "0.2"], b"apply to --diagnose"),
                       (["--diagnose", "--diagnose-bg-thresh", "0.5"], b"bg_thresh must be inside")):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=str(tmp_path), timeout=120)
        assert r.returncode == 2 and msg in r.stdout, r.stdout


def test_inference_checks_diagnose_before_the_run():
    from mega.pytorch_amd import config, inference
    cfg = config.get_cfg("R-50")
    with pytest.raises(ValueError, match="bg_thresh"):
        inference.inference(cfg, None, "nowhere", "nothing.txt", diagnose={"bg_thresh": 0.6})
    cfg.MODEL.RPN_ONLY = True
    with pytest.raises(ValueError, match="RPN_ONLY returns proposals: the error diagnosis"):
        inference.inference(cfg, None, "nowhere", "nothing.txt", diagnose=True)
