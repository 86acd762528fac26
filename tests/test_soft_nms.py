"""CPU: TEST.SOFT_NMS / TEST.BBOX_VOTE -- the numpy twin of soft_nms.py (tests/soft_nms_twin.py) against the pinned
bbox_aug twin and on hand-computed cases, the preconditions of the seeded GPU fixtures, the config keys, and the routing
of compute_on_dataset / VIDDemo with a stub detector and a stub merge (no device)."""
import types

import numpy as np
import pytest
import torch

import bbox_aug_twin as bt
import soft_nms_twin as tw
from mega.pytorch_amd import bbox_aug, config, demo, inference, ops, soft_nms
from mega.pytorch_amd.structures import BoxList

f32 = np.float32


def _bits(a):
    return np.asarray(a, f32).view(np.uint32)


def _same_bits(a, b):
    for x, y in zip(a[:2], b[:2]):
        np.testing.assert_array_equal(_bits(x), _bits(y))
    np.testing.assert_array_equal(a[2], b[2])


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("strict", [True, False])
def test_twin_with_both_options_off_is_the_pinned_merge(strict):
    sizes = [(160, 96), (160, 96), (203, 117), (203, 117)]
    flips = [False, True, False, True]
    for seed in (3, 4):
        v, _ = bt.random_views(seed, 4, 120, C1=5, sizes=sizes, grid=25)
        for max_det in (300, 40, 0):
            _same_bits(tw.merge(v, sizes, flips, max_det=max_det, strict_gt=strict),
                       bt.merge(v, sizes, flips, max_det=max_det, strict_gt=strict))
    frames, sizes, flips = tw.fixture(3, 300)
    _same_bits(tw.merge(frames[0], sizes, flips, strict_gt=strict), bt.merge(frames[0], sizes, flips, strict_gt=strict))


def _one_class(boxes, scores):
    return [(np.asarray(boxes, f32)[None], np.asarray(scores, f32)[None])], [(1000, 600)], [False]


def test_gaussian_with_a_huge_sigma_keeps_every_live_row_unchanged():
    frames, sizes, flips = tw.fixture(1, 300)
    b, s, l = tw.merge(frames[0], sizes, flips, max_det=0, soft_method="gaussian", sigma=1e30)
    mb, ms = tw.map_views(frames[0], sizes, flips)
    live = ms > f32(0.001)
    assert len(s) == int(live.sum()) > 200
    np.testing.assert_array_equal(_bits(s), _bits(ms[live]))
    np.testing.assert_array_equal(_bits(b), _bits(mb[live]))


def test_linear_on_disjoint_boxes_is_the_input():
    boxes = [[10 + 40 * i, 20, 30 + 40 * i, 50] for i in range(8)]
    scores = [0.3, 0.9, -1, 0.5, 0.0005, 0.7, 0.2, 0.4]
    b, s, l = tw.merge(*_one_class(boxes, scores), soft_method="linear")
    want = [0, 1, 3, 5, 6, 7]
    np.testing.assert_array_equal(s, np.asarray(scores, f32)[want])
    np.testing.assert_array_equal(b, np.asarray(boxes, f32)[want])
    assert l.tolist() == [1] * 6


def test_two_identical_boxes_under_linear_keep_one():
    st = {}
    kept, ks = tw.soft_nms(np.asarray([[5, 5, 20, 30]] * 2, f32), np.asarray([0.8, 0.8], f32), "linear", stats=st)
    assert kept.tolist() == [0] and ks.tolist() == [f32(0.8)]          # equal scores: the lower row wins; 0.8 * (1 - 1) = 0
    b, s, l = tw.merge(*_one_class([[5, 5, 20, 30]] * 2, [0.6, 0.8]), soft_method="linear")
    assert s.tolist() == [f32(0.8)] and b.tolist() == [[5, 5, 20, 30]]


def test_linear_threshold_comparison_follows_strict_gt():
    boxes, scores = [[0, 0, 9, 9], [0, 0, 9, 19]], [0.75, 0.5]        # IoU = 100 / 200 = 0.5 exactly
    assert tw.iou(np.asarray(boxes[0], f32), np.asarray(boxes[1:], f32))[0] == f32(0.5)
    _, s, _ = tw.merge(*_one_class(boxes, scores), soft_method="linear", strict_gt=True)
    assert s.tolist() == [0.75, 0.5]
    _, s, _ = tw.merge(*_one_class(boxes, scores), soft_method="linear", strict_gt=False)
    assert s.tolist() == [0.75, 0.25]


def test_gaussian_decay_and_the_score_threshold():
    boxes, scores = [[0, 0, 9, 9], [0, 0, 9, 19], [100, 100, 120, 120]], [0.75, 0.5, 0.0011]
    _, s, _ = tw.merge(*_one_class(boxes, scores), soft_method="gaussian", sigma=0.5)
    w = np.exp(f32(-0.25) / f32(0.5))
    assert s.tolist() == [f32(0.75), f32(0.5) * f32(w), f32(0.0011)]   # (the far box: IoU 0, expf(0) = 1)
    _, s, _ = tw.merge(*_one_class(boxes, [0.75, 0.0016, 0.5]), soft_method="gaussian", sigma=0.5)
    assert s.tolist() == [f32(0.75), f32(0.5)]                          # 0.0016 * 0.607 < 0.001: it leaves unkept


def test_vote_threshold_one_on_distinct_boxes_changes_nothing():
    frames, sizes, flips = tw.fixture(3, 37)
    a = tw.merge(frames[0], sizes, flips, vote_on=True, vote_thresh=1.0)
    _same_bits(a, bt.merge(frames[0], sizes, flips))


CLUSTER = [[10, 10, 29, 29], [11, 10, 30, 29], [10, 11, 29, 30], [200, 200, 240, 230]]


def test_three_box_cluster_votes_to_hand_computed_coordinates():
    # IoU(A, B) = IoU(A, C) = 380 / 420 = 0.905: A is kept, B and C are suppressed and vote; the far box votes alone
    b, s, l = tw.merge(*_one_class(CLUSTER, [0.6, 0.3, 0.1, 0.9]), vote_on=True, vote_thresh=0.8)
    assert s.tolist() == [f32(0.6), f32(0.9)]                          # "ID"
    np.testing.assert_allclose(b[0], [10.3, 10.1, 29.3, 29.1], rtol=0, atol=2e-6)
    np.testing.assert_array_equal(b[1], [200, 200, 240, 230])
    # below the vote threshold nothing joins: IoU(B, C) = 361 / 439 = 0.82 but neither is kept
    b, _, _ = tw.merge(*_one_class(CLUSTER, [0.6, 0.3, 0.1, 0.9]), vote_on=True, vote_thresh=0.95)
    np.testing.assert_array_equal(b[0], CLUSTER[0])


def test_avg_scoring_is_the_mean_of_the_voters_original_scores():
    _, s, _ = tw.merge(*_one_class(CLUSTER, [0.6, 0.3, 0.1, 0.9]), vote_on=True, vote_thresh=0.8, vote_scoring="AVG")
    want = f32((np.float64(f32(0.6)) + np.float64(f32(0.3)) + np.float64(f32(0.1))) / 3)
    assert s.tolist() == [want, f32(0.9)] and abs(float(want) - 1 / 3) < 1e-7
    # after linear soft-NMS B survives decayed (0.3 * (1 - 0.905)); its voters still carry their original scores
    b, s, _ = tw.merge(*_one_class(CLUSTER, [0.6, 0.3, 0.1, 0.9]), soft_method="linear", vote_on=True, vote_thresh=0.8,
                       vote_scoring="AVG")
    assert len(s) == 4 and s[0] == want and s[1] == want and s[2] == want
    np.testing.assert_allclose(b[1], [10.3, 10.1, 29.3, 29.1], rtol=0, atol=2e-6)
    _, s, _ = tw.merge(*_one_class(CLUSTER, [0.6, 0.3, 0.1, 0.9]), soft_method="linear", vote_on=True, vote_thresh=0.8)
    o = tw.iou(np.asarray(CLUSTER[0], f32), np.asarray(CLUSTER[1:2], f32))[0]
    assert s[1] == f32(0.3) * (f32(1) - o)


def test_nan_iou_neither_decays_nor_votes():
    boxes = [[0, 0, 9, 9], [np.nan, 0, 9, 9]]
    for method in ("linear", "gaussian"):
        b, s, _ = tw.merge(*_one_class(boxes, [0.75, 0.5]), soft_method=method, vote_on=True, vote_thresh=0.5)
        assert s.tolist() == [0.75, 0.5]
        np.testing.assert_array_equal(b[0], boxes[0])


@pytest.mark.parametrize("K,R", sorted(tw.FIXTURE_SEEDS))
def test_gpu_fixture_preconditions(K, R):
    """for every seeded gaussian fixture of tests/test_soft_nms_gpu.py: no selection and no threshold crossing lies within
    1e-3 (relative) of flipping, so the GPU's expf may differ from numpy's by the tolerance of that test"""
    frames, sizes, flips = tw.fixture(K, R)
    st = {}
    for fr in frames:
        assert all(s.shape == (3, R) for _, s in fr) and len(fr) == K
        tw.merge(fr, sizes, flips, max_det=0, soft_method="gaussian", sigma=tw.FIXTURE_SIGMA, stats=st)
        _, ms = tw.map_views(fr, sizes, flips)
        assert (ms > f32(0.001)).sum(1).max() <= 111
    print("K=%d R=%d: gap %.3e thresh %.3e steps %d" % (K, R, st.get("gap", np.inf), st.get("thresh", np.inf), st["steps"]))
    assert st.get("gap", np.inf) >= 1e-3 and st.get("thresh", np.inf) >= 1e-3
    if R > 1:       # dead rows are interleaved with live ones, and IoUs fall on both sides of 0.5 and 0.8
        mb, ms = tw.map_views(frames[0], sizes, flips)
        live = np.nonzero(ms[0] > 0)[0]
        assert (ms[0][:live.max()] < 0).any()
        o = np.concatenate([tw.iou(mb[0][i], mb[0][live]) for i in live])
        for lo, hi in ((0.0, 0.5), (0.5, 0.8), (0.8, 0.999)):
            assert ((o > lo) & (o < hi)).any(), (lo, hi)


# ------------------------------------------------------------------------------------------------ config
def test_config_has_the_keys_with_their_defaults():
    for m in ("mega", "rdn", "fgfa", "dff", "base"):
        cfg = config.get_cfg("R-50", m)
        assert dict(cfg.TEST.SOFT_NMS) == {"ENABLED": False, "METHOD": "linear", "SIGMA": 0.5}
        assert dict(cfg.TEST.BBOX_VOTE) == {"ENABLED": False, "VOTE_TH": 0.8, "SCORING_METHOD": "ID"}
        ff = config.final_filter(cfg)
        assert not ff.enabled and soft_nms.enabled_filter(cfg) is None
    cfg.merge_from_list(["TEST.SOFT_NMS.ENABLED", True, "TEST.SOFT_NMS.METHOD", "gaussian", "TEST.SOFT_NMS.SIGMA", 0.25,
                         "TEST.BBOX_VOTE.ENABLED", True, "TEST.BBOX_VOTE.VOTE_TH", 0.9, "TEST.BBOX_VOTE.SCORING_METHOD", "AVG"])
    assert config.final_filter(cfg.clone()).kwargs() == {"soft_method": "gaussian", "sigma": 0.25, "vote": True,
                                                         "vote_thresh": 0.9, "vote_scoring": "AVG"}
    cfg.TEST.SOFT_NMS.ENABLED = False
    ff = config.final_filter(cfg)
    assert ff.enabled and ff.soft_method is None and ff.vote


def test_a_reference_cfg_without_the_keys_reads_as_disabled():
    ref_like = types.SimpleNamespace(TEST=types.SimpleNamespace(BBOX_AUG=types.SimpleNamespace(ENABLED=False)))
    assert not config.final_filter(ref_like).enabled
    assert not config.final_filter(types.SimpleNamespace()).enabled


@pytest.mark.parametrize("key,value", [("TEST.SOFT_NMS.METHOD", "quadratic"), ("TEST.SOFT_NMS.SIGMA", 0.0),
                                       ("TEST.SOFT_NMS.SIGMA", -1.0), ("TEST.BBOX_VOTE.VOTE_TH", 0.0),
                                       ("TEST.BBOX_VOTE.VOTE_TH", 1.5), ("TEST.BBOX_VOTE.SCORING_METHOD", "MAX")])
def test_bad_values_raise_before_any_device_work(key, value, tmp_path):
    cfg = config.get_cfg("R-50", "base")
    cfg.merge_from_list([key, value])
    with pytest.raises(ValueError, match=key.rsplit(".", 1)[0]):
        config.final_filter(cfg)
    model = _StubModel(cfg)
    with pytest.raises(ValueError, match=key.rsplit(".", 1)[0]):      # inference(): before the index file is even opened
        inference.inference(cfg, model, str(tmp_path), str(tmp_path / "missing.txt"), device="cpu")
    with pytest.raises(ValueError, match=key.rsplit(".", 1)[0]):
        demo.VIDDemo(cfg, model=model, runner=lambda src, v: [])


def test_rpn_only_refuses_the_options(tmp_path):
    cfg = config.get_cfg("R-50", "base")
    cfg.MODEL.RPN_ONLY = True
    cfg.TEST.BBOX_VOTE.ENABLED = True
    with pytest.raises(ValueError, match="BBOX_VOTE"):
        inference.inference(cfg, _StubModel(cfg), str(tmp_path), str(tmp_path / "missing.txt"), device="cpu")


# ------------------------------------------------------------------------------------------------ routing
L, NC, R = 3, 4, 5


class _StubModel(object):
    def __init__(self, cfg):
        self.cfg = cfg
        rh = cfg.MODEL.ROI_HEADS
        pp = types.SimpleNamespace(candidates=False, score_thresh=rh.SCORE_THRESH, nms=rh.NMS,
                                   detections_per_img=rh.DETECTIONS_PER_IMG, strict_gt=bool(cfg.NMS_STRICT_GT))
        self.roi_heads = types.SimpleNamespace(box=types.SimpleNamespace(post_processor=pp))

    def eval(self):
        return self


def _cfg(**kv):
    cfg = config.get_cfg("R-50", "base")
    cfg.MODEL.DEVICE = "cpu"
    cfg.MODEL.ROI_BOX_HEAD.NUM_CLASSES = NC
    cfg.MODEL.ROI_HEADS.NMS = 0.45
    cfg.MODEL.ROI_HEADS.DETECTIONS_PER_IMG = 77
    cfg.NMS_STRICT_GT = False
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 60, 100
    lst = []
    for k, v in kv.items():
        lst += [k, v]
    cfg.merge_from_list(lst)
    return cfg


def _routing(cfg, monkeypatch):
    """compute_on_dataset over one 3-frame video with a stub engine (it records the candidate flag and the feed it was
    given) and stub merges -> (calls, results)"""
    model = _StubModel(cfg)
    pp = model.roi_heads.box.post_processor
    calls = {"runs": [], "soft": [], "hard": []}

    def runner(src, v):
        calls["runs"].append((pp.candidates, src.out_hw, src.hflip))
        n = (NC - 1) * R if pp.candidates else 2
        out = []
        for t in range(v["seg_len"]):
            b = BoxList(torch.arange(n * 4, dtype=torch.float32).reshape(n, 4) + t, (src.out_hw[1], src.out_hw[0]))
            b.add_field("scores", torch.full((n,), 0.5))
            b.add_field("labels", torch.ones(n, dtype=torch.int64))
            out.append(b)
        return out

    def fake(name):
        def merge(cb, cs, sizes, flips, score_thresh, nms_thresh, max_det, strict_gt=True, **kw):
            calls[name].append(dict(kw, shape=tuple(cs.shape), sizes=list(sizes), flips=list(flips),
                                    score_thresh=score_thresh, nms_thresh=nms_thresh, max_det=max_det, strict_gt=strict_gt))
            F = cs.shape[1]
            return (torch.zeros((F, 1, 4)), torch.full((F, 1), 0.25), torch.full((F, 1), 2, dtype=torch.int64),
                    torch.ones(F, dtype=torch.int32))
        return merge
    monkeypatch.setattr(ops, "soft_merge", fake("soft"))
    monkeypatch.setattr(ops, "bbox_aug_merge", fake("hard"))
    index = types.SimpleNamespace(videos=[{"start": 0, "pattern": "v/%06d", "seg_len": L}])
    res = inference.compute_on_dataset(model, index, "unused", torch.device("cpu"), runner=runner,
                                       source_kwargs={"opener": lambda f: np.zeros((48, 80, 3), np.uint8), "workers": 1})
    assert not pp.candidates                      # candidate mode only inside the run
    return calls, res


def test_routing_both_off_leaves_the_plain_path_alone(monkeypatch):
    calls, res = _routing(_cfg(), monkeypatch)
    assert calls["runs"] == [(False, (60, 100), False)] and not calls["soft"] and not calls["hard"]
    assert sorted(res) == [0, 1, 2] and all(len(r) == 2 for r in res.values())


@pytest.mark.parametrize("kv,want", [
    ({"TEST.SOFT_NMS.ENABLED": True},
     {"soft_method": "linear", "sigma": 0.5, "vote": False, "vote_thresh": 0.8, "vote_scoring": "ID"}),
    ({"TEST.SOFT_NMS.ENABLED": True, "TEST.SOFT_NMS.METHOD": "gaussian", "TEST.SOFT_NMS.SIGMA": 0.3},
     {"soft_method": "gaussian", "sigma": 0.3, "vote": False, "vote_thresh": 0.8, "vote_scoring": "ID"}),
    ({"TEST.BBOX_VOTE.ENABLED": True, "TEST.BBOX_VOTE.VOTE_TH": 0.7, "TEST.BBOX_VOTE.SCORING_METHOD": "AVG"},
     {"soft_method": None, "sigma": 0.5, "vote": True, "vote_thresh": 0.7, "vote_scoring": "AVG"})])
def test_routing_an_option_enters_candidate_mode_and_calls_the_soft_merge(monkeypatch, kv, want):
    calls, res = _routing(_cfg(**kv), monkeypatch)
    assert calls["runs"] == [(True, (60, 100), False)]               # the identity view alone, one pass
    assert not calls["hard"] and len(calls["soft"]) == 1
    c = calls["soft"][0]
    assert {k: c[k] for k in want} == want
    assert c["shape"] == (1, L, NC - 1, R) and c["sizes"] == [(100, 60)] and c["flips"] == [False]
    assert (c["score_thresh"], c["nms_thresh"], c["max_det"], c["strict_gt"]) == (0.001, 0.45, 77, False)
    assert sorted(res) == [0, 1, 2]
    for r in res.values():
        assert len(r) == 1 and r.size == (100, 60) and r.get_field("labels").tolist() == [2]
        assert r.get_field("scores").tolist() == [0.25]


def test_routing_with_bbox_aug_its_views_feed_the_soft_merge(monkeypatch):
    base = {"TEST.BBOX_AUG.ENABLED": True, "TEST.BBOX_AUG.H_FLIP": True}
    calls, _ = _routing(_cfg(**base), monkeypatch)
    assert len(calls["hard"]) == 1 and not calls["soft"]             # box augmentation alone: the plain merge, as before
    calls, _ = _routing(_cfg(**dict(base, **{"TEST.SOFT_NMS.ENABLED": True, "TEST.BBOX_VOTE.ENABLED": True})), monkeypatch)
    assert calls["runs"] == [(True, (60, 100), False), (True, (60, 100), True)]
    assert not calls["hard"] and len(calls["soft"]) == 1
    c = calls["soft"][0]
    assert c["shape"] == (2, L, NC - 1, R) and c["flips"] == [False, True] and c["soft_method"] == "linear" and c["vote"]


def test_viddemo_routes_the_folder_through_the_soft_merge(tmp_path, monkeypatch):
    from PIL import Image
    import overlay_twin
    folder = tmp_path / "frames"
    folder.mkdir()
    for t in range(L):
        Image.fromarray(np.zeros((48, 80, 3), np.uint8)).save(str(folder / ("%06d.JPEG" % t)), format="JPEG")
    seen = {"soft": 0, "cand": []}
    for kv in ({}, {"TEST.BBOX_VOTE.ENABLED": True}):
        cfg = _cfg(**kv)
        model = _StubModel(cfg)
        pp = model.roi_heads.box.post_processor

        def runner(src, v):
            seen["cand"].append(pp.candidates)
            n = (NC - 1) * R if pp.candidates else 2
            out = []
            for t in range(v["seg_len"]):
                b = BoxList(torch.zeros((n, 4)), (100, 60))
                b.add_field("scores", torch.full((n,), 0.5))
                b.add_field("labels", torch.ones(n, dtype=torch.int64))
                out.append(b)
            return out

        def soft(cb, cs, sizes, flips, *a, **kw):
            seen["soft"] += 1
            assert kw["vote"] and kw["soft_method"] is None
            F = cs.shape[1]
            return (torch.zeros((F, 1, 4)), torch.full((F, 1), 0.25), torch.full((F, 1), 2, dtype=torch.int64),
                    torch.ones(F, dtype=torch.int32))
        monkeypatch.setattr(ops, "soft_merge", soft)
        d = demo.VIDDemo(cfg, model=model, runner=runner, overlay=overlay_twin.as_op(demo.CATEGORIES),
                         source_kwargs={"workers": 1})
        d.run_on_image_folder(str(folder))
        assert [len(p) for p in d.predictions] == ([1] * L if kv else [2] * L)
    assert seen == {"soft": 1, "cand": [False, True]}
