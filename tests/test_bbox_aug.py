"""CPU: TEST.BBOX_AUG in the config, the reference's view order and sizes (views_from_cfg), and the numpy twin of the
merge (tests/bbox_aug_twin.py) on hand-computed cases."""
import numpy as np
import pytest

import bbox_aug_twin as tw
from mega.pytorch_amd import bbox_aug, config, feed

f32 = np.float32


def test_config_has_the_reference_bbox_aug_defaults_and_round_trips():
    cfg = config.get_cfg("R-50", "base")
    a = cfg.TEST.BBOX_AUG
    assert (a.ENABLED, a.H_FLIP, tuple(a.SCALES), a.MAX_SIZE, a.SCALE_H_FLIP) == (False, False, (), 4000, False)
    cfg.merge_from_list(["TEST.BBOX_AUG.ENABLED", True, "TEST.BBOX_AUG.H_FLIP", True, "TEST.BBOX_AUG.SCALES", (400, 500),
                         "TEST.BBOX_AUG.MAX_SIZE", 1200, "TEST.BBOX_AUG.SCALE_H_FLIP", True])
    c2 = cfg.clone()
    assert (c2.TEST.BBOX_AUG.ENABLED, c2.TEST.BBOX_AUG.H_FLIP, c2.TEST.BBOX_AUG.SCALES, c2.TEST.BBOX_AUG.MAX_SIZE,
            c2.TEST.BBOX_AUG.SCALE_H_FLIP) == (True, True, (400, 500), 1200, True)
    with pytest.raises(KeyError):
        cfg.merge_from_list(["TEST.BBOX_AUG.VOTE", True])
    for m in ("mega", "rdn", "fgfa", "dff", "base"):
        assert config.get_cfg("R-101", m).TEST.BBOX_AUG.ENABLED is False


def test_views_follow_the_reference_order_and_sizes():
    cfg = config.get_cfg("R-50", "base")
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 600, 1000
    cfg.TEST.BBOX_AUG.ENABLED = True
    in_wh = (1280, 720)
    assert bbox_aug.views_from_cfg(cfg, in_wh) == [bbox_aug.View(600, 1000, False, (999, 562))]   # long side capped
    cfg.TEST.BBOX_AUG.H_FLIP = True
    cfg.TEST.BBOX_AUG.SCALES = (400, 800)
    cfg.TEST.BBOX_AUG.MAX_SIZE = 1200
    cfg.TEST.BBOX_AUG.SCALE_H_FLIP = True
    v = bbox_aug.views_from_cfg(cfg, in_wh)
    assert [(x.min_size, x.max_size, x.hflip) for x in v] == [
        (600, 1000, False), (600, 1000, True), (400, 1200, False), (400, 1200, True), (800, 1200, False), (800, 1200, True)]
    for x in v:
        h, w = feed.get_size(in_wh, x.min_size, x.max_size)
        assert x.size == (w, h)
    assert v[4].size == (1200, 675)         # 800 would give 1422 > MAX_SIZE: the long side is capped
    cfg.TEST.BBOX_AUG.SCALES = tuple(range(100, 900, 100))
    with pytest.raises(ValueError):
        bbox_aug.views_from_cfg(cfg, in_wh)  # 2 + 2 * 8 = 18 views > 16


def test_twin_transpose_and_resize_round_like_boxlist():
    b = np.array([[10.25, 3.0, 20.5, 7.75]], f32)
    t = tw.transpose(b, 101)
    assert t.tolist() == [[101 - 20.5 - 1, 3.0, 101 - 10.25 - 1, 7.75]]
    r = tw.resize(b, (300, 200), (150, 300))            # unequal ratios: x * 2, y * (2/3 in f32)
    assert r[0, 0] == f32(10.25) * f32(2.0) and r[0, 1] == f32(3.0) * f32(200.0 / 300.0)
    r = tw.resize(b, (100, 60), (300, 180))             # equal ratios: one f32 multiply by f32(1/3)
    assert r[0, 2] == f32(20.5) * f32(1.0 / 3.0) and r[0, 3] == f32(7.75) * f32(60.0 / 180.0)


def test_twin_filter_results_hand_computed():
    # class 1: three boxes; rows 0 and 2 overlap (IoU 0.9 > 0.5), row 2 scores higher -> row 0 suppressed; row 1 apart
    boxes = np.array([[[0, 0, 9, 9], [50, 50, 59, 59], [0, 0, 9, 10]]], f32)
    scores = np.array([[0.6, 0.3, 0.8]], f32)
    ob, os_, ol = tw.filter_results(boxes, scores)
    assert ol.tolist() == [1, 1] and os_.tolist() == [f32(0.3), f32(0.8)]      # kept rows ascending: 1, 2
    # exact tie at the k-th value: both kept (torch.kthvalue + >=)
    boxes = np.array([[[0, 0, 9, 9], [50, 50, 59, 59], [100, 0, 109, 9]]], f32)
    scores = np.array([[0.5, 0.4, 0.4]], f32)
    ob, os_, ol = tw.filter_results(boxes, scores, max_det=2)
    assert len(os_) == 3
    ob, os_, ol = tw.filter_results(boxes, scores, max_det=1)
    assert os_.tolist() == [f32(0.5)]
    # a flipped view's box lands on the identity view's one and is suppressed by it
    v0 = (np.array([[[10, 5, 29, 25]]], f32), np.array([[0.9]], f32))
    v1 = (np.array([[[100 - 29 - 1, 5, 100 - 10 - 1, 25]]], f32), np.array([[0.7]], f32))
    ob, os_, ol = tw.merge([v0, v1], [(100, 50), (100, 50)], [False, True])
    assert os_.tolist() == [f32(0.9)] and ob.tolist() == [[10, 5, 29, 25]]


def test_twin_single_identity_view_is_filter_results():
    views, sizes = tw.random_views(3, 1, 60, C1=4, grid=20)
    a = tw.merge(views, sizes, [False])
    b = tw.filter_results(*views[0])
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def _ref_views(d, nc=31):
    """the recorded per-view candidates of frame 0 (R * NC rows, proposal-major, background included) -> the twin's
    class-major (boxes [NC-1,R,4], scores [NC-1,R]) without the background class"""
    views, sizes = [], []
    for k in range(4):
        b, s = d["cand_boxes_v%d" % k], d["cand_scores_v%d" % k]
        R = s.shape[0] // nc
        views.append((np.ascontiguousarray(b.reshape(R, nc, 4)[:, 1:].transpose(1, 0, 2)),
                      np.ascontiguousarray(s.reshape(R, nc)[:, 1:].T)))
        sizes.append(tuple(int(x) for x in d["cand_size_v%d" % k]))
    return views, sizes, [bool(x) for x in d["view_flip"]]


def test_twin_merge_reproduces_the_reference_fixture():
    """tests/golden/ref_bbox_aug.npz (the reference's unmodified im_detect_bbox_aug, see make_bbox_aug.py): the twin's
    merge of the recorded per-view candidates == the recorded merged detections, bit for bit -- identity, flip, an
    unequal-ratio scale (145x97 of 192x128) and its flip, CPU NMS rule (IoU >= thr)"""
    import os
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_bbox_aug.npz"))
    views, sizes, flips = _ref_views(d)
    assert sizes == [(192, 128), (192, 128), (145, 97), (145, 97)] and flips == [False, True, False, True]
    assert 145 / 192 != 97 / 128
    wb, ws, wl = tw.merge(views, sizes, flips, strict_gt=False)
    assert len(ws) == len(d["scores0"]) > 0
    np.testing.assert_array_equal(wl, d["labels0"])
    np.testing.assert_array_equal(ws.view(np.uint32), d["scores0"].view(np.uint32))
    np.testing.assert_array_equal(wb.view(np.uint32), d["boxes0"].view(np.uint32))
    # the view sizes are views_from_cfg's for the fixture's settings
    cfg = config.get_cfg("R-50", "base")
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = int(d["cfg_min_size"]), int(d["cfg_max_size"])
    cfg.merge_from_list(["TEST.BBOX_AUG.ENABLED", True, "TEST.BBOX_AUG.H_FLIP", True,
                         "TEST.BBOX_AUG.SCALES", (int(d["cfg_scale"]),), "TEST.BBOX_AUG.MAX_SIZE", int(d["cfg_aug_max_size"]),
                         "TEST.BBOX_AUG.SCALE_H_FLIP", True])
    v = bbox_aug.views_from_cfg(cfg, (int(d["cfg_W"]), int(d["cfg_H"])))
    assert [x.size for x in v] == sizes and [x.hflip for x in v] == flips
