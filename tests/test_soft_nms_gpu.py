"""GPU: ops.soft_merge (csrc/soft_nms.hip) against the numpy twin tests/soft_nms_twin.py -- both options off against
ops.bbox_aug_merge, linear soft-NMS bit for bit (also with exact score ties and IoU == threshold pairs), gaussian within
the tolerance its expf leaves, box voting after the greedy NMS and after soft-NMS, the edges and the limits -- and
inference() with TEST.SOFT_NMS + TEST.BBOX_VOTE against the hand-assembled path.

Tolerances.  Linear: f32 multiply, subtract and a correctly rounded divide only: bits.  Gaussian: every factor carries a
few f32 ulps (2^-22) from expf and a score is a product of at most 111 factors (the fixtures' live rows per class):
111 * 2^-22 = 2.6e-5, rtol 1e-4; the fixtures keep every selection and threshold crossing 1e-3 away from flipping
(tests/test_soft_nms.py::test_gpu_fixture_preconditions).  Voting: f64 sums, one rounding to f32: 1e-3 px is 16 ulps at
coordinate 1000; "AVG" rtol 1e-6."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bbox_aug_twin as bt
import soft_nms_twin as tw
from mega.pytorch_amd import _lib, bbox_aug, inference, ops

pytestmark = pytest.mark.gpu

KR = sorted(tw.FIXTURE_SEEDS)              # K in {1, 3} x R in {1, 37, 300}
f32 = np.float32


def _bits(a):
    return np.asarray(a, f32).view(np.uint32)


def _stack(frames, dev):
    K = len(frames[0])
    cb = torch.from_numpy(np.stack([np.stack([fr[k][0] for fr in frames]) for k in range(K)])).to(dev).contiguous()
    cs = torch.from_numpy(np.stack([np.stack([fr[k][1] for fr in frames]) for k in range(K)])).to(dev).contiguous()
    return cb, cs


_GPU_KW = {"soft_method": "soft_method", "sigma": "sigma", "vote_on": "vote", "vote_thresh": "vote_thresh",
           "vote_scoring": "vote_scoring"}


def _gpu(dev, frames, sizes, flips, max_det=300, strict_gt=True, **kw):
    """-> per frame (boxes, scores, labels) numpy, the first counts[f] rows"""
    cb, cs = _stack(frames, dev)
    ob, os_, ol, oc = ops.soft_merge(cb, cs, sizes, flips, 0.001, 0.5, max_det, strict_gt,
                                     **{_GPU_KW[k]: v for k, v in kw.items()})
    ob, os_, ol = ob.cpu().numpy(), os_.cpu().numpy(), ol.cpu().numpy()
    return [(ob[f, :n], os_[f, :n], ol[f, :n]) for f, n in enumerate(oc.tolist())]


@functools.lru_cache(maxsize=None)
def _fixture(name, K, R):
    if name == "tie":
        frames = []
        for f in range(2):
            v, sizes, flips = tw.tie_views(100 * K + R + f, K, R)
            frames.append(v)
        return frames, sizes, flips
    return tw.fixture(K, R)


@functools.lru_cache(maxsize=None)
def _twin(name, K, R, max_det, strict_gt, kw):
    """the twin's result per frame, computed once per case and shared"""
    frames, sizes, flips = _fixture(name, K, R)
    return [tw.merge(fr, sizes, flips, max_det=max_det, strict_gt=strict_gt, **dict(kw)) for fr in frames]


def _case(dev, name, K, R, max_det=300, strict_gt=True, **kw):
    frames, sizes, flips = _fixture(name, K, R)
    got = _gpu(dev, frames, sizes, flips, max_det, strict_gt, **kw)
    want = _twin(name, K, R, max_det, strict_gt, tuple(sorted(kw.items())))
    assert len(got) == len(want) == 2
    for f, (g, w) in enumerate(zip(got, want)):
        assert len(g[1]) == len(w[1]), "frame %d: %d rows, twin %d" % (f, len(g[1]), len(w[1]))
        np.testing.assert_array_equal(g[2], w[2])
    return got, want


def _assert_bits(got, want):
    for g, w in zip(got, want):
        np.testing.assert_array_equal(_bits(g[1]), _bits(w[1]))
        np.testing.assert_array_equal(_bits(g[0]), _bits(w[0]))


@pytest.mark.parametrize("K,R", KR)
def test_both_off_is_bbox_aug_merge(dev, K, R):
    frames, sizes, flips = _fixture("clustered", K, R)
    cb, cs = _stack(frames, dev)
    for strict in (True, False):
        a = ops.soft_merge(cb, cs, sizes, flips, 0.001, 0.5, 300, strict)
        b = ops.bbox_aug_merge(cb, cs, sizes, flips, 0.001, 0.5, 300, strict)
        assert torch.equal(a[3], b[3])
        for f, n in enumerate(b[3].tolist()):
            assert all(torch.equal(x[f, :n], y[f, :n]) for x, y in zip(a[:3], b[:3]))
    assert int(b[3].sum()) > 0


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("K,R", KR)
def test_linear_equals_twin_bit_for_bit(dev, K, R, strict):
    _assert_bits(*_case(dev, "clustered", K, R, max_det=0, strict_gt=strict, soft_method="linear"))


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("K,R", [(1, 37), (3, 37), (3, 300)])
def test_linear_with_score_ties_and_iou_equal_to_the_threshold(dev, K, R, strict):
    """integer boxes, scores k / 8: equal scores are selected by row, IoU == 0.5 pairs decay only under >="""
    got, want = _case(dev, "tie", K, R, max_det=0, strict_gt=strict, soft_method="linear")
    _assert_bits(got, want)
    if strict:      # the two comparisons give different results on this fixture: the threshold pairs are there
        other = _twin("tie", K, R, 0, False, (("soft_method", "linear"),))
        assert any(len(a[1]) != len(b[1]) or (a[1] != b[1]).any() for a, b in zip(want, other))


@pytest.mark.parametrize("K,R", KR)
def test_gaussian_equals_twin(dev, K, R):
    got, want = _case(dev, "clustered", K, R, max_det=0, soft_method="gaussian", sigma=tw.FIXTURE_SIGMA)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(_bits(g[0]), _bits(w[0]))         # the kept rows' own boxes: the same kept set
        err = np.abs(g[1].astype(np.float64) - w[1]) / w[1]
        print("K=%d R=%d: %d kept, max relative score error %.3e" % (K, R, len(w[1]), err.max() if len(err) else 0.0))
        np.testing.assert_allclose(g[1], w[1], rtol=1e-4, atol=0)


@pytest.mark.parametrize("scoring", ["ID", "AVG"])
@pytest.mark.parametrize("soft", [None, "linear"])
@pytest.mark.parametrize("K,R", KR)
def test_voting_equals_twin(dev, K, R, soft, scoring):
    kw = dict(vote_on=True, vote_thresh=0.8, vote_scoring=scoring)
    if soft:
        kw["soft_method"] = soft
    got, want = _case(dev, "clustered", K, R, max_det=0, **kw)
    plain, _ = _case(dev, "clustered", K, R, max_det=0, **({"soft_method": soft} if soft else {}))
    moved = 0
    for g, w, p in zip(got, want, plain):
        assert len(p[1]) == len(g[1])                                    # voting changes no kept set
        err = np.abs(g[0].astype(np.float64) - w[0])
        print("K=%d R=%d %s %s: max box error %.3e px" % (K, R, soft, scoring, err.max() if err.size else 0.0))
        np.testing.assert_allclose(g[0], w[0], rtol=0, atol=1e-3)
        if scoring == "ID":
            np.testing.assert_array_equal(_bits(g[1]), _bits(w[1]))
            np.testing.assert_array_equal(_bits(g[1]), _bits(p[1]))
        else:
            np.testing.assert_allclose(g[1], w[1], rtol=1e-6, atol=0)
        moved += int((g[0] != p[0]).any())
    assert moved or R == 1


# ------------------------------------------------------------------------------------------------ edges
MODES = [dict(soft_method="linear"), dict(soft_method="gaussian"), dict(vote_on=True),
         dict(soft_method="linear", vote_on=True, vote_scoring="AVG")]


@pytest.mark.parametrize("kw", MODES, ids=["linear", "gaussian", "vote", "linear+vote"])
def test_empty_class_empty_frame_and_single_row(dev, kw):
    sizes, flips = tw.VIEW_SIZES[:3], tw.VIEW_FLIPS[:3]
    a, _, _ = tw.clustered_views((53, 54, 55), 3, 37, p_live=0.6, empty_classes=(1,))      # class 2 has no live row
    b = [(x, np.full_like(s, -1)) for x, s in a]                                             # a frame with none
    c = [(x, s.copy()) for x, s in b]
    c[1][1][2, 20] = 0.7                                                                      # a single live row, in the flipped view
    got = _gpu(dev, [a, b, c], sizes, flips, **kw)
    st = {}
    want = [tw.merge(fr, sizes, flips, stats=st, **kw) for fr in (a, b, c)]
    if kw.get("soft_method") == "gaussian":      # as for the seeded fixtures: nothing within 1e-3 of flipping
        assert st.get("gap", 1) >= 1e-3 and st.get("thresh", 1) >= 1e-3
    assert len(got[1][1]) == 0 and len(want[1][1]) == 0
    assert 2 not in got[0][2] and 1 in got[0][2] and 3 in got[0][2]
    assert got[2][2].tolist() == [3] and got[2][1].tolist() == [f32(0.7)]
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g[2], w[2])
        np.testing.assert_allclose(g[1], w[1], rtol=1e-4, atol=0)
        np.testing.assert_allclose(g[0], w[0], rtol=0, atol=1e-3)
    mb, _ = tw.map_views(c, sizes, flips)
    np.testing.assert_array_equal(_bits(got[2][0][0]), _bits(mb[2, 37 + 20]))


def test_max_det_cut_keeps_the_ties_of_the_kth_score(dev):
    got, want = _case(dev, "tie", 3, 37, max_det=7, soft_method="linear")
    _assert_bits(got, want)
    assert any(len(w[1]) > 7 for w in want)      # the 7th score is tied: every row with it stays
    full = _twin("tie", 3, 37, 0, True, (("soft_method", "linear"),))
    assert all(len(w[1]) < len(u[1]) for w, u in zip(want, full))


def test_the_row_limit_8192_against_the_twin(dev):
    """K = 16 views x 512 rows = 8192 rows per class exactly (8 rows a thread), one frame, two classes, scores on a grid
    (ties): linear soft-NMS bit for bit, then with voting"""
    sizes = [(120 + 7 * k, 80 + 3 * (k % 5)) for k in range(16)]
    flips = [k % 2 == 1 for k in range(16)]
    v, _ = bt.random_views(77, 16, 512, C1=2, sizes=sizes, grid=50, p_live=0.5)
    (g,) = _gpu(dev, [v], sizes, flips, max_det=0, soft_method="linear")
    w = tw.merge(v, sizes, flips, max_det=0, soft_method="linear")
    assert len(w[1]) > 2000
    np.testing.assert_array_equal(g[2], w[2])
    _assert_bits([g], [w])
    (g,) = _gpu(dev, [v], sizes, flips, max_det=300, soft_method="linear", vote_on=True, vote_scoring="AVG")
    w = tw.merge(v, sizes, flips, max_det=300, soft_method="linear", vote_on=True, vote_scoring="AVG")
    np.testing.assert_array_equal(g[2], w[2])
    np.testing.assert_allclose(g[1], w[1], rtol=1e-6, atol=0)
    np.testing.assert_allclose(g[0], w[0], rtol=0, atol=1e-3)
    # 2 and 4 rows a thread
    for K, R in ((2, 1000), (4, 1000)):
        v, _ = bt.random_views(78, K, R, C1=2, sizes=sizes[:K], grid=50, p_live=0.5)
        (g,) = _gpu(dev, [v], sizes[:K], flips[:K], max_det=0, strict_gt=False, soft_method="linear")
        w = tw.merge(v, sizes[:K], flips[:K], max_det=0, strict_gt=False, soft_method="linear")
        np.testing.assert_array_equal(g[2], w[2])
        _assert_bits([g], [w])


# ------------------------------------------------------------------------------------------------ limits
def _raw_call(dev, K=1, F=1, R=4, NC=3, ws_short=0, soft_method=1, sigma=0.5, vote=1, vote_thresh=0.8, vote_scoring=0,
              alloc=True):
    """mega_soft_merge itself on a tiny valid problem (buffers sized for it; alloc=False: for calls that must return
    before any launch, with ws_bytes = 0 so that a regressed check stops at MEGA_ERR_WS) -> (rc, outputs untouched)"""
    lib = _lib.load()
    C1 = NC - 1
    n = K * F * C1 * R if alloc else 16
    cb = torch.zeros((n, 4), device=dev)
    cs = torch.full((n,), 0.5, device=dev)
    cap = C1 * K * R if alloc else 16
    ob = torch.full((F, cap, 4), 7.0, device=dev)
    os_ = torch.full((F, cap), 7.0, device=dev)
    ol = torch.full((F, cap), 7, dtype=torch.int64, device=dev)
    oc = torch.full((F,), 7, dtype=torch.int32, device=dev)
    nb = lib.mega_soft_merge_workspace_bytes(F, K, R, NC) if alloc else 0
    ws = torch.zeros((max(nb, 16),), dtype=torch.uint8, device=dev)
    arr = (ctypes.c_int * K)(*([10] * K))
    zero = (ctypes.c_int * K)(*([0] * K))
    vp = ctypes.c_void_p
    rc = lib.mega_soft_merge(cb.data_ptr(), cs.data_ptr(), F, K, R, NC, ctypes.cast(arr, vp), ctypes.cast(arr, vp),
                             ctypes.cast(zero, vp), 0.001, 0.5, 1, soft_method, sigma, vote, vote_thresh, vote_scoring, 300,
                             ob.data_ptr(), os_.data_ptr(), ol.data_ptr(), oc.data_ptr(), ws.data_ptr(), nb - ws_short, None)
    torch.cuda.synchronize(dev)
    untouched = bool((ob == 7).all() and (os_ == 7).all() and (ol == 7).all() and (oc == 7).all())
    return rc, untouched


def test_limits_and_bad_arguments_return_before_any_launch(dev):
    assert _raw_call(dev)[0] == 0                                        # the tiny problem itself is valid
    assert _raw_call(dev, K=1, R=8193, alloc=False) == (4, True)         # MEGA_ERR_LIMIT
    assert _raw_call(dev, K=17, R=4, alloc=False) == (4, True)
    for bad in (dict(soft_method=3), dict(soft_method=-1), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")),
                dict(vote_thresh=0.0), dict(vote_thresh=1.5), dict(vote=2), dict(vote_scoring=2)):
        assert _raw_call(dev, **bad) == (1, True), bad                   # MEGA_ERR_ARG
    assert _raw_call(dev, ws_short=1) == (3, True)                       # MEGA_ERR_WS
    cs = torch.full((1, 1, 2, 8193), -1.0, device=dev)
    cb = torch.zeros((1, 1, 2, 8193, 4), device=dev)
    with pytest.raises(ValueError):
        ops.soft_merge(cb, cs, [(10, 10)], [False], 0.001, 0.5, 300, soft_method="linear")
    cs = torch.full((17, 1, 2, 4), -1.0, device=dev)
    cb = torch.zeros((17, 1, 2, 4, 4), device=dev)
    with pytest.raises(ValueError):
        ops.soft_merge(cb, cs, [(10, 10)] * 17, [False] * 17, 0.001, 0.5, 300, vote=True)
    for bad in (dict(soft_method="quadratic"), dict(sigma=0), dict(vote_thresh=0), dict(vote_scoring="MAX")):
        with pytest.raises(ValueError):
            ops.soft_merge(cb[:1], cs[:1], [(10, 10)], [False], 0.001, 0.5, 300, **bad)


# ------------------------------------------------------------------------------------------------ inference() end to end
@pytest.mark.parametrize("hflip", [False, True])
def test_inference_soft_nms_and_vote_equals_the_hand_assembled_path(dev, tmp_path, hflip):
    """the R-50 base detector on the small synthetic clip with SOFT_NMS linear + BBOX_VOTE (and BBOX_AUG.H_FLIP):
    inference() == candidate-mode run -> stack_candidates -> ops.soft_merge"""
    from test_bbox_aug_gpu import L, _model, _same, _video
    from mega.pytorch_amd import feed
    img_dir, idx = _video(tmp_path)
    cfg, model = _model(dev, "base")
    cfg.TEST.SOFT_NMS.ENABLED = True
    cfg.TEST.BBOX_VOTE.ENABLED = True
    if hflip:
        cfg.TEST.BBOX_AUG.ENABLED = True
        cfg.TEST.BBOX_AUG.H_FLIP = True
    got = inference.inference(cfg, model, img_dir, idx, output_folder=str(tmp_path / "soft"))
    pp = model.roi_heads.box.post_processor
    assert not pp.candidates and len(got) == L
    # by hand
    run = inference._video_runner(model, 10, 0, None)
    v = inference.VIDTestIndex(idx).videos[0]
    per_view = []
    with bbox_aug.candidate_mode(model), torch.no_grad():
        for flip in ([False, True] if hflip else [False]):
            src = feed.FrameSource(img_dir + "/%s.JPEG", v["pattern"], L, dev, min_size=180, max_size=320, hflip=flip)
            per_view.append(bbox_aug.stack_candidates(run(src, v), 31))
            src.close()
    cb = torch.stack([b for b, _ in per_view]).contiguous()
    cs = torch.stack([s for _, s in per_view]).contiguous()
    K = len(per_view)
    ob, os_, ol, oc = ops.soft_merge(cb, cs, [(320, 180)] * K, [False, True][:K], pp.score_thresh, pp.nms,
                                     pp.detections_per_img, pp.strict_gt, soft_method="linear", vote=True, vote_thresh=0.8,
                                     vote_scoring="ID")
    for f, n in enumerate(oc.tolist()):
        g = got[f]
        assert g.size == (320, 180) and len(g) == n
        assert torch.equal(g.bbox, ob[f, :n].cpu()) and torch.equal(g.get_field("scores"), os_[f, :n].cpu())
        assert torch.equal(g.get_field("labels"), ol[f, :n].cpu())
    _same(got, inference.load_predictions(str(tmp_path / "soft" / "predictions.pth")))
    assert sum(len(g) for g in got) > 0
