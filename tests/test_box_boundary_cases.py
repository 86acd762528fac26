"""The boundary cases of tests/box_boundary_cases.py, proved on the CPU with the oracle alone before the GPU file trusts
them: (1) every case has the facts it claims -- the band classes, the closed-form chain keep sets, n_gt / take_eq and the
chunks the ties fall in, the invalid share, the clamped deltas, D against max_det, the margins; (2) the comparison helpers
the GPU file uses reject an answer with one planted fault: tie order reversed, one invalid box let through, > swapped for
>=, the cut taken at max_det without ties, nprop ignored.  Each test prints its figures (run with -s to see them)."""
import numpy as np
import pytest
import torch

import box_boundary_cases as bc
from oracle import native

RPN_NAMES = [s.name for s in bc.RPN_SPECS]
POST_NAMES = sorted(bc.POST_BY_NAME)


# ===================================================================================================== band pairs, chains
@pytest.mark.parametrize("thr", bc.THRS)
def test_band_classes_and_the_oracles_decisions(thr):
    bp = bc.band_pairs(thr)
    print("thr %.1f: %s pairs in the band" % (thr, {c: len(bp[c]) for c in bc.CLASSES}))
    for c in bc.CLASSES:
        W, H, w, h = bp[c].T
        assert len(bp[c]) >= bc.PER_CLASS, (thr, c, len(bp[c]))
        assert (np.abs(w * h - thr * W * H) <= bc.BAND * thr * W * H).all() and (W * H + w * h < 1 << 24).all()
        assert (bc.quotient_class(bp[c], thr) == bc.CLASSES.index(c) - 1).all()
    for large in (False, True):
        bs = bc.band_set(thr, large)
        assert len(bs.boxes) == (2200 if large else 6 * bc.PER_CLASS) and float(np.abs(bs.boxes).max()) < 1 << 20
        assert all(int((bs.cls == v).sum()) >= bc.PER_CLASS for v in (-1, 0, 1))
        assert np.array_equal(bs.boxes, np.round(bs.boxes)) and (bs.scores[bs.outer] > bs.scores[bs.inner]).all()
        for strict in (True, False):          # every pair's decision, from the oracle, is the f32 quotient's
            bc.check_keep(native.nms(bs.boxes, bs.scores, thr, strict), bc.band_keep(bs, strict), "band %g %s" % (thr, strict))
        # planted fault: > swapped for >= changes the answer on the equal class, and only there
        diff = np.setxor1d(bc.band_keep(bs, True), bc.band_keep(bs, False))
        assert np.array_equal(diff, np.sort(bs.inner[bs.cls == 0]))
        with pytest.raises(AssertionError, match="only in got"):
            bc.check_keep(bc.band_keep(bs, True), bc.band_keep(bs, False), "> for >=")


@pytest.mark.parametrize("shift,thr", sorted(bc.CHAIN_PERIOD))
def test_chain_keep_sets_in_closed_form(shift, thr):
    period = bc.CHAIN_PERIOD[(shift, thr)]
    for n in (65, 1025, 3073):
        boxes, scores, rank = bc.chain(n, shift)
        assert not np.array_equal(rank, np.arange(n)) and np.array_equal(np.sort(rank), np.arange(n))
        for strict in (True, False):
            bc.check_keep(native.nms(boxes, scores, thr, strict), bc.chain_keep(rank, period), "chain %d" % n)
    print("shift %d thr %.1f: every %d. box kept" % (shift, thr, period))


def test_chain_all_disjoint_and_all_identical():
    for n in (2049, 3073):
        for shift, period in ((100, 1), (0, n)):
            boxes, scores, rank = bc.chain(n, shift)
            want = bc.chain_keep(rank, period)
            assert len(want) == (n if shift else 1)
            for strict in (True, False):
                bc.check_keep(native.nms(boxes, scores, 0.5, strict), want, "chain %d shift %d" % (n, shift))


# ===================================================================================================== RPN cases
@pytest.mark.parametrize("name", RPN_NAMES)
def test_rpn_case_facts(name):
    case = bc.rpn_case(name)
    spec, f = case.spec, case.facts
    NA = case.logit.numel()
    print("%s (seed %d): n_gt %d, ties %d in chunks %s, take_eq %d; invalid %.1f %%, first block invalid %s; clamped %d "
          "(visible %d), columns %d; margins side %.3g IoU %.3g; kept %d" % (
              name, case.seed, f["n_gt"], f["n_eq"], f["tie_chunks"], f["take_eq"], 100 * f["invalid_share"],
              f["first_block_invalid"], f["clamped"], f["clamp_visible"], f["columns"], f["side_margin"], f["iou_margin"], f["kept"]))
    assert f["n_gt"] + f["take_eq"] == spec.k and f["take_eq"] <= f["n_eq"] and f["side_margin"] >= bc.MARGIN and f["iou_margin"] >= bc.MARGIN
    nchunk = (NA + 1023) // 1024
    kind = spec.logit[0]
    if kind == "ties":
        T, n_eq, take_eq, where = spec.logit[1:]
        assert (f["T"], f["n_eq"], f["take_eq"], f["n_gt"]) == (T, n_eq, take_eq, spec.k - take_eq)
        assert f["tie_chunks"] == ([nchunk - 1] if where == "last" else list(range(nchunk)))
    elif kind == "equal":
        assert (f["n_gt"], f["n_eq"], f["take_eq"]) == (0, NA, spec.k)
    elif kind == "zeros":
        n_neg, n_pos, take_eq = spec.logit[1:]
        assert (f["T"], f["n_eq"], f["take_eq"]) == (0.0, n_neg + n_pos, take_eq) and f["tie_chunks"] == list(range(nchunk))
        zeros = (case.logit == 0).nonzero().squeeze(1)
        neg = torch.signbit(case.logit[zeros])
        assert int(neg.sum()) == n_neg and bool(neg[:n_neg].all())                   # -0.0 at lower indices than +0.0
        if take_eq < n_neg + n_pos:        # the cut falls inside the zeros: by value +0.0 first, by the rule the lower indices
            assert set(case.order[f["n_gt"]:].tolist()) == set(zeros[:take_eq].tolist())
    else:
        if spec.logit == bc.L1:
            assert f["keys_sharing_top3"] >= 256 and f["top3_prefixes"] == 1           # only the last radix pass decides
        else:
            assert f["top3_prefixes"] >= 2 and len(set((bc.sortable_key(case.logit.numpy()) >> 16).tolist())) >= 2
        assert f["take_eq"] < f["n_eq"] or spec.k == NA
    if spec.k == NA:
        assert f["take_eq"] == f["n_eq"]                                                # no cut
    # deltas
    if "two_sizes" in spec.delta:
        assert 0.10 <= f["invalid_share"] <= 0.90 and spec.min_size == 30
    if "block0" in spec.delta:
        assert f["first_block_invalid"] and spec.min_size == 2 and f["invalid_share"] >= 64 / spec.k
    if spec.min_size == 0:
        assert f["invalid_share"] == 0
    assert "clamp" in spec.delta and f["clamped"] >= 2 and f["clamp_visible"] == f["clamped"]    # unclamped, the box would differ
    if "column" in spec.delta:
        assert f["columns"] == 8
    # the step-by-step reference is the oracle
    for got, want in zip(case.reference(), case.oracle()):
        assert torch.equal(got, want)
    assert case.post in (1, 63, 64, 65, 300) and case.reference()[0].shape[0] == f["kept"] <= case.post
    # G = 3: the max_keep stop; larger G: the walk reaches the last candidate, so the ties at the cut show in the answer
    assert (f["kept"] == case.post) if spec.G == 3 else (f["kept"] < case.post)


def test_rpn_cases_cover_the_forms():
    ks = {(s.Hf * s.Wf * 12, s.k, s.post) for s in bc.RPN_SPECS}
    lazy = {(na, k, p) for na, k, p in ks if k >= 1024 and (4 * p <= k or k > 2048)}
    assert {na for na, _, _ in ks} == {648, 1920, 2592} and lazy and ks - lazy
    assert any(k < 1024 for _, k, _ in ks - lazy) and any(k >= 1024 for _, k, _ in ks - lazy)      # scan: <= 16 and > 16 blocks
    assert any(k > 2048 for _, k, _ in lazy) and any(k <= 2048 for _, k, _ in lazy)                # lazy: one and several windows
    assert {s.post for s in bc.RPN_SPECS} == {1, 63, 64, 65, 300} and {s.min_size for s in bc.RPN_SPECS} == {0, 2, 30}
    assert len(bc.rpn_batches()) >= 4
    # the key twin: order, ties, signed zeros
    x = np.array([-np.inf, -2.0, -1e-30, -0.0, 0.0, 1e-30, 1.0, np.nextafter(np.float32(1), np.float32(2)), np.inf], dtype=np.float32)
    key = bc.sortable_key(x).astype(np.int64)
    assert key[3] == key[4] and (np.diff(key)[[0, 1, 2, 4, 5, 6, 7]] > 0).all()


@pytest.mark.parametrize("name", ["s-ties-half", "m-zeros", "l-ties-half", "l-ladder"])
def test_check_rpn_rejects_a_reversed_tie_order(name):
    case = bc.rpn_case(name)
    want = case.reference()
    bc.check_rpn(bc.rpn_output(want, case.post), want, name)
    bad = case.reference(fault="tie_reversed")
    assert not torch.equal(bad[2], want[2])
    with pytest.raises(AssertionError, match="kept anchor indices differ|kept .* vs oracle"):
        bc.check_rpn(bc.rpn_output(bad, case.post), want, name)


def test_check_rpn_rejects_the_value_order_of_signed_zeros():
    """what a key that ranks +0.0 above -0.0 selects (the +0.0 anchors first) is not the oracle's answer"""
    case = bc.rpn_case("m-zeros")
    lg = case.logit.clone()
    lg[(lg == 0) & ~torch.signbit(lg)] = 1e-30                   # +0.0 strictly above -0.0, nothing else moves
    bad_order = torch.sort(-lg, stable=True)[1][:case.pre]
    assert set(bad_order.tolist()) != set(case.order.tolist())
    keep = case.facts["n_gt"]
    assert torch.equal(bad_order[:keep], case.order[:keep])


@pytest.mark.parametrize("name", ["s-nocut-equal", "m-negative-T", "m-scan-block0", "l-ties-1"])
def test_check_rpn_rejects_an_invalid_box_let_through(name):
    case = bc.rpn_case(name)
    want = case.reference()
    bad = case.reference(fault="invalid_through")
    with pytest.raises(AssertionError):
        bc.check_rpn(bc.rpn_output(bad, case.post), want, name)
    # and the padding rows: a stale row past the count, an index that is not -1
    out = list(bc.rpn_output(case.reference(), case.post + 1))
    bc.check_rpn(out, want, name)
    out[3] = out[3].clone()
    out[3][-1] = 0
    with pytest.raises(AssertionError, match="rows past the count"):
        bc.check_rpn(out, want, name)


# ===================================================================================================== post-processor cases
@pytest.mark.parametrize("name", POST_NAMES)
def test_post_case_facts(name):
    case = bc.post_case(name)
    spec, f = case.spec, case.facts
    print("%s (seed %d): nprop %d of R %d, NC %d; D %d against max_det %d -> kept %d, %d ties at the cut; clamped %d; dead rows %d NaN "
          "+ %d confident; margins IoU %.3g, score_thresh %.3g, score gap %.3g" % (
              name, case.seed, case.nprop, case.R, case.NC, f["D"], case.max_det, f["kept"], f["ties_at_cut"], f["clamped"],
              f["dead_nan"], f["dead_confident"], f["iou_margin"], f["thresh_margin"], f["score_gap"]))
    assert f["iou_margin"] >= bc.MARGIN and f["dead_nan"] + f["dead_confident"] == case.R - case.nprop
    assert case.R - case.nprop < 2 or (f["dead_nan"] > 0 and f["dead_confident"] > 0)
    assert bool((case.deltas[case.nprop:] == 1e30).all()) and (f["clamped"] > 0) == (spec.clamp and case.nprop > 0)
    for r in case.clamp_rows:
        assert float(case.deltas[r].max()) / case.weights[2] > bc.CLIP
    if case.nprop == 0:
        assert f["D"] == 0
    if spec.layout == "disjoint":
        assert f["D"] == case.nprop
        a, b = spec.ties or (0, 0)
        if f["D"] > case.max_det:
            assert f["ties_at_cut"] == a + b + 1 and f["kept"] == case.max_det + b
        else:
            assert f["kept"] == f["D"] and f["D"] in (0, case.max_det)
    elif case.max_det == 0:
        assert f["kept"] == f["D"] > 300
    elif f["D"] > case.max_det:
        assert f["kept"] == case.max_det and f["ties_at_cut"] == 1
    else:
        assert f["kept"] == f["D"]


def test_post_cases_cover_the_cut():
    facts = {n: bc.post_case(n).facts for n in POST_NAMES}
    md = {n: bc.post_case(n).max_det for n in POST_NAMES}
    assert any(f["D"] == md[n] > 0 for n, f in facts.items())                                       # D == max_det
    assert any(f["D"] == md[n] + 1 and f["kept"] == md[n] for n, f in facts.items())                # one past, one dropped
    assert any(f["D"] == md[n] + 1 and f["kept"] == md[n] + 1 for n, f in facts.items())            # one past, tied: all kept
    assert any(f["D"] > 3 * md[n] > 0 and f["kept"] > md[n] for n, f in facts.items())              # far past, tied at the cut
    assert {s.R for s in bc.POST_SPECS} == {1, 63, 64, 65, 300, 1024} and {s.NC for s in bc.POST_SPECS} == {2, 31}
    for R in (64, 300, 1024):
        assert {0, R // 2, R} <= {s.nprop for s in bc.POST_SPECS if s.R == R}
    assert {1, 0} <= {s.nprop for s in bc.POST_SPECS}
    for names in bc.POST_BATCHES:
        cs = [bc.post_case(n) for n in names]
        assert len({(c.R, c.NC, c.max_det, c.score_thresh) for c in cs}) == 1
        assert 0 in [c.nprop for c in cs] and len({c.nprop for c in cs}) == len(cs)


@pytest.mark.parametrize("name", ["R65-D-max+1-tied", "R300-tied", "R300-nc2-half", "R1024-tied"])
def test_check_post_rejects_a_cut_without_ties(name):
    case = bc.post_case(name)
    b, s, l = want = case.reference()
    bc.check_post((b, s, l, len(s)), want, name)
    bad = case.reference(fault="cut_without_ties")
    assert bad[1].numel() == case.max_det < s.numel()
    with pytest.raises(AssertionError, match="detections vs oracle"):
        bc.check_post(bad + (case.max_det,), want, name)


@pytest.mark.parametrize("name", ["R63-half", "R64-none", "R300-nc2-half", "R300-one", "R1024-half"])
def test_check_post_rejects_nprop_ignored(name):
    case = bc.post_case(name)
    want = case.reference()
    bad = case.reference(fault="nprop_ignored")
    with pytest.raises(AssertionError):
        bc.check_post(bad + (bad[1].numel(),), want, name)
