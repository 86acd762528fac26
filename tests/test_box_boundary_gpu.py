"""-m gpu: the box selection kernels of csrc/boxes.hip ON their decision boundaries -- the cases of
tests/box_boundary_cases.py (proved on the CPU by tests/test_box_boundary_cases.py) against the oracle: IoUs inside the
quotient band of dev_suppresses_areas, chains with closed-form keep sets across 64-box blocks and 1024-box windows, ties and
signed zeros across the top-k cut, ulp ladders for the radix select's lower passes, invalid candidates (remove_small_boxes),
clamped dw / dh, ragged nprop and score ties at the detections-per-image cut.  Indices, counts and labels bit for bit; boxes
within 1e-3 and scores within 1e-6, the tolerances of test_rpn_select / test_postprocess.  NaN scores are out of scope:
no caller orders them, the kernels' keys give them no defined rank."""
import numpy as np
import pytest
import torch

import box_boundary_cases as bc
from oracle import native

pytestmark = pytest.mark.gpu


def _ops():
    from mega.pytorch_amd import ops
    return ops


def _nms(dev, boxes, scores, thr, strict):
    return _ops().nms(torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), thr, strict_gt=strict).cpu().numpy()


# ===================================================================================================== ops.nms
@pytest.mark.parametrize("large", [False, True], ids=["scan-384", "lazy-2200"])
@pytest.mark.parametrize("thr", bc.THRS)
def test_nms_band_pairs(dev, thr, large):
    """IoU within 1e-5 of the threshold: the quotient path.  The decision must be the f32 quotient's, i.e. the device's
    division must round like the host's."""
    bs = bc.band_set(thr, large)
    for strict in (True, False):
        got = _nms(dev, bs.boxes, bs.scores, thr, strict)
        what = "band thr %g strict %s (%d boxes)" % (thr, strict, len(bs.boxes))
        bc.check_keep(got, native.nms(bs.boxes, bs.scores, thr, strict), what + " vs oracle")
        bc.check_keep(got, bc.band_keep(bs, strict), what + " vs quotient classes")


@pytest.mark.parametrize("n", bc.CHAIN_N)
def test_nms_chains(dev, n):
    """every box's fate hangs on its predecessor's: block edges (64), the scan / lazy switch (2048), window edges (1024)"""
    for (shift, thr), period in sorted(bc.CHAIN_PERIOD.items()):
        boxes, scores, rank = bc.chain(n, shift)
        want = bc.chain_keep(rank, period)
        for strict in (True, False):
            got = _nms(dev, boxes, scores, thr, strict)
            bc.check_keep(got, want, "chain n %d shift %d thr %g strict %s vs closed form" % (n, shift, thr, strict))
            bc.check_keep(got, native.nms(boxes, scores, thr, strict), "chain n %d shift %d thr %g vs oracle" % (n, shift, thr))


@pytest.mark.parametrize("n", [2049, 3073])
def test_nms_all_disjoint_and_all_identical(dev, n):
    for shift, period in ((100, 1), (0, n)):
        boxes, scores, rank = bc.chain(n, shift)
        for strict in (True, False):
            got = _nms(dev, boxes, scores, 0.5, strict)
            bc.check_keep(got, bc.chain_keep(rank, period), "n %d shift %d strict %s" % (n, shift, strict))
            bc.check_keep(got, native.nms(boxes, scores, 0.5, strict), "n %d shift %d vs oracle" % (n, shift))


@pytest.mark.parametrize("n", [200, 1500])
def test_nms_signed_zero_scores_are_ties(dev, n):
    """-0.0 == +0.0: a tie, ordered by index (score desc, index asc).  Box i at 20 * i, -0.0 on the even rows, +0.0 on the odd
    ones: by index every even row is kept; a key that ranks +0.0 first keeps the odd rows.  (NaN scores: out of scope.)"""
    i = np.arange(n)
    boxes = np.stack([i * 20, 0 * i, i * 20 + 99, 0 * i + 49], 1).astype(np.float32)
    scores = np.where(i % 2 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    want = native.nms(boxes, scores, 0.5, True)
    assert np.array_equal(want, i[::2])
    bc.check_keep(_nms(dev, boxes, scores, 0.5, True), want, "signed-zero scores, n %d" % n)


# ===================================================================================================== ops.rpn_select
def _rpn_select(dev, cases, want_index):
    c = cases[0]
    rpn_out = torch.stack([k.rpn_out() for k in cases]).to(dev)
    return [t.cpu() for t in _ops().rpn_select(rpn_out, c.cell.to(dev), c.Hf, c.Wf, 16, c.pre, c.post, c.thr, c.min_size, c.im_w,
                                               c.im_h, True, want_index=want_index)]


def _check_rpn_launch(dev, names):
    cases = [bc.rpn_case(n) for n in names]
    props, scores, cnt, index = _rpn_select(dev, cases, True)
    p2, s2, c2 = _rpn_select(dev, cases, False)
    assert torch.equal(p2, props) and torch.equal(s2, scores) and torch.equal(c2, cnt), "without want_index the result differs"
    for b, case in enumerate(cases):
        f = case.facts
        what = "%s (frame %d of %d; n_gt %d, take_eq %d of %d ties, %.0f %% invalid)" % (
            case.name, b, len(cases), f["n_gt"], f["take_eq"], f["n_eq"], 100 * f["invalid_share"])
        bc.check_rpn((props[b], scores[b], int(cnt[b]), index[b]), case.oracle(), what)


@pytest.mark.parametrize("name", [s.name for s in bc.RPN_SPECS])
def test_rpn_select_boundary_case(dev, name):
    _check_rpn_launch(dev, [name])


@pytest.mark.parametrize("names", bc.rpn_batches(), ids=lambda n: "+".join(n))
def test_rpn_select_three_cases_in_one_launch(dev, names):
    _check_rpn_launch(dev, names)


# ===================================================================================================== ops.postprocess
def _post_args(c):
    return (c.weights, c.im_w, c.im_h, c.score_thresh, c.nms, c.max_det, True)


def _postprocess(dev, c):
    nprop = torch.tensor([c.nprop], dtype=torch.int32, device=dev)
    return _ops().postprocess(c.logits.to(dev), c.deltas.to(dev), c.props.to(dev), nprop, *_post_args(c))


@pytest.mark.parametrize("name", sorted(bc.POST_BY_NAME))
def test_postprocess_boundary_case(dev, name):
    c = bc.post_case(name)
    ob, os_, ol, oc = _postprocess(dev, c)
    f = c.facts
    bc.check_post((ob.cpu(), os_.cpu(), ol.cpu(), int(oc.item())), c.reference(),
                  "%s (nprop %d of %d, D %d against max_det %d, %d ties at the cut)" % (name, c.nprop, c.R, f["D"], c.max_det, f["ties_at_cut"]))


@pytest.mark.parametrize("names", bc.POST_BATCHES, ids=lambda n: "+".join(n))
def test_postprocess_batched_ragged_nprop(dev, names):
    cases = [bc.post_case(n) for n in names]
    nprop = torch.tensor([c.nprop for c in cases], dtype=torch.int32, device=dev)
    ob, os_, ol, oc = _ops().postprocess_batched(torch.cat([c.logits for c in cases]).to(dev), torch.cat([c.deltas for c in cases]).to(dev),
                                                 torch.cat([c.props for c in cases]).to(dev), len(cases), *_post_args(cases[0]), nprop=nprop)
    for b, c in enumerate(cases):
        n = int(oc[b].item())
        bc.check_post((ob[b].cpu(), os_[b].cpu(), ol[b].cpu(), n), c.reference(), "%s (image %d of the batch, nprop %d)" % (c.name, b, c.nprop))
        wb, ws, wl, wc = _postprocess(dev, c)             # every image has the bits of its own call
        assert int(wc.item()) == n
        assert torch.equal(ob[b, :n], wb[:n]) and torch.equal(os_[b, :n], ws[:n]) and torch.equal(ol[b, :n], wl[:n]), c.name
