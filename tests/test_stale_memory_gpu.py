"""-m gpu: no kernel's result depends on what its workspace or its output held before.

Every wrapper in mega/pytorch_amd/ops.py takes its workspace from ops._ws() and almost every output from torch.empty.  A test
process mostly sees fresh zero pages there; the clip engines replay hipGraphs on fixed buffers and see the previous
step-batch's values.  tests/poison.py makes the difference visible, and each case below asserts four things:

  1. two clean runs are bit-equal (no operation here uses float atomics: every case is compared bit for bit, none under a bound);
  2. under `zeros` and `ones` the defined part of every output is bit-equal to the clean run and passes the reference check
     the operation's own GPU test applies (the case builders, twins and references are those tests');
  3. under `replay` -- a bump allocator over one slab, rewound between calls -- a larger, different problem A runs first and
     then problem B on the same bytes: B is bit-equal to clean B; then B' (the shapes of B, other values) and B again, which
     catches an output region that is never written and would show B's own previous answer;
  4. the helper filled at least one allocation of the call.

"Defined part" is what the wrapper's docstring promises: rows below the count, keys below Nk, a channel slice.  A region a
wrapper leaves alone on purpose (the columns round deconv4x4s2_into's slice, the bytes round copy_blocks' destinations) is
checked the other way: it still holds the poison.

WS_OPS names the test of every function in ops.py whose source calls _ws(); tests/test_stale_memory.py (CPU) fails when a new
workspace operation has no entry here.  The whole-model cases run eagerly (graphs=False): the helper's fills are extra
launches and do not belong inside a graph capture."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bbox_aug_twin as bt
import box_boundary_cases as bc
import cpu_ops
import exact_conv_cases as ec
import motion_iou_cases
import motion_iou_twin
import multi_launch_cases as mc
import overlay_twin
import poison
import proposal_recall_twin
import sampling_lattice_cases as sc
import seq_nms_twin
import soft_nms_twin
import track_eval_twin
import tracks_twin
import vid_twin
from oracle import native

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
_NAME = {BF16: "bf16", F16: "f16", F32: "f32"}

# function of ops.py that calls _ws() -> the test below that runs it under every poison mode
WS_OPS = {
    "conv2d_nhwc": "test_gemm",
    "deconv4x4s2_into": "test_gemm",
    "conv2d_sp": "test_gemm",
    "nms": "test_nms",
    "rpn_select": "test_rpn_select",
    "postprocess": "test_postprocess",
    "postprocess_batched": "test_postprocess",
    "_merge_setup": "test_merge",                     # bbox_aug_merge and soft_merge
    "relation_attention_batched": "test_attention",
    "vid_eval_ap": "test_evaluation",
    "seq_nms": "test_evaluation",
    "link_tracks": "test_evaluation",
    "tubelet_match": "test_evaluation",
    "motion_iou": "test_evaluation",
    "overlay_detections": "test_evaluation",
}
# the modules whose own torch.empty / empty_like sites are poisoned by some case (the CPU completeness check reads their
# source for allocation idioms the proxy cannot see)
MODULE_NAMES = ("ops", "modeling", "relation", "fgfa", "rdn", "engine", "seq_nms", "tracks", "track_eval", "vid_eval",
                "motion_iou", "flat")


def _mods(*names):
    import importlib
    return tuple(importlib.import_module("mega.pytorch_amd." + n) for n in names)


def _ops():
    from mega.pytorch_amd import ops
    return ops


def _lib():
    from mega.pytorch_amd import _lib
    return _lib.load()


# ===================================================================================================== the harness
def _host(v):
    """a value of a case's result as something comparable on the host: tensors and arrays by their bytes"""
    ops = _ops()
    if isinstance(v, ops.Planes):
        v = v.t
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().contiguous().clone()
    if isinstance(v, np.ndarray):
        return np.ascontiguousarray(v).copy()
    if isinstance(v, (list, tuple)):
        return [_host(x) for x in v]
    if isinstance(v, dict):
        return {k: _host(x) for k, x in v.items()}
    return v


def _bytes(v):
    if isinstance(v, torch.Tensor):
        return v.reshape(-1).view(torch.uint8).numpy().tobytes() if v.numel() else b""
    return v.tobytes()


def _same(got, want, what):
    if isinstance(want, (torch.Tensor, np.ndarray)):
        assert type(got) is type(want) and tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, \
            "%s: %s %s vs %s %s" % (what, tuple(got.shape), got.dtype, tuple(want.shape), want.dtype)
        if _bytes(got) != _bytes(want):
            a = np.frombuffer(_bytes(got), np.uint8)
            b = np.frombuffer(_bytes(want), np.uint8)
            bad = np.nonzero(a != b)[0]
            isz = got.element_size() if isinstance(got, torch.Tensor) else got.itemsize
            raise AssertionError("%s: %d of %d bytes differ from the clean run, the first in element %d of %s" % (
                what, bad.size, a.size, int(bad[0]) // isz, tuple(got.shape)))
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, "%s[%d]" % (what, i))
    elif isinstance(want, dict):
        assert sorted(got) == sorted(want), what
        for k in want:
            _same(got[k], want[k], "%s[%r]" % (what, k))
    else:
        assert got == want, "%s: %r vs %r" % (what, got, want)


def _snap(case, which, dev):
    """-> (defined outputs, regions that must keep what they held), on the host"""
    out = case.run(which, dev)
    torch.cuda.synchronize()
    kept = out.pop("untouched", {}) if isinstance(out, dict) else {}
    return _host(out), _host(kept)


_CLEAN = {}


def _clean(case, dev):
    """assertion 1, once per case: two clean runs are bit-equal, and the clean run passes the reference check"""
    if case.name not in _CLEAN:
        a, _ = _snap(case, "B", dev)
        b, _ = _snap(case, "B", dev)
        _same(b, a, case.name + ": second clean run")
        if case.check is not None:
            case.check(a)
        _CLEAN[case.name] = a
    return _CLEAN[case.name]


def _stale(case, mode, dev):
    want = _clean(case, dev)
    modules = case.modules or _mods("ops")
    if mode != "replay":
        with poison.poisoned(mode, modules) as p:
            got, kept = _snap(case, "B", dev)
        assert p.count >= 1, "%s: no allocation went through the helper" % case.name
        _same(got, want, "%s under %s" % (case.name, mode))
        if case.check is not None:
            case.check(got)
        fill = {"zeros": 0, "ones": 255}[mode]
        for k, v in kept.items():
            raw = np.frombuffer(_bytes(v), np.uint8)
            assert raw.size and (raw == fill).all(), "%s under %s: %s was written (%d of %d bytes)" % (
                case.name, mode, k, int((raw != fill).sum()), raw.size)
        return
    # the slab: twice the larger of the two problems' allocations (a stale index of A, applied in B, stays inside) + 1 MiB
    need = 0
    for which in ("A", "B"):
        with poison.poisoned("zeros", modules) as p:
            _snap(case, which, dev)
        need = max(need, p.nbytes)
    with poison.poisoned("replay", modules, slab_bytes=2 * need + (1 << 20), device=dev) as p:
        _snap(case, "A", dev)
        p.reset()
        n0 = p.count
        got, _ = _snap(case, "B", dev)
        assert p.count - n0 >= 1, "%s: no allocation went through the helper" % case.name
        _same(got, want, "%s on the bytes of a larger problem" % case.name)
        if case.check is not None:
            case.check(got)
        p.reset()
        _snap(case, "Bp", dev)
        p.reset()
        got, _ = _snap(case, "B", dev)
        _same(got, want, "%s on the bytes of the same shapes with other values" % case.name)


def _case(name, run, check=None, modules=None):
    return SimpleNamespace(name=name, run=run, check=check, modules=modules)


def _family(builder):
    """builder() -> [case]; -> (names for parametrize: built on the host at collection, lookup by name)"""
    cached = functools.lru_cache(maxsize=None)(lambda: {c.name: c for c in builder()})
    return cached


def _alloc(shape, dtype, dev):
    """a caller's buffer, allocated the way the callers in the package do: through the (possibly poisoned) ops.torch"""
    return _ops().torch.empty(shape, dtype=dtype, device=dev)


MODES = poison.MODES


# ===================================================================================================== nms
NMS_N = (1, 64, 65, 200, 2100)          # one box; one mask word; two; mask + scan; above 2048: the lazy kernel


def _nms_cases():
    out = []
    for n in NMS_N:
        def run(which, dev, n=n):
            m, seed = {"B": (n, 0), "A": (3000, 0), "Bp": (n, 1)}[which]
            boxes, scores, _ = bc.chain(m, 20, seed)
            return {"keep": _ops().nms(torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), 0.5, strict_gt=True)}

        def check(o, n=n):
            boxes, scores, rank = bc.chain(n, 20)
            bc.check_keep(o["keep"].numpy(), bc.chain_keep(rank, bc.CHAIN_PERIOD[(20, 0.5)]), "nms chain n %d vs closed form" % n)
            bc.check_keep(o["keep"].numpy(), native.nms(boxes, scores, 0.5, True), "nms chain n %d vs oracle" % n)
        out.append(_case("nms-%d" % n, run, check))
    return out


_NMS = _family(_nms_cases)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", NMS_N)
def test_nms(dev, n, mode):
    """boxes 20 px apart on a line (thr 0.5: every second one is suppressed).  flags / mask words / the count live in the
    workspace and in `cnt`."""
    _stale(_NMS()["nms-%d" % n], mode, dev)


# ===================================================================================================== rpn_select
# mask + scan form: k = 600 < 4 * post; lazy form: all 12 x 12 x 9 = 1296 candidates, k >= 4 * post.  G = 12 boxes per lattice
# cell of which two survive: fewer than post are kept, so rows past the count exist in every frame (zero rows, index -1).
RPN_STALE = {
    "mask-k600": [bc.RpnSpec("stale-mask-a", 6, 9, 600, 300, 2, 12, ("ties", 0.75, 100, 60, "spread"), {"block0", "column", "clamp"}),
                  bc.RpnSpec("stale-mask-b", 6, 9, 600, 300, 2, 12, ("zeros", 150, 150, 300), {"block0", "column", "clamp"})],
    "lazy-1296": [bc.RpnSpec("stale-lazy-a", 12, 12, 1296, 300, 2, 12, ("ties", -0.5, 500, 500, "spread"), {"block0", "column", "clamp"}),
                  bc.RpnSpec("stale-lazy-b", 12, 12, 1296, 300, 2, 3, ("equal", 2.0), {"clamp"})],
}


@functools.lru_cache(maxsize=None)
def _rpn_frames(form, shift=0):
    """the two frames of a launch, each at the first seed that keeps its decisions off the boundaries (bc.rpn_case's rule)"""
    frames = []
    for i, spec in enumerate(RPN_STALE[form]):
        for seed in range(3000 + 50 * i + 17 * shift, 3000 + 50 * i + 17 * shift + 40):
            c = bc.RpnCase(spec, seed)
            if c.facts["side_margin"] >= bc.MARGIN and c.facts["iou_margin"] >= bc.MARGIN:
                frames.append(c)
                break
        else:
            raise AssertionError("%s: no seed meets the margins" % spec.name)
    return frames


def _rpn_launch(cases, dev):
    c = cases[0]
    rpn_out = torch.stack([k.rpn_out() for k in cases]).to(dev)
    props, scores, cnt, index = _ops().rpn_select(rpn_out, c.cell.to(dev), c.Hf, c.Wf, 16, c.pre, c.post, c.thr, c.min_size,
                                                  c.im_w, c.im_h, True, want_index=True)
    return {"props": props, "scores": scores, "count": cnt, "index": index}


def _rpn_cases():
    out = []
    for form in RPN_STALE:
        def run(which, dev, form=form):
            if which == "A":        # three frames of 12 x 18 x 9 = 2592 candidates, no cut
                return _rpn_launch([bc.rpn_case(n) for n in ("l-nocut-equal", "l-nocut-ties", "l-nocut-zeros")], dev)
            return _rpn_launch(_rpn_frames(form, 0 if which == "B" else 1), dev)

        def check(o, form=form):
            frames = _rpn_frames(form)
            assert any(int(o["count"][b]) < frames[b].post for b in range(len(frames))), "no frame stays below post_nms"
            for b, c in enumerate(frames):
                bc.check_rpn((o["props"][b], o["scores"][b], int(o["count"][b]), o["index"][b]), c.oracle(), "%s frame %d" % (form, b))
        out.append(_case("rpn-" + form, run, check))
    return out


_RPN = _family(_rpn_cases)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", sorted(RPN_STALE))
def test_rpn_select(dev, form, mode):
    """B = 2, want_index=True.  The whole of props / scores / index is defined: zero rows and index -1 past the count."""
    c = _RPN()["rpn-" + form]
    k, post = RPN_STALE[form][0].k, RPN_STALE[form][0].post
    assert (k >= 4 * post) == form.startswith("lazy")
    _stale(c, mode, dev)


# ===================================================================================================== postprocess*
POST_R, POST_NC, POST_NPROP, POST_MAX_DET = 70, 4, (70, 33), 80
POST_DEAD_CLASS = 3                    # no candidate of this class passes score_thresh


@functools.lru_cache(maxsize=None)
def _post_images(shift=0):
    """two images, R = 70, NC = 4, nprop 70 and 33: class 3 never passes the threshold; max_det = 80 lies below the first
    image's kept count (the radix select runs) and above the second's"""
    images = []
    for i, nprop in enumerate(POST_NPROP):
        spec = bc.PostSpec("stale-R70-n%d" % nprop, POST_R, POST_NC, nprop, POST_MAX_DET, "pairs", None, True)
        for seed in range(5000 + 50 * i + 17 * shift, 5000 + 50 * i + 17 * shift + 40):
            c = bc.PostCase(spec, seed)
            c.logits[:nprop, POST_DEAD_CLASS] = -30.0
            c.facts = c._facts()
            f = c.facts
            if f["iou_margin"] >= bc.MARGIN and f["thresh_margin"] >= 1e-8 and f["score_gap"] >= 1e-5:
                images.append(c)
                break
        else:
            raise AssertionError("%s: no seed meets the margins" % spec.name)
    return images


def _post_args(c):
    return (c.weights, c.im_w, c.im_h, c.score_thresh, c.nms, c.max_det, True)


def _post_rows(ob, os_, ol, oc):
    """the defined part: rows below the count"""
    counts = [int(v) for v in oc.reshape(-1).tolist()]
    if ob.dim() == 2:
        ob, os_, ol = ob[None], os_[None], ol[None]
    return {"count": counts, "rows": [(ob[b, :n], os_[b, :n], ol[b, :n]) for b, n in enumerate(counts)]}


def _post_batch(cases, dev):
    cat = [torch.cat([getattr(c, n) for c in cases]).to(dev).contiguous() for n in ("logits", "deltas", "props")]
    return cat, torch.tensor([c.nprop for c in cases], dtype=torch.int32, device=dev)


def _post_pick(which):
    if which == "A":
        return [bc.post_case(n) for n in ("R300-nc2", "R300-nc2-none", "R300-one")]
    return _post_images(0 if which == "B" else 1)


def _post_cases():
    def check_rows(o):
        imgs = _post_images()
        for b, c in enumerate(imgs):
            bx, s, l = o["rows"][b]
            bc.check_post((bx, s, l, o["count"][b]), c.reference(), "%s (image %d)" % (c.name, b))
            assert not bool((l == POST_DEAD_CLASS).any())
        D = [c.facts["D"] for c in imgs]
        assert D[0] > POST_MAX_DET > D[1] > 0, D

    def run_batched(which, dev):
        cases = _post_pick(which)
        (lg, dl, pr), nprop = _post_batch(cases, dev)
        return _post_rows(*_ops().postprocess_batched(lg, dl, pr, len(cases), *_post_args(cases[0]), nprop=nprop))

    def run_single(which, dev):
        rows = {"count": [], "rows": []}
        for c in _post_pick(which)[:2]:
            nprop = torch.tensor([c.nprop], dtype=torch.int32, device=dev)
            r = _post_rows(*_ops().postprocess(c.logits.to(dev), c.deltas.to(dev), c.props.to(dev), nprop, *_post_args(c)))
            rows["count"] += r["count"]
            rows["rows"] += [tuple(t.clone() for t in r["rows"][0])]
        return rows

    def run_candidates(which, dev):
        cases = _post_pick(which)
        (lg, dl, pr), nprop = _post_batch(cases, dev)
        c = cases[0]
        cb, cs = _ops().postprocess_candidates_batched(lg, dl, pr, len(cases), c.weights, c.im_w, c.im_h, c.score_thresh, nprop=nprop)
        live = cs >= 0
        # the scores are defined everywhere (-1 where there is no candidate), the boxes where there is one
        return {"scores": cs, "boxes": torch.where(live[..., None], cb, torch.zeros_like(cb))}

    def check_candidates(o):
        for b, c in enumerate(_post_images()):
            tb, ts = bt.candidates(c.logits, c.deltas, c.props, c.im_w, c.im_h, c.weights, c.score_thresh, nprop=c.nprop)
            live = ts >= 0
            np.testing.assert_array_equal(o["scores"][b].numpy() >= 0, live)
            assert not live[POST_DEAD_CLASS - 1].any() and not live[:, c.nprop:].any() and live.any()
            np.testing.assert_allclose(o["scores"][b].numpy(), ts, rtol=0, atol=1e-6)
            np.testing.assert_allclose(o["boxes"][b].numpy()[live], tb[live], rtol=0, atol=1e-3)

    return [_case("postprocess", run_single, check_rows), _case("postprocess_batched", run_batched, check_rows),
            _case("postprocess_candidates_batched", run_candidates, check_candidates)]


_POST = _family(_post_cases)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("op", ["postprocess", "postprocess_batched", "postprocess_candidates_batched"])
def test_postprocess(dev, op, mode):
    """B = 2, R = 70, NC = 4, nprop = [70, 33], one class without a candidate, max_det between the two images' kept counts.
    Defined: the rows below each count (postprocess*), every score and the boxes of the live candidates (candidates)."""
    _stale(_POST()[op], mode, dev)


# ===================================================================================================== bbox_aug_merge, soft_merge
MERGE_SIZES, MERGE_FLIPS = [(160, 96), (203, 117)], [False, True]
MERGE_KW = {"bbox_aug_merge": None, "soft-none": {}, "soft-linear": {"soft_method": "linear"},
            "soft-gaussian": {"soft_method": "gaussian", "sigma": 0.5},
            "soft-linear-vote": {"soft_method": "linear", "vote_on": True, "vote_thresh": 0.8, "vote_scoring": "AVG"}}
_SOFT_KW = {"soft_method": "soft_method", "sigma": "sigma", "vote_on": "vote", "vote_thresh": "vote_thresh", "vote_scoring": "vote_scoring"}


@functools.lru_cache(maxsize=None)
def _merge_frames(which):
    """K = 2 views, F = 2 frames, R = 40 rows, NC = 3 (B, B'); A: K = 3, F = 3, R = 100, NC = 5"""
    if which == "A":
        sizes, flips = MERGE_SIZES + [(203, 117)], MERGE_FLIPS + [False]
        return [bt.random_views(40 + f, 3, 100, C1=4, sizes=sizes, grid=25)[0] for f in range(3)], sizes, flips
    seed = 20 if which == "B" else 30
    return [bt.random_views(seed + f, 2, 40, C1=2, sizes=MERGE_SIZES, grid=25)[0] for f in range(2)], MERGE_SIZES, MERGE_FLIPS


def _merge_cases():
    out = []
    for name, kw in MERGE_KW.items():
        def run(which, dev, kw=kw):
            frames, sizes, flips = _merge_frames(which)
            K = len(sizes)
            cb = torch.from_numpy(np.stack([np.stack([fr[k][0] for fr in frames]) for k in range(K)])).to(dev).contiguous()
            cs = torch.from_numpy(np.stack([np.stack([fr[k][1] for fr in frames]) for k in range(K)])).to(dev).contiguous()
            if kw is None:
                return _post_rows(*_ops().bbox_aug_merge(cb, cs, sizes, flips, 0.001, 0.5, 30, True))
            return _post_rows(*_ops().soft_merge(cb, cs, sizes, flips, 0.001, 0.5, 30, True, **{_SOFT_KW[k]: v for k, v in kw.items()}))

        def check(o, kw=kw, name=name):
            frames, sizes, flips = _merge_frames("B")
            assert sum(o["count"]) > 0
            for f, fr in enumerate(frames):
                if kw is None:
                    wb, ws, wl = bt.merge(fr, sizes, flips, max_det=30, strict_gt=True)
                else:
                    wb, ws, wl = soft_nms_twin.merge(fr, sizes, flips, max_det=30, strict_gt=True, **kw)
                gb, gs, gl = (t.numpy() for t in o["rows"][f])
                assert o["count"][f] == len(ws), "%s frame %d: %d rows, twin %d" % (name, f, o["count"][f], len(ws))
                np.testing.assert_array_equal(gl, wl)
                if kw and kw.get("soft_method") == "gaussian":      # expf: test_soft_nms_gpu's tolerance
                    np.testing.assert_array_equal(gb.view(np.uint32), np.asarray(wb, np.float32).view(np.uint32))
                    np.testing.assert_allclose(gs, ws, rtol=1e-4, atol=0)
                elif kw and kw.get("vote_on"):                     # f64 sums, one rounding: test_soft_nms_gpu's tolerances
                    np.testing.assert_allclose(gb, wb, rtol=0, atol=1e-3)
                    np.testing.assert_allclose(gs, ws, rtol=1e-6, atol=0)
                else:
                    np.testing.assert_array_equal(gs.view(np.uint32), np.asarray(ws, np.float32).view(np.uint32))
                    np.testing.assert_array_equal(gb.view(np.uint32), np.asarray(wb, np.float32).view(np.uint32))
        out.append(_case(name, run, check))
    return out


_MERGE = _family(_merge_cases)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("op", sorted(MERGE_KW))
def test_merge(dev, op, mode):
    """K = 2 views, F = 2, R = 40, NC = 3, max_det 30; every soft method and box voting.  Defined: rows below the count."""
    _stale(_MERGE()[op], mode, dev)


# ===================================================================================================== the GEMM family
LIB_SPLITK = (1, 2, 3, 32768 + 1024, 72, 1, 1, 0, 1)      # M = 6 rows, K past the library's own split-K threshold
LINEAR_ROWS3 = (3, 1, 1, 32768 + 1024, 72, 1, 1, 0, 1)
SP_SPLITK = (1, 2, 2, 11264, 72, 1, 1, 0, 1)               # x3 operands: K = 3 * 11264 >= 32768
SP_LINEAR3 = (3, 1, 1, 11264, 72, 1, 1, 0, 1)
GEMM_A = (2, 9, 11, 512, 264, 3, 1, 1, 1)                  # the larger problem run first under replay (split 8 ways: 1.7 MB of partials)
RS_SHAPE = (2, 5, 7, 128, 256, 1, 1, 0, 1)                 # _conv1x1_strided_residual (Cout % 256 == 0): the output's size; the residual is 9 x 13
DECONV = (1, 4, 6, 386, 64, 128)
LT = (37, 128, 72, 64)                                     # linear_transposed: M rows, K, Nout, ld


def _seeded(shape, dtype, odt, relu, use_res, which):
    if which == "B":
        return ec.conv_case(shape, dtype, odt, relu, use_res)
    return ec.make_case(shape, dtype, odt, relu, use_res, seed=sum(shape) % 1009 + 1)


def _gemm_a(dev):
    """the larger problem: a caller split-K conv whose partial sums cover what any B case allocates"""
    c = ec.conv_case(GEMM_A, BF16, F32, 1, False)
    _ops().conv2d_nhwc(c.x.to(dev), c.w.to(dev), c.scale.to(dev), c.bias.to(dev), None, pad=1, relu=1, out_dtype=F32, ksplit=8)
    x = torch.ones((4, 1, 1, 32768 + 1024), dtype=BF16, device=dev)
    w = torch.ones((136, 1, 1, 32768 + 1024), dtype=BF16, device=dev)
    return {"y": _ops().conv2d_nhwc(x, w)}


def _conv_run(shape, dtype, odt, relu, use_res, **kw):
    def run(which, dev):
        if which == "A":
            return _gemm_a(dev)
        c = _seeded(shape, dtype, odt, relu, use_res, which)
        N, H, W, Cin, Cout, R, stride, pad, dil = shape
        return {"y": _ops().conv2d_nhwc(c.x.to(dev), c.w.to(dev), c.scale.to(dev), c.bias.to(dev),
                                        None if c.res is None else c.res.to(dev), stride=stride, pad=pad, dil=dil, relu=relu,
                                        out_dtype=odt, **kw)}

    def check(o):
        c = ec.conv_case(shape, dtype, odt, relu, use_res)
        ec.assert_bits_equal(o["y"], ec.reference(c)[0], "conv %s %s->%s %s" % (shape, dtype, odt, kw), relu=relu)
    return run, check


def _gemm_cases():
    ops = _ops()
    out = []
    lib = _lib()
    # ---- conv2d_nhwc: the library's own split-K (f32, 16-bit and f32-from-16-bit outputs), M = 6
    M, K, Cout = 6, LIB_SPLITK[3], LIB_SPLITK[4]
    assert lib.mega_conv2d_nhwc_workspace_bytes(M, Cout, K) > 0 and lib.mega_conv2d_nhwc_workspace_bytes(M, Cout, 4096) == 0
    for dt, odt in ((F32, F32), (BF16, BF16), (F16, F16), (BF16, F32)):
        out.append(_case("conv-lib-splitk-%s-%s" % (_NAME[dt], _NAME[odt]), *_conv_run(LIB_SPLITK, dt, odt, 1, False)))
    # ---- caller split-K: 4 ranges, and a count far past the K-tile count (clamped); LeakyReLU + residual in the finalize
    for dt, odt in ((F32, F32), (BF16, BF16), (BF16, F32)):
        for ks in (4, 1000):
            Mc, Kc = 2 * 6 * 8, 9 * ec.CALLER_SPLITK_SHAPE[3]
            ranges = lib.mega_conv2d_nhwc_ks_workspace_bytes(Mc, 128, Kc, ops._DT[dt], ks) // (Mc * 128 * 4)
            assert ranges == (4 if ks == 4 else Kc // (32 if dt == F32 else 64)), (dt, ks, ranges)
            out.append(_case("conv-ksplit%d-%s-%s" % (ks, _NAME[dt], _NAME[odt]),
                             *_conv_run(ec.CALLER_SPLITK_SHAPE, dt, odt, 2, True, ksplit=ks)))
    # ---- linear: split-K on 3 rows
    assert lib.mega_conv2d_nhwc_workspace_bytes(3, 72, LINEAR_ROWS3[3]) > 0
    for dt in (F32, BF16):
        def run(which, dev, dt=dt):
            if which == "A":
                return _gemm_a(dev)
            c = _seeded(LINEAR_ROWS3, dt, dt, 1, False, which)
            Kl = LINEAR_ROWS3[3]
            return {"y": ops.linear(c.x.view(3, Kl).to(dev), c.w.view(72, Kl).to(dev), c.bias.to(dev), relu=True, scale=c.scale.to(dev))}

        def check(o, dt=dt):
            c = ec.conv_case(LINEAR_ROWS3, dt, dt, 1, False)
            ec.assert_bits_equal(o["y"].view(3, 1, 1, 72), ec.reference(c)[0], "linear split-K, 3 rows, %s" % dt, relu=1)
        out.append(_case("linear-splitk-3rows-" + _NAME[dt], run, check))
    # ---- conv2d_sp / linear_sp with split-K (x3 operands, f32 output, no residual: the path that takes a workspace)
    for name, shape in (("conv2d_sp-splitk", SP_SPLITK), ("linear_sp-splitk", SP_LINEAR3)):
        N, H, W, Cs, Co = shape[:5]
        assert lib.mega_conv2d_nhwc_workspace_bytes(N * H * W, Co, 3 * Cs) > 0

        def run(which, dev, shape=shape, name=name):
            if which == "A":
                return _gemm_a(dev)
            c = ec.make_sp_case(shape, False, 1, False, seed=sum(shape) + (0 if which == "B" else 1))
            xp = ops.split_planes(c.x.to(dev))
            w3 = ops.split_conv_weight_x3(c.w).to(dev)
            if name.startswith("linear"):
                M_, C_ = shape[0], shape[3]
                y = ops.linear_sp(ops.Planes(xp.t.view(M_, 2 * C_), C_), w3.view(shape[4], 3 * C_), c.bias.to(dev), relu=True)
                return {"planes": xp, "y": y.view(M_, 1, 1, shape[4])}
            return {"planes": xp, "y": ops.conv2d_sp(xp, w3, c.scale.to(dev), c.bias.to(dev), relu=1, out_mode="f32", operands="x3")}

        def check(o, shape=shape, name=name):
            c = ec.make_sp_case(shape, False, 1, False, seed=sum(shape))
            if name.startswith("linear"):
                c.scale = torch.ones_like(c.scale)
            ec.assert_bits_equal(o["planes"], torch.cat(ec.split_hi_lo(c.x), dim=-1), "split_planes %s" % (shape,))
            ec.assert_bits_equal(o["y"], ec.reference_sp(c, "f32")[0], "%s %s" % (name, shape), relu=1)
        out.append(_case(name, run, check))

    # ---- the 1x1 conv with its residual read at pixel stride 2 (no workspace: the output is the allocation)
    def rs_case(which):
        c = _seeded(RS_SHAPE, BF16, BF16, 1, False, which)
        g = torch.Generator().manual_seed(3 if which == "B" else 4)
        full = torch.randint(-8, 9, (2, 9, 13, RS_SHAPE[4]), generator=g).to(BF16)
        return c, full

    def run_rs(which, dev):
        if which == "A":
            return _gemm_a(dev)
        c, full = rs_case(which)
        return {"y": ops.conv2d_nhwc(c.x.to(dev), c.w.to(dev), c.scale.to(dev), c.bias.to(dev), residual=full.to(dev), relu=True,
                                     residual_stride=2)}

    def check_rs(o):
        c, full = rs_case("B")
        c = SimpleNamespace(**dict(vars(c), res=full[:, ::2, ::2].contiguous()))
        ec.assert_bits_equal(o["y"], ec.reference(c)[0], "conv1x1 strided residual", relu=1)
    out.append(_case("conv1x1-strided-residual", run_rs, check_rs))

    # ---- deconv4x4s2_into a wider buffer, ksplit 1 and 4: the slice is right, the columns round it keep what they held
    for dt in (F32, BF16):
        for ks in (1, 4):
            mult = 32 if dt == F32 else 64
            N, H, W, Cin, C, Cs = DECONV
            ldo = (Cs + C + 2 + mult - 1) // mult * mult
            H2, W2 = 2 * H + 1, 2 * W

            def run(which, dev, dt=dt, ks=ks, mult=mult, ldo=ldo):
                if which == "A":
                    return _gemm_a(dev)
                c = ec.deconv_case(DECONV, dt) if which == "B" else ec.make_deconv_case(N, H, W, Cin, C, dt, seed=7)
                cp = (Cin + mult - 1) // mult * mult
                xp = torch.zeros((N, H, W, cp), dtype=dt)
                xp[..., :Cin] = c.x
                w4 = ops.pack_deconv4x4s2(c.wt, dt, mult)
                buf = _alloc((N, H2, W2, ldo), dt, dev)
                ops.deconv4x4s2_into(xp.to(dev), w4.to(dev), c.bias.repeat(4).to(dev), buf, Cs, relu=2, ksplit=ks)
                return {"slice": buf[..., Cs:Cs + C], "untouched": {"below the slice": buf[..., :Cs], "above the slice": buf[..., Cs + C:]}}

            def check(o, dt=dt, ks=ks):
                want, _ = ec.reference_deconv(ec.deconv_case(DECONV, dt), 2, H2, W2)
                ec.assert_bits_equal(o["slice"], want, "deconv %s %s ksplit %d" % (DECONV, dt, ks), relu=2)
            out.append(_case("deconv-into-%s-ksplit%d" % (_NAME[dt], ks), run, check))

    # ---- linear_transposed (residual; X3Weight): [Nout, ld] with the pad columns zero.  Integer operands: exact
    def lt_inputs(which):
        M_, K_, N_, ld = LT
        g = torch.Generator().manual_seed(5 if which == "B" else 6)
        w = torch.randint(-4, 5, (N_, K_), generator=g).float()
        x = torch.randint(-8, 9, (M_, K_), generator=g).float()
        r = torch.randint(-8, 9, (N_, ld), generator=g).float()
        return w, x, r

    def run_lt(which, dev):
        if which == "A":
            return _gemm_a(dev)
        w, x, r = lt_inputs(which)
        return {"y": ops.linear_transposed(w.to(BF16).to(dev), x.to(BF16).to(dev), LT[3], residual=r.to(BF16).to(dev))}

    def check_lt(o):
        w, x, r = lt_inputs("B")
        M_ = LT[0]
        want = ec.convert((w.double() @ x.double().t()) + r.double()[:, :M_], BF16)
        ec.assert_bits_equal(o["y"][:, :M_].contiguous(), want, "linear_transposed + residual")
        assert not bool(o["y"][:, M_:].float().abs().any()) and not bool(torch.isnan(o["y"].float()).any()), "pad columns not zero"
    out.append(_case("linear_transposed-residual", run_lt, check_lt))

    def run_lt3(which, dev):
        if which == "A":
            return _gemm_a(dev)
        w, x, _ = lt_inputs(which)
        xw = ops.X3Weight(w, dev)
        return {"yt": ops.linear_transposed(xw, x.to(dev), LT[3]), "y": ops.linear(x.to(dev), xw)}

    def check_lt3(o):
        w, x, _ = lt_inputs("B")
        M_ = LT[0]
        want = (w.double() @ x.double().t()).float()
        ec.assert_bits_equal(o["yt"][:, :M_].contiguous(), want, "linear_transposed, X3Weight")
        assert bool((o["yt"][:, M_:] == 0).all()), "pad columns not zero"
        ec.assert_bits_equal(o["y"], want.t().contiguous(), "linear, X3Weight")
    out.append(_case("linear_transposed-x3", run_lt3, check_lt3))
    return out


_GEMM = _family(_gemm_cases)
GEMM_NAMES = (["conv-lib-splitk-%s-%s" % p for p in (("f32", "f32"), ("bf16", "bf16"), ("f16", "f16"), ("bf16", "f32"))] +
              ["conv-ksplit%d-%s-%s" % ((ks,) + p) for p in (("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32")) for ks in (4, 1000)] +
              ["linear-splitk-3rows-f32", "linear-splitk-3rows-bf16", "conv2d_sp-splitk", "linear_sp-splitk",
               "conv1x1-strided-residual"] +
              ["deconv-into-%s-ksplit%d" % (d, k) for d in ("f32", "bf16") for k in (1, 4)] +
              ["linear_transposed-residual", "linear_transposed-x3"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", GEMM_NAMES)
def test_gemm(dev, name, mode, monkeypatch):
    """conv2d_nhwc (library and caller split-K), linear, conv2d_sp, linear_sp, _conv1x1_strided_residual, deconv4x4s2_into,
    linear_transposed: integer operands, bit for bit against float64 (tests/exact_conv_cases.py).  The split-K partial sums
    are the workspace; every threshold is asked from the library (mega_conv2d_nhwc_*workspace_bytes)."""
    monkeypatch.delenv("MEGA_IGEMM_TILE", raising=False)
    cases = _GEMM()
    assert sorted(cases) == sorted(GEMM_NAMES)
    _stale(cases[name], mode, dev)


# ===================================================================================================== attention
ATTN_SHAPES = [(40, 1500), (33, 97), (40, 700, 800)]       # three key-range splits; one; two key segments
ATTN_A = [(300, 750), (129, 64), (257, 33), (40, 1800)]


def _untile_pos(t, Nk):
    """16-bit [16, KT, Nq, 32] in the attention kernel's tile order -> f32 [16, Nq, Nk]: the slots of the keys below Nk"""
    G, KT, Nq, _ = t.shape
    x = t.float().view(G, KT, Nq, 2, 4, 4).permute(0, 2, 1, 4, 3, 5)
    return x.reshape(G, Nq, KT * 32)[:, :, :Nk].contiguous()


def _attn_dev_item(it, dev, pos):
    d = {"q": it["q"].to(dev), "Nk": it["Nk"], "resid": it["resid"].to(dev), "bias_v": it["bias_v"].to(dev), "pos": pos}
    if it["N2"]:
        N1, N2, a, b = it["N1"], it["N2"], it["a_cols"], it["b_cols"]
        big1, big2, kb1, kb2 = (it[n].to(dev) for n in ("big1", "big2", "kb1", "kb2"))
        d.update(k=kb1[2:2 + N1], vt=big1[:, a:a + N1], N1=N1, k2=kb2[1:1 + N2], vt2=big2[:, b:b + N2])
    else:
        d.update(k=it["k"].to(dev), vt=it["vt"].to(dev))
    return d


def _attn_chain(shapes, seed0, dev, dtype):
    """tile-ordered position logits -> the batched attention that reads them (pad-key slots included), one poison for both"""
    ops = _ops()
    wg, bg, dm = (t.to(dev) for t in mc.attn_pos_weights())
    its = [mc.attn_item(s, dtype, seed=seed0 + i) for i, s in enumerate(shapes)]
    if dtype == F32:
        pos = [ops.position_logits(it["rq"].to(dev), it["rk"].to(dev), wg, bg, dm, precise=True) for it in its]
        defined = [p[:, :, :it["Nk"]] for p, it in zip(pos, its)]
    else:
        pos = ops.position_logits_batched([it["rq"].to(dev) for it in its], [it["rk"].to(dev) for it in its], wg, bg, dm,
                                          precise=False, tiled=dtype)
        defined = [_untile_pos(p, it["Nk"]) for p, it in zip(pos, its)]
    outs = ops.relation_attention_batched([_attn_dev_item(it, dev, p) for it, p in zip(its, pos)])
    return {"pos": defined, "out": list(outs)}


_pos_weights = functools.lru_cache(maxsize=None)(mc.pos_weights)      # (builds a seeded state dict: once)


def _attn_cases():
    out = []
    for dt in (BF16, F32):
        def run(which, dev, dt=dt):
            if which == "A":
                return _attn_chain(ATTN_A, 50, dev, dt)
            return _attn_chain(ATTN_SHAPES, 0 if which == "B" else 20, dev, dt)

        def check(o, dt=dt):
            for i, shape in enumerate(ATTN_SHAPES):
                it = mc.attn_item(shape, dt, seed=i)
                ref = mc.relation_attention_f64(it["q"], it["k"], it["vt"], it["Nk"], pos=o["pos"][i], resid=it["resid"],
                                                bias_v=it["bias_v"])
                got = o["out"][i]
                err = ((got.double() - ref).abs().max() / (ref.abs().max() + 1e-12)).item()
                assert torch.isfinite(got.float()).all() and torch.isfinite(o["pos"][i]).all(), (shape, dt)
                assert err < mc.ATTN_BOUND[dt], (shape, dt, err)
        out.append(_case("attention-chain-" + _NAME[dt], run, check))

    # the position logits alone against float64 (mc.pos_problem's boxes, the bounds of test_position_logits)
    def run_pos(which, dev):
        Nq, Nk = (300, 750) if which == "A" else (37, 70)
        bq, bk = mc.pos_problem(Nq, Nk) if which != "Bp" else tuple(t + 3.0 for t in mc.pos_problem(Nq, Nk))
        wg_t, bg, dm = (t.to(dev) for t in _pos_weights())
        ops = _ops()
        rows = ops.position_logits(bq.to(dev), bk.to(dev), wg_t, bg, dm, precise=True)
        fast = ops.position_logits(bq.to(dev), bk.to(dev), wg_t, bg, dm, precise=False)
        tiled = ops.position_logits(bq.to(dev), bk.to(dev), wg_t, bg, dm, precise=False, tiled=BF16)
        assert rows.shape[2] == (Nk + 31) // 32 * 32 and tuple(tiled.shape) == (16, (Nk + 31) // 32, Nq, 32)
        return {"rows": rows[:, :, :Nk], "fast": fast[:, :, :Nk], "tiled": _untile_pos(tiled, Nk)}

    def check_pos(o):
        from oracle import mega_oracle as mo
        bq, bk = mc.pos_problem(37, 70)
        wg_t, bg, _ = _pos_weights()
        # precise rows: the f32 formula (test_position_logits' reference and bound; f32 itself is up to 5e-4 from float64 here)
        ref32 = (F.relu(F.conv2d(mo.cal_position_embedding(bq, bk), wg_t.t().contiguous().view(16, 64, 1, 1), bg)) + 1e-6).log()[0]
        assert (o["rows"].exp() - ref32.exp()).abs().max() < 2e-5
        ref = mc.position_logits_f64(bq, bk, wg_t, bg).exp()
        for k in ("fast", "tiled"):
            err = (o[k].double().exp() - ref).abs()
            assert torch.isfinite(o[k]).all() and err.max() < 6e-3 and err.mean() < 1e-3, (k, err.max(), err.mean())
    out.append(_case("position_logits", run_pos, check_pos))
    return out


_ATTN = _family(_attn_cases)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["attention-chain-bf16", "attention-chain-f32", "position_logits"])
def test_attention(dev, name, mode):
    """position_logits feeding relation_attention_batched under the same poison: three ragged problems (three key-range
    splits, one, two key segments; Nq no multiple of 64, Nk no multiple of 32).  The logits' pad-key slots are never written
    and ARE the attention's input: under `ones` they are NaN, and the attention's output must not see them.  Defined:
    the logits of the keys below Nk, every output row."""
    lib = _lib()
    assert [lib.mega_relation_attention_splits(s[0], sum(s[1:]), 16) for s in ATTN_SHAPES] == [3, 1, 3]
    assert lib.mega_relation_attention_workspace_bytes(40, 1500, 16) > 0 and lib.mega_relation_attention_workspace_bytes(33, 97, 16) == 0
    _stale(_ATTN()[name], mode, dev)


# ===================================================================================================== FGFA / FlowNetS
FGFA_GEOM = (9, 5, 6, 7, 16, 8)             # S, T, H, W, Cf, Ce
FGFA_GEOM_A = (25, 21, 12, 17, 64, 128)
FGFA_W_BOUND = {F32: 2e-5, BF16: 2e-3}      # test_fgfa_warp_aggregate's bounds
FGFA_O_BOUND = {F32: 1e-5, BF16: 1e-2}
LEVEL = (2, 4, 6, 386, 64, 9, 12, 128)      # N, H, W, Cin, C, H2, W2, Cs: an odd x even target (one row / column cropped)


def _relerr(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _fgfa_inputs(which, dtype):
    geom = FGFA_GEOM_A if which == "A" else FGFA_GEOM
    ring, flow = mc.fgfa_ring(geom, dtype, seed=1 if which == "Bp" else 0)
    return geom, ring, flow


def _flow_cases():
    ops = _ops()
    out = []
    for dt in (F32, BF16):
        def run(which, dev, dt=dt):
            (S, T, H, W, Cf, Ce), ring, flow = _fgfa_inputs(which, dt)
            slots = mc.wrapped_slots(S, T)
            key_pos = T // 2
            idx = torch.tensor(slots)
            feats, fl = ring[idx].contiguous().to(dev), flow[idx].contiguous().to(dev)
            a, aw = ops.fgfa_warp_aggregate(feats, fl, Cf, key_pos, want_weights=True)
            order = mc.orders_tensor(mc.order_row(slots, key_pos)).to(dev)
            b, bw = ops.fgfa_warp_aggregate(ring.to(dev), fl, Cf, 0, want_weights=True, order=order, flow_pos=key_pos)
            rows = mc.group_slots(S, T, 2)
            orders = mc.orders_tensor([mc.order_row(r, key_pos) for r in rows]).to(dev)
            flows = mc.fgfa_flow(torch.Generator().manual_seed(2 + (which == "Bp")), 2 * T, H, W).to(dev)
            g = ops.fgfa_warp_aggregate_group(ring.to(dev), flows, Cf, orders, key_pos)
            singles = [ops.fgfa_warp_aggregate(ring.to(dev), flows[i * T:(i + 1) * T], Cf, 0, order=orders[i], flow_pos=key_pos)
                       for i in range(2)]
            return {"out": a, "weights": aw, "ring": b, "ring_weights": bw, "group": g, "singles": singles}

        def check(o, dt=dt):
            (S, T, H, W, Cf, Ce), ring, flow = _fgfa_inputs("B", dt)
            slots = mc.wrapped_slots(S, T)
            ref, ref_w = mc.fgfa_aggregate_f64(ring, flow[torch.tensor(slots)], slots, T // 2, Cf)
            werr, err = (o["weights"].double() - ref_w).abs().max().item(), _relerr(o["out"], ref)
            assert werr < FGFA_W_BOUND[dt] and err < FGFA_O_BOUND[dt], (dt, werr, err)
            assert torch.equal(o["ring"], o["out"]) and torch.equal(o["ring_weights"], o["weights"])
            for i in range(2):
                assert torch.equal(o["group"][i], o["singles"][i]) and torch.isfinite(o["group"][i].float()).all()
        out.append(_case("fgfa_warp_aggregate-" + _NAME[dt], run, check))

    # ---- fgfa_pair_taps: the three zero rows above and below are part of the output
    def taps_inputs(which):
        T, H, W = (7, 60, 100) if which == "A" else (3, 37, 51)
        g = torch.Generator().manual_seed(T + H + W + (which == "Bp"))
        return torch.rand((T, 3, H, W), generator=g) * 255.0 - 110.0, torch.rand((1, 3, H, W), generator=g) * 255.0 - 110.0

    def run_taps(which, dev):
        refs, cur = taps_inputs(which)
        return {"taps": ops.fgfa_pair_taps(refs.to(dev), cur.to(dev), None, BF16)}

    def check_taps(o):
        refs, cur = taps_inputs("B")
        want = cpu_ops.fgfa_pair_taps(refs, cur, None, BF16)
        assert torch.equal(o["taps"].view(torch.int16), want.view(torch.int16))
        assert not bool(o["taps"][:, :3].float().abs().any()) and not bool(o["taps"][:, -3:].float().abs().any())
    out.append(_case("fgfa_pair_taps", run_taps, check_taps))

    # ---- flow_conv1_combine (group tables) and flow_pred_finish
    def conv1_inputs(which):
        S, h, w = (9, 11, 13) if which == "A" else (6, 5, 7)
        ab, bias = mc.conv1_inputs(S, h, w, seed=1 if which == "Bp" else 0)
        return S, ab, bias, mc.conv1_group_orders(S, 2, S - 2)

    def run_conv1(which, dev):
        S, ab, bias, rows = conv1_inputs(which)
        return {"y": ops.flow_conv1_combine(ab.to(dev), bias.to(dev), BF16, order=mc.orders_tensor(rows).to(dev), nwin=S - 2)}

    def check_conv1(o):
        S, ab, bias, rows = conv1_inputs("B")
        want = cpu_ops.flow_conv1_combine(ab, bias, BF16, order=mc.orders_tensor(rows), nwin=S - 2)
        assert torch.equal(o["y"].view(torch.int16), want.view(torch.int16))
    out.append(_case("flow_conv1_combine", run_conv1, check_conv1))

    for dt in (F32, BF16):
        def run_pred(which, dev, dt=dt):
            shape = (3, 7, 9, 64) if which == "A" else (2, 3, 5, 18)
            z, bias = mc.pred_inputs(*shape, seed=1 if which == "Bp" else 0)
            return {"flow": ops.flow_pred_finish(z.to(dev), bias.to(dev), 2.5, dt)}

        def check_pred(o, dt=dt):
            z, bias = mc.pred_inputs(2, 3, 5, 18)
            ref, mag = mc.flow_pred_finish_f64(z, bias, 2.5)
            bound = 10 * 2.0 ** -24 * mag + mc.half_ulp(ref, dt)
            assert ((o["flow"].double() - ref).abs() <= bound).all()
        out.append(_case("flow_pred_finish-" + _NAME[dt], run_pred, check_pred))

    # ---- dff_warp_scale on the exact lattice
    for dt in (F32, BF16):
        def dff_inputs(which, dt=dt):
            Hm, Wm = (17, 33) if which == "A" else (5, 9)
            seed = Hm + (which == "Bp")
            return (sc.int_features(1, Hm, Wm, 64, seed=seed)[0].to(dt), sc.warp_lattice(Hm, Wm)[0].contiguous(),
                    sc.pow2_scale(Hm, Wm, 64, seed=seed).to(dt))

        def run_dff(which, dev, dff_inputs=dff_inputs):
            feats, flow, scale = dff_inputs(which)
            return {"y": ops.dff_warp_scale(feats.to(dev), flow.to(dev), scale.to(dev))}

        def check_dff(o, dff_inputs=dff_inputs):
            feats, flow, scale = dff_inputs("B")
            sc.assert_bits(o["y"], cpu_ops.dff_warp_scale(feats, flow, scale), "dff_warp_scale")
        out.append(_case("dff_warp_scale-" + _NAME[dt], run_dff, check_dff))

    # ---- one refinement level as FlowNetS._trunk.level builds it: deconv into the torch.empty concatenation buffer, the
    #      assemble kernel for the rest (zero pad channels included), then the 18-column prediction conv that reads ALL channels
    for dt in (F32, BF16):
        mult = 32 if dt == F32 else 64

        def level_inputs(which, dt=dt, mult=mult):
            N, H, W, Cin, C, H2, W2, Cs = LEVEL if which != "A" else (3, 7, 9, 770, 128, 13, 17, 256)
            g = torch.Generator().manual_seed(N + Cin + (which == "Bp"))
            d = SimpleNamespace(N=N, H=H, W=W, Cin=Cin, C=C, H2=H2, W2=W2, Cs=Cs)
            d.x = torch.randint(-8, 9, (N, H, W, Cin), generator=g).to(dt)
            d.wt = torch.randint(-4, 5, (Cin, C, 4, 4), generator=g).float()
            d.b = torch.randint(-16, 17, (C,), generator=g).float()
            d.skip = torch.randint(-8, 9, (N, H2, W2, Cs), generator=g).to(dt)
            d.flow = torch.randint(-4, 5, (N, H, W, 2), generator=g).to(dt)
            d.wu = torch.randint(-2, 3, (2, 2, 4, 4), generator=g).float()
            d.bu = torch.randint(-4, 5, (2,), generator=g).float()
            d.ldo = (Cs + C + 2 + mult - 1) // mult * mult
            w18 = torch.zeros((32 if dt == F32 else 64, 1, 1, d.ldo))           # (Cout padded; the pad channels' weights are zero)
            w18[:18, 0, 0, :Cs + C + 2] = torch.randint(-1, 2, (18, Cs + C + 2), generator=g).float()
            d.w18 = w18.to(dt)
            return d

        def run_level(which, dev, dt=dt, mult=mult, level_inputs=level_inputs):
            d = level_inputs(which)
            cp = (d.Cin + mult - 1) // mult * mult
            xp = torch.zeros((d.N, d.H, d.W, cp), dtype=dt)
            xp[..., :d.Cin] = d.x
            w4 = ops.pack_deconv4x4s2(d.wt, dt, mult)
            cc = _alloc((d.N, d.H2, d.W2, d.ldo), dt, dev)
            ops.deconv4x4s2_into(xp.to(dev), w4.to(dev), d.b.repeat(4).to(dev), cc, d.Cs, relu=2)
            cc = ops.flow_level_assemble(d.skip.to(dev), d.flow.to(dev), d.wu.to(dev), d.bu.to(dev), cc, d.C)
            z = ops.conv2d_nhwc(cc, d.w18.to(dev), None, None, out_dtype=F32)
            return {"cc": cc, "z": z[..., :18]}

        def check_level(o, dt=dt, level_inputs=level_inputs):
            d = level_inputs("B")
            crop = 0 if (2 * d.H + 2, 2 * d.W + 2) == (d.H2, d.W2) else 1
            case = SimpleNamespace(dtype=dt, x=d.x, wt=d.wt, bias=d.b)
            dec, _ = ec.reference_deconv(case, 2, d.H2, d.W2)
            up = F.conv_transpose2d(d.flow.double().permute(0, 3, 1, 2), d.wu.double(), d.bu.double(), stride=2)
            up = up[:, :, crop:crop + d.H2, crop:crop + d.W2].permute(0, 2, 3, 1).contiguous()
            want = torch.zeros((d.N, d.H2, d.W2, d.ldo), dtype=torch.float64)
            want[..., :d.Cs], want[..., d.Cs:d.Cs + d.C], want[..., d.Cs + d.C:d.Cs + d.C + 2] = d.skip.double(), dec.double(), up
            want = ec.convert(want, dt)
            ec.assert_bits_equal(o["cc"], want, "FlowNetS level concatenation %s" % dt)
            assert not bool(o["cc"][..., d.Cs + d.C + 2:].float().abs().any()), "pad channels not zero"
            # the conv over ALL ldo channels (LeakyReLU left non-integers): f32 accumulation of ldo terms in any order is within
            # ldo * 2^-24 * sum |terms| of the exact sum
            a, w = want.double().reshape(-1, d.ldo), d.w18.double().view(-1, d.ldo).t()[:, :18]
            z, mag = (a @ w).view(d.N, d.H2, d.W2, 18), (a.abs() @ w.abs()).view(d.N, d.H2, d.W2, 18)
            assert torch.isfinite(o["z"]).all(), "the prediction conv saw the unwritten pad channels"
            assert bool(((o["z"].double() - z).abs() <= d.ldo * 2.0 ** -24 * mag).all()), "prediction conv over the padded channels %s" % dt
        out.append(_case("flow-level-" + _NAME[dt], run_level, check_level))
    return out


_FLOW = _family(_flow_cases)
FLOW_NAMES = (["fgfa_warp_aggregate-f32", "fgfa_warp_aggregate-bf16", "fgfa_pair_taps", "flow_conv1_combine"] +
              ["%s-%s" % (n, d) for n in ("flow_pred_finish", "dff_warp_scale", "flow-level") for d in ("f32", "bf16")])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", FLOW_NAMES)
def test_fgfa_flownet(dev, name, mode):
    """fgfa_warp_aggregate (contiguous, window-order and group forms), fgfa_pair_taps with its zero rows, flow_conv1_combine,
    flow_pred_finish, dff_warp_scale, and one flow_level_assemble level after deconv4x4s2_into exactly as FlowNetS._trunk builds
    it, followed by the conv that reads the padded channels (zero weight x unwritten channel = NaN under `ones`)."""
    cases = _FLOW()
    assert sorted(cases) == sorted(FLOW_NAMES)
    _stale(cases[name], mode, dev)


# ===================================================================================================== spatial
def _spatial_cases():
    ops = _ops()
    out = []
    # ---- roi_align / roi_align_planes on the exact lattice, and K = 0
    for dt in (F32, BF16):
        def roi_inputs(which, dt=dt):
            C = 64
            feat = sc.int_features(sc.MAP_B, sc.MAP_H, sc.MAP_W, 1032, seed=1 if which == "Bp" else 0)[..., :C].contiguous()
            rois = sc.roi_lattice(7, sc.EXACT_GS)
            if which == "A":
                rois = sc.repeat_to(rois, 2 * rois.shape[0])
            elif which == "Bp":
                rois = rois.flip(0).contiguous()
            return feat, rois

        def run_roi(which, dev, dt=dt, roi_inputs=roi_inputs):
            feat, rois = roi_inputs(which)
            f, r = feat.to(dt).to(dev), rois.to(dev)
            o = {"rows": ops.roi_align(f, r, sc.SCALE, (7, 7), 0), "k0": ops.roi_align(f, r[:0].contiguous(), sc.SCALE, (7, 7), 0)}
            if dt == F32:
                o["planes"] = ops.roi_align_planes(f, r, sc.SCALE, (7, 7), 0)
                o["planes_k0"] = ops.roi_align_planes(f, r[:0].contiguous(), sc.SCALE, (7, 7), 0)
            return o

        def check_roi(o, dt=dt, roi_inputs=roi_inputs):
            feat, rois = roi_inputs("B")
            ref = sc.oracle_roi_align(feat, rois, 7, 0)
            sc.assert_bits(o["rows"], ref.to(dt), "roi_align %s" % dt)
            assert tuple(o["k0"].shape) == (0, 49, 64)
            if dt == F32:
                want = cpu_ops._planes(ref.reshape(rois.shape[0], -1), BF16)
                sc.assert_bits(o["planes"], want.t, "roi_align_planes")
                assert o["planes_k0"].shape[0] == 0
        out.append(_case("roi_align-" + _NAME[dt], run_roi, check_roi))

    # ---- stem_pool, maxpool3x3s2, avgpool2x2_ceil on odd sizes
    def run_stem(which, dev):
        hw = (2, 31, 33) if which == "A" else (1, 9, 7)
        case = ec.stem_case(hw) if which != "Bp" else ec.make_stem_case(hw, seed=99)
        w160 = ops.pack_stem_weight_bf16(case.w, BF16).to(dev)
        return {"y": ops.stem_pool(case.u8.to(dev), w160, case.scale.to(dev), case.bias.to(dev), case.mean, True)}

    def check_stem(o):
        want, _ = ec.reference_stem(ec.stem_case((1, 9, 7)), BF16, True, pool=True)
        ec.assert_bits_equal(o["y"], want, "stem_pool 9 x 7", relu=1)
    out.append(_case("stem_pool", run_stem, check_stem))

    def pool_input(which):
        shape = (3, 21, 17, 64) if which == "A" else (2, 7, 9, 8)
        g = torch.Generator().manual_seed(11 + (which == "Bp"))
        return torch.randint(-8, 9, shape, generator=g).float()

    for dt in (F32, BF16):
        def run_pool(which, dev, dt=dt):
            x = pool_input(which).to(dt).to(dev)
            return {"max": ops.maxpool3x3s2(x), "avg": ops.avgpool2x2_ceil(x)}

        def check_pool(o, dt=dt):
            x = pool_input("B")
            sc.assert_bits(o["max"], F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous().to(dt), "max-pool")
            sc.assert_bits(o["avg"], F.avg_pool2d(x.permute(0, 3, 1, 2), 2, 2, ceil_mode=True).permute(0, 2, 3, 1).contiguous().to(dt),
                           "avg-pool")
        out.append(_case("pools-" + _NAME[dt], run_pool, check_pool))

    # ---- the fused bottlenecks: dense, even pixels only, downsample
    for ds in (False, True):
        def bn_case(which, ds=ds):
            hw = (3, 37, 53) if which == "A" else (2, 9, 13)
            return ec.make_bottleneck_case(hw, BF16, seed=sum(hw) + int(ds) + 100 * (which == "Bp"), ds=ds)

        def run_bn(which, dev, ds=ds, bn_case=bn_case):
            c = bn_case(which)
            args = [c.x.to(dev)]
            for i in range(3):
                args += [c.w[i].to(dev), c.sb[i][0].to(dev), c.sb[i][1].to(dev)]
            if ds:
                return {"y": ops.bottleneck64_ds(*args, c.w[3].to(dev), c.sb[3][0].to(dev), c.sb[3][1].to(dev))}
            return {"y": ops.bottleneck64(*args), "even": ops.bottleneck64(*args, subsample=True)}

        def check_bn(o, ds=ds, bn_case=bn_case):
            want, _ = ec.reference_bottleneck(bn_case("B"))
            ec.assert_bits_equal(o["y"], want, "bottleneck64%s" % ("_ds" if ds else ""), relu=1)
            if not ds:
                ec.assert_bits_equal(o["even"], want[:, ::2, ::2].contiguous(), "bottleneck64, even pixels", relu=1)
        out.append(_case("bottleneck64_ds" if ds else "bottleneck64", run_bn, check_bn))

    # ---- resize_bilinear_u8 and its mirrored form, both passes (the tmp buffer is in use)
    def resize_inputs(which):
        (n, hi, wi), out_hw = ((3, 61, 77), (40, 50)) if which == "A" else ((2, 37, 53), (24, 40))
        g = torch.Generator().manual_seed(hi + (which == "Bp"))
        return torch.randint(0, 256, (n, hi, wi, 3), generator=g, dtype=torch.uint8), out_hw

    def run_resize(which, dev):
        from mega.pytorch_amd import feed
        frames, out_hw = resize_inputs(which)
        tables = feed.ResizeTables(tuple(frames.shape[1:3]), out_hw, dev)
        f = frames.to(dev)
        return {"resized": ops.resize_bilinear_u8(f, out_hw, tables), "flipped": ops.resize_bilinear_u8_flip(f, out_hw, tables)}

    def check_resize(o):
        frames, out_hw = resize_inputs("B")
        want = cpu_ops.resize_bilinear_u8(frames, out_hw)
        assert torch.equal(o["resized"], want) and torch.equal(o["flipped"], want.flip(2))
    out.append(_case("resize_bilinear_u8", run_resize, check_resize))
    return out


_SPATIAL = _family(_spatial_cases)
SPATIAL_NAMES = ["roi_align-f32", "roi_align-bf16", "stem_pool", "pools-f32", "pools-bf16", "bottleneck64", "bottleneck64_ds",
                 "resize_bilinear_u8"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SPATIAL_NAMES)
def test_spatial(dev, name, mode):
    """roi_align and roi_align_planes (K = 0 too), stem_pool / maxpool3x3s2 / avgpool2x2_ceil on odd sizes, bottleneck64 (dense
    and even pixels), bottleneck64_ds, resize_bilinear_u8 and _flip with both passes.  No workspace: the output (and the
    resize's tmp) is the allocation, and every element of it is defined."""
    cases = _SPATIAL()
    assert sorted(cases) == sorted(SPATIAL_NAMES)
    _stale(cases[name], mode, dev)


# ===================================================================================================== copies and casts
def _copy_cases():
    ops = _ops()
    out = []

    def src(which, dev):
        g = torch.Generator().manual_seed(3 + (which == "Bp"))
        n = 600 if which == "A" else 300
        return (torch.randn((n, 256), generator=g).to(BF16).to(dev), torch.randn((64, n), generator=g).to(BF16).to(dev),
                torch.randint(0, 256, (37, 301), generator=g, dtype=torch.uint8).to(dev))

    def run_cat(which, dev):
        big, vt, u8 = src(which, dev)
        many = [big[i * 3:i * 3 + 2] for i in range(60)]                       # with the 4 column blocks 64 segments: two launches
        cols = [vt[:, 0:75], vt[:, 75:150], vt[:, 151:154], vt[:, 3:4]]        # 150-byte rows at 2-byte alignment
        outs = ops.multi_cat([(many, 0), (cols, 1)])
        # copy_blocks into the middle of poisoned destinations: odd byte counts and alignments
        d8 = _alloc((37, 400), torch.uint8, dev)
        d16 = _alloc((64, 200), BF16, dev)
        ops.copy_blocks([(d8[:, 3:304], u8), (d16[:, 1:76], vt[:, 75:150]), (d16[:, 77:80], vt[:, 101:104])] +
                        [(d16[i:i + 1, 100:110], vt[i:i + 1, 10:20]) for i in range(60)])
        return {"cat_rows": outs[0], "cat_cols": outs[1], "d8": d8[:, 3:304], "d16a": d16[:, 1:76], "d16b": d16[:, 77:80],
                "d16c": d16[:60, 100:110],
                "untouched": {"d8 left": d8[:, :3], "d8 right": d8[:, 304:], "d16 col 0": d16[:, :1], "d16 col 76": d16[:, 76:77],
                              "d16 cols 80..99": d16[:, 80:100], "d16 right": d16[:, 110:], "d16 rows 60..": d16[60:, 100:110]}}

    def check_cat(o):
        big, vt, u8 = (t.cpu() for t in src("B", "cpu"))
        assert torch.equal(o["cat_rows"], torch.cat([big[i * 3:i * 3 + 2] for i in range(60)], 0))
        assert torch.equal(o["cat_cols"], torch.cat([vt[:, 0:75], vt[:, 75:150], vt[:, 151:154], vt[:, 3:4]], 1))
        assert torch.equal(o["d8"], u8) and torch.equal(o["d16a"], vt[:, 75:150]) and torch.equal(o["d16b"], vt[:, 101:104])
        assert torch.equal(o["d16c"], vt[:60, 10:20])
    out.append(_case("copy_blocks-multi_cat", run_cat, check_cat))

    def cast_inputs(which):
        g = torch.Generator().manual_seed(8 + (which == "Bp"))
        n = 3 if which != "A" else 2
        pieces = [torch.randn((5 * n, 64), generator=g) * 3, torch.randn((1, 64), generator=g), torch.randn((7 * n, 64), generator=g)]
        pieces += [torch.randn((2, 64), generator=g) for _ in range(60 * n // 3)]        # more than 56 segments
        flat_n = 1024 * 3 + 5 if which != "A" else 1024 * 9 + 3                        # n % 8 != 0
        return pieces, torch.randn((flat_n,), generator=g) * 3, torch.randn((11 * n, 72), generator=g) * 100

    def run_cast(which, dev):
        pieces, flat_x, x2 = cast_inputs(which)
        x2d = x2.to(dev)
        return {"cat_cast": ops.cat_rows_cast_bf16([p.to(dev) for p in pieces]), "cast_bf16": ops.cast_half(flat_x.to(dev), BF16),
                "cast_f16": ops.cast_half(flat_x.to(dev), F16), "planes": ops.split_planes(x2d), "x3": ops.split_bf16x3(x2d)}

    def check_cast(o):
        pieces, flat_x, x2 = cast_inputs("B")
        assert flat_x.numel() % 8 != 0
        assert torch.equal(o["cat_cast"].view(torch.int16), torch.cat(pieces, 0).to(BF16).view(torch.int16))
        assert torch.equal(o["cast_bf16"].view(torch.int16), flat_x.to(BF16).view(torch.int16))
        assert torch.equal(o["cast_f16"].view(torch.int16), flat_x.to(F16).view(torch.int16))
        hi, lo = ec.split_hi_lo(x2)
        assert torch.equal(o["planes"].view(torch.int16), torch.cat([hi, lo], -1).view(torch.int16))
        assert torch.equal(o["x3"].view(torch.int16), torch.cat([hi, lo, hi], -1).view(torch.int16))
    out.append(_case("casts", run_cast, check_cast))
    return out


_COPY = _family(_copy_cases)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["copy_blocks-multi_cat", "casts"])
def test_copies_casts(dev, name, mode):
    """copy_blocks and multi_cat with more than 56 segments (two launches), odd byte alignments and 150-byte rows: the bytes
    outside the destination blocks keep their poison.  cat_rows_cast_bf16, cast_half with n % 8 != 0, split_planes,
    split_bf16x3: every element of the output is defined."""
    _stale(_COPY()[name], mode, dev)


# ===================================================================================================== evaluation / linking
def _roll_scores(frames):
    """the same frames with each frame's scores rotated by one: the shapes of B, other values"""
    return [dict(f, score=np.roll(f["score"], 1)) for f in frames]


@functools.lru_cache(maxsize=None)
def _video_set(which):
    if which == "A":
        return seq_nms_twin.make_videos(21, n_videos=8, max_len=30, tracks=6, clutter=12)
    frames, videos = seq_nms_twin.make_videos(5, n_videos=3, max_len=12, tracks=3, clutter=5)
    return (frames, videos) if which == "B" else (_roll_scores(frames), videos)


_TE_SPEC = {"B": [dict(L=12, n_gt=3, labels=(1, 2), n_clutter=4) for _ in range(2)] + [dict(L=1, n_gt=2, labels=(1, 2), n_clutter=2, p_drop=0.0, p_miss=0.0)],
            # 1,100 clutter tubelets against 70 GT tracks: the pair table lives in the workspace
            "A": [dict(L=6, n_gt=70, labels=(3,), n_clutter=1100, max_gt_len=4, p_drop=0.1, p_miss=0.3)]}


@functools.lru_cache(maxsize=None)
def _tubelet_set(which):
    if which == "A":
        return track_eval_twin.make_set(33, _TE_SPEC["A"])
    return track_eval_twin.make_set(41 if which == "B" else 42, _TE_SPEC["B"])


@functools.lru_cache(maxsize=None)
def _tubelet_ws_set(which):
    """a task whose pair table does not fit LDS: it lives in the workspace (A: the same with more clutter)"""
    spec = dict(_TE_SPEC["A"][0])
    if which == "A":
        spec["n_clutter"] = 1500
    return track_eval_twin.make_set({"B": 33, "Bp": 34, "A": 35}[which], [spec])


def _bits32(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _eval_cases():
    ops = _ops()
    out = []
    from mega.pytorch_amd import demo, motion_iou, seq_nms, track_eval, tracks, vid_eval
    mods = _mods("ops", "seq_nms", "tracks", "track_eval")

    # ---- seq_nms
    def run_seq(which, dev):
        frames, videos = _video_set(which)
        r = seq_nms.run(seq_nms_twin.to_boxlists(frames), videos, device=dev)
        return {"keep": r["keep"], "scores": np.where(r["keep"], r["scores"], np.float32(0))}

    def check_seq(o):
        frames, videos = _video_set("B")
        keep, new, _ = seq_nms_twin.seq_nms(frames, videos)
        wk, ws = np.concatenate(keep), np.concatenate(new)
        np.testing.assert_array_equal(o["keep"], wk)
        np.testing.assert_array_equal(_bits32(o["scores"][wk]), _bits32(ws[wk]))
    out.append(_case("seq_nms", run_seq, check_seq, mods))

    # ---- link_tracks
    def run_link(which, dev):
        frames, videos = _video_set(which)
        r = tracks.run(tracks_twin.to_boxlists(frames), videos, rescore="avg", device=dev)
        return {"track_ids": r["track_ids"], "scores": r["scores"], "table": r["table"]}

    def check_link(o):
        frames, videos = _video_set("B")
        ids, new, table = tracks_twin.link(frames, videos, rescore="avg")
        np.testing.assert_array_equal(o["track_ids"], np.concatenate(ids).astype(np.int64))
        np.testing.assert_array_equal(_bits32(o["scores"]), _bits32(np.concatenate(new)))
        assert [(int(r["video"]), int(r["id"]), int(r["label"]), int(r["first"]), int(r["last"]), int(r["count"]), float(r["mean"]))
                for r in o["table"]] == table
    out.append(_case("link_tracks", run_link, check_link, mods))

    # ---- tubelet_scores + tubelet_match (track_eval.run), the pair table in LDS and in the workspace
    for name, pick in (("tubelets", _tubelet_set), ("tubelets-workspace", _tubelet_ws_set)):
        def run_te(which, dev, pick=pick):
            preds, gts, videos = pick(which)
            bl, gt = track_eval_twin.to_inputs(preds, gts)
            r = track_eval.run(bl, gt, videos, device=dev)
            return {k: r[k] for k in ("tubelets", "match", "matched_gt", "n_pos", "ap", "gt_table", "ws_pairs")} | \
                {"pairs": {str(k): {"hits": v["hits"], "both": v["both"]} for k, v in r["pairs"].items()}}

        def check_te(o, pick=pick, name=name):
            preds, gts, videos = pick("B")
            want = track_eval_twin.run(preds, gts, videos)
            assert (o["ws_pairs"] > 0) == name.endswith("workspace")
            assert [float(t["score"]) for t in o["tubelets"]] == [t[4] for t in want["tubelets"]]
            np.testing.assert_array_equal(o["match"], want["match"])
            np.testing.assert_array_equal(o["matched_gt"], want["matched_gt"])
            np.testing.assert_array_equal(o["n_pos"], want["n_pos"])
            for key, w in want["pairs"].items():
                np.testing.assert_array_equal(o["pairs"][str(key)]["hits"], w["hits"])
                np.testing.assert_array_equal(o["pairs"][str(key)]["both"], w["both"])
            np.testing.assert_allclose(o["ap"], want["ap"], rtol=0, atol=1e-12)
        out.append(_case(name, run_te, check_te, mods))

    # ---- vid_eval_match + vid_eval_ap
    def vid_frames(which):
        if which == "A":
            return vid_twin.make_frames(7, F=40, tie_scores=True, motion=True)
        return vid_twin.make_frames(11 if which == "B" else 12, F=12, tie_scores=True, motion=True)

    def run_vid(which, dev):
        preds, gts, mot = vid_frames(which)
        bl, gt = vid_twin.to_boxlists(preds, gts)
        r = vid_eval.match_and_ap(bl, gt, mot, device=dev)
        return {k: r[k] for k in ("match", "pred_ignore", "n_pos", "ap")}

    def check_vid(o):
        preds, gts, mot = vid_frames("B")
        for ri, w in enumerate(vid_twin.evaluate(preds, gts, mot)):
            np.testing.assert_array_equal(o["match"][ri], w["match"])
            np.testing.assert_array_equal(o["pred_ignore"][ri], w["pred_ignore"])
            np.testing.assert_array_equal(o["n_pos"][ri], w["n_pos"])
            np.testing.assert_allclose(o["ap"][ri], w["ap"], rtol=0, atol=1e-9, equal_nan=True)
    out.append(_case("vid_eval", run_vid, check_vid, mods))

    # ---- proposal_recall_match
    def prop_frames(which):
        if which == "A":
            return proposal_recall_twin.make_frames(11, F=40, ties=True)
        return proposal_recall_twin.make_frames(13 if which == "B" else 14, F=10, ties=True)

    def run_prop(which, dev):
        preds, gts = prop_frames(which)
        bl, gt = proposal_recall_twin.to_boxlists(preds, gts)
        ov, pr = vid_eval.match_proposals(bl, gt, [10, 300], dev)
        return {"gt_overlap": ov, "gt_prop": pr}

    def check_prop(o):
        preds, gts = prop_frames("B")
        for li, lim in enumerate([10, 300]):
            wov, wpr = proposal_recall_twin.match(preds, gts, lim)
            np.testing.assert_array_equal(_bits32(o["gt_overlap"][li].numpy()), _bits32(wov))
            np.testing.assert_array_equal(o["gt_prop"][li].numpy(), wpr)
    out.append(_case("proposal_recall_match", run_prop, check_prop, mods))

    # ---- motion_iou: frames that fit LDS (g_random) and the 130-box frame that runs in the workspace
    mi = motion_iou_cases.cases()
    for name, (b_name, a_name) in (("motion_iou", ("g_random", "f_130_boxes")), ("motion_iou-workspace", ("f_130_boxes", "f_130_boxes"))):
        def run_mi(which, dev, b_name=b_name, a_name=a_name):
            c = mi[a_name if which == "A" else b_name]
            gt = c["gt"]
            if which == "Bp":
                import copy
                gt = copy.copy(gt)
                gt.boxes = (gt.boxes + np.float32(1.0)).astype(np.float32)
            v, cnt = motion_iou.run(gt, c["videos"], c["window"], device=dev)
            return {"values": v, "counts": cnt}

        def check_mi(o, b_name=b_name):
            c = mi[b_name]
            tv, tc = motion_iou_twin.run(c["gt"].boxes, c["gt"].off, c["gt"].track_ids, c["videos"], c["window"])
            np.testing.assert_array_equal(o["counts"], tc)
            np.testing.assert_array_equal(o["values"].view(np.int64), tv.view(np.int64))
        out.append(_case(name, run_mi, check_mi, mods))

    # ---- overlay_detections (draws in place on the caller's frames: the workspace is the only allocation)
    atlas = demo.LabelAtlas(*demo.glyph_atlas(16))
    palette = demo.class_palette(len(demo.CATEGORIES))

    def ov_inputs(which):
        hw, rhw, Fn, R = ((375, 500), (600, 800), 5, 300) if which == "A" else ((96, 160), (96, 160), 3, 40)
        seed = 11 + (which == "Bp")
        frames = np.random.default_rng(seed).integers(0, 256, (Fn,) + hw + (3,)).astype(np.uint8)
        return (frames,) + tuple(overlay_twin.random_detections(seed, Fn, R, rhw)) + (rhw,)

    def run_ov(which, dev):
        frames, box, score, label, counts, rhw = ov_inputs(which)
        d = ops.overlay_detections(torch.from_numpy(frames).to(dev), torch.from_numpy(box).to(dev), torch.from_numpy(score).to(dev),
                                   torch.from_numpy(label).to(dev), torch.from_numpy(counts).to(dev), rhw, 0.5, 3,
                                   torch.from_numpy(palette).to(dev), atlas.to(dev))
        return {"frames": d}

    def check_ov(o):
        frames, box, score, label, counts, rhw = ov_inputs("B")
        want = overlay_twin.draw_batch(frames, box, score, label, counts, rhw, 0.5, 3, palette, atlas, demo.CATEGORIES)
        np.testing.assert_array_equal(o["frames"].numpy(), want)
        assert (want != frames).any()
    out.append(_case("overlay_detections", run_ov, check_ov, mods))
    return out


_EVAL = _family(_eval_cases)
EVAL_NAMES = ["seq_nms", "link_tracks", "tubelets", "tubelets-workspace", "vid_eval", "proposal_recall_match", "motion_iou",
              "motion_iou-workspace", "overlay_detections"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", EVAL_NAMES)
def test_evaluation(dev, name, mode):
    """seq_nms, link_tracks, tubelet_scores + tubelet_match, vid_eval_match + vid_eval_ap, proposal_recall_match, motion_iou and
    overlay_detections through their modules' entry points on the twins' small tied sets; the modules' own torch.empty sites
    (seq_nms.py, tracks.py, track_eval.py) are poisoned too.  Defined: what the entry point returns -- for Seq-NMS the
    new score where keep is set."""
    cases = _EVAL()
    assert sorted(cases) == sorted(EVAL_NAMES)
    _stale(cases[name], mode, dev)


# ===================================================================================================== whole model, eager
_MODEL_RUNS = {}


def _mega_run(dev, dtype):
    from mega.pytorch_amd import engine
    from test_e2e_gpu import _model
    from test_oracle_golden import _npz, e2e_inputs
    d = _npz("ref_e2e_r50.npz")
    sd, frames, gfor, T = e2e_inputs(d)
    nkey = int(d["cfg_nkey"])
    key = ("mega", dtype)
    if key not in _MODEL_RUNS:
        _MODEL_RUNS[key] = _model(dev, dtype, strict_gt=False, sd=sd)[1]
    eng = engine.ClipEngine(_MODEL_RUNS[key], steps_per_batch=2, graphs=False, keep_logits=True)
    dets = eng.run(frames.to(dev), T, gfor, first=0, last=nkey)
    torch.cuda.synchronize()
    return {"logits": [l.cpu() for l in eng.logits_log],
            "dets": [(b.bbox.cpu(), b.get_field("scores").cpu(), b.get_field("labels").cpu()) for b in dets[:nkey]]}


def _fgfa_run_once(dev, dtype):
    from test_e2e_gpu import _fgfa_model
    from test_oracle_golden import _npz, fgfa_inputs
    d = _npz("ref_fgfa_r50.npz")
    sd, frames, T = fgfa_inputs(d)
    key = ("fgfa", dtype)
    if key not in _MODEL_RUNS:
        _MODEL_RUNS[key] = _fgfa_model(dev, dtype, sd)
    model = _MODEL_RUNS[key]
    traces, outs = [], []
    h = model.roi_heads.box.predictor.register_forward_hook(lambda m, i, o: traces.append((o[0].float().cpu(), o[1].float().cpu())))
    try:
        for idx in range(2):
            images = {"cur": frames[idx].to(dev), "ref": [frames[min(T - 1, idx + 9)].to(dev)],
                      "frame_category": 0 if idx == 0 else 1, "seg_len": T, "ref_init": [frames[i].to(dev) for i in range(1, 10)]}
            outs.append(model(images)[0])
    finally:
        h.remove()
    torch.cuda.synchronize()
    return {"logits": [t[0] for t in traces], "deltas": [t[1] for t in traces],
            "dets": [(b.bbox.cpu(), b.get_field("scores").cpu(), b.get_field("labels").cpu()) for b in outs]}


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
@pytest.mark.parametrize("arch", ["mega", "fgfa"])
def test_whole_model_eager(dev, arch, dtype):
    """The small synthetic R-50 MEGA clip and the small FGFA clip of test_e2e_gpu.py, eager (no graph capture), with every
    torch.empty of ops, modeling, relation, fgfa, rdn and engine filled with 0xFF: detections and logits are bit-equal to
    the clean run.  (How close the clean run is to the reference is test_e2e_gpu.py's business.)"""
    run = _mega_run if arch == "mega" else _fgfa_run_once
    clean = _host(run(dev, dtype))
    again = _host(run(dev, dtype))
    _same(again, clean, "%s %s: second clean run" % (arch, dtype))
    assert sum(len(d[1]) for d in clean["dets"]) > 0
    with poison.poisoned("ones", _mods("ops", "modeling", "relation", "fgfa", "rdn", "engine")) as p:
        got = _host(run(dev, dtype))
    assert p.count >= 1 and p.ws_count >= 1
    _same(got, clean, "%s %s under ones" % (arch, dtype))
