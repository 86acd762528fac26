"""-m gpu: the kernels that turn a coordinate into a weighted gather -- ROIAlign in its three kernels and their
instantiations, the 3 x 3 max-pool and the ceil-mode 2 x 2 average (csrc/spatial.hip), the DFF and FGFA flow warps
(csrc/fgfa.hip) -- on the cases of tests/sampling_lattice_cases.py (proved on the CPU by
tests/test_sampling_lattice_cases.py), where the answer does not depend on the order of the sums:

  exact class, fixed-ratio sets, pools, DFF warp   bit for bit against the oracle rounded to the kernel's dtype
  one-ulp class                                    every element within 1 ulp of its dtype, at most 1e-3 of them different
                                                   at all (the oracle alone gives 0: only the final division rounds)
  ceil ladder (f32 forms)                          the members whose grid count is g bit for bit; the bumped member within
                                                   test_roi_align's 2e-5 of max |feature| and closer to the oracle than to
                                                   the oracle with the neighbouring grid count
  FGFA aggregate                                   the cosine and the softmax are not exact: test_fgfa_warp_aggregate's
                                                   tolerances, but PER PIXEL

Which kernel a parametrisation reaches is restated from the launch code's thresholds (sc.roi_align_form /
sc.roi_align_planes_form) and asserted against the form the case is meant for; no test inspects the binary.  Every case
prints the share of its one-ulp class that differs (run with -s)."""
import collections
import functools

import pytest
import torch
import torch.nn.functional as F

import cpu_ops
import sampling_lattice_cases as sc

pytestmark = pytest.mark.gpu

B, H, W = sc.MAP_B, sc.MAP_H, sc.MAP_W
C_MAX = 1032
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
MAX_SHARE = 1e-3


def _ops():
    from mega.pytorch_amd import ops
    return ops


def _name(dt):
    return {BF16: "bf16", F16: "f16", F32: "f32"}[dt]


# ===================================================================================================== expected values, once
@functools.lru_cache(maxsize=None)
def _expected(P, cls, C=C_MAX):
    """(rois, the oracle's f32 [K][P P][C]) of a class: 'exact', 'ulp' or 'ratio' (sampling_ratio 2)"""
    rois = {"exact": lambda: sc.roi_lattice(P, sc.EXACT_GS), "ulp": lambda: sc.ulp_set(P), "ratio": lambda: sc.ratio_lattice(P)}[cls]()
    feat = sc.int_features(B, H, W, C_MAX)[..., :C].contiguous()
    return rois, sc.oracle_roi_align(feat, rois, P, 2 if cls == "ratio" else 0)


@functools.lru_cache(maxsize=4)
def _feat(C, dtype):
    return sc.int_features(B, H, W, C_MAX)[..., :C].contiguous().to(dtype)


def _case(P, cls, C, K):
    """the class's ROIs repeated (or cut) to K rows (None: as they are) with the oracle's rows for C channels"""
    rois, ref = _expected(P, cls, C_MAX if P <= 8 else C)
    idx = torch.arange(K or rois.shape[0]) % rois.shape[0]
    return rois[idx].contiguous(), ref[idx][..., :C].contiguous()


def _compare(got, want, cls, what):
    if cls == "ulp":
        share = sc.assert_one_ulp(got, want, what, MAX_SHARE)
        print("%s: one-ulp class, %.3g of %d elements differ by 1 ulp" % (what, share, got.numel()))
    else:
        sc.assert_bits(got, want, what)


# ===================================================================================================== ROIAlign: the launch table
NHWC = (True, True)
RoiCase = collections.namedtuple("RoiCase", "form dtype C P ratio K layouts id")


def _rc(form, dtype, C, P, ratio=0, K=None, layouts=NHWC):
    cid = "%s-%s-C%d-P%d-r%d%s%s" % (form, _name(dtype), C, P, ratio, "-K%d" % K if K else "",
                                     "" if layouts == NHWC else "-%s-%s" % tuple("nhwc" if v else "nchw" for v in layouts))
    return RoiCase(form, dtype, C, P, ratio, K, layouts, cid)


def _roi_cases():
    cases = []
    for dt in (BF16, F16):
        for P in (7, 8, 4):
            cases.append(_rc("sep8", dt, 1024, P))                        # the hot form
            cases.append(_rc("sep1", dt, 64, P))
            cases.append(_rc("sep1", dt, 1032, P))                        # 129 channel vectors: no XCD slices
            cases.append(_rc("vec", dt, 64, P, ratio=2))
        cases.append(_rc("vec", dt, 64, 9))                               # pooled 9 x 9: past the separable tables
    for P, K in ((7, None), (8, None), (4, 64)):                          # K P P 128 / 8 >= 16384
        cases.append(_rc("vec-sliced", BF16, 1024, P, ratio=2, K=K))
    for P in (7, 8, 4):
        cases.append(_rc("vec", F32, 64, P))
        cases.append(_rc("vec", F32, 64, P, ratio=2))
    cases.append(_rc("vec", F32, 512, 7, K=20))                           # slices exist, 20 ROIs are below the threshold
    for P, K in ((7, 42), (8, None), (4, 64)):
        cases.append(_rc("vec-sliced", F32, 512, P, K=K))
    cases.append(_rc("vec-sliced", F32, 512, 7, ratio=2, K=42))
    for dt in (F32, BF16, F16):                                           # the generic kernel with 64, 128 and 256 threads
        cases.append(_rc("generic/64", dt, 20, 7, layouts=(True, False)))
        cases.append(_rc("generic/128", dt, 136, 7, layouts=(False, False)))
        cases.append(_rc("generic/256", dt, 264, 7, layouts=(False, True)))
    cases.append(_rc("generic/64", F32, 18, 7))                           # NHWC both ways, C no multiple of a channel vector
    cases.append(_rc("generic/64", BF16, 20, 7, ratio=2))
    return cases


def _run_roi_align(dev, c, rois):
    in_nhwc, out_nhwc = c.layouts
    feat = _feat(c.C, c.dtype)
    if not in_nhwc:
        feat = feat.permute(0, 3, 1, 2).contiguous()
    got = _ops().roi_align(feat.to(dev), rois.to(dev), sc.SCALE, (c.P, c.P), c.ratio, in_nhwc=in_nhwc, out_nhwc=out_nhwc).cpu()
    if not out_nhwc:
        got = got.permute(0, 2, 3, 1).reshape(rois.shape[0], c.P * c.P, c.C).contiguous()
    return got


@pytest.mark.parametrize("c", _roi_cases(), ids=lambda c: c.id)
def test_roi_align_lattice(dev, c):
    classes = ("ratio",) if c.ratio else ("exact",) if c.P > 8 else ("exact", "ulp")
    for cls in classes:
        rois, ref = _case(c.P, cls, c.C, c.K)
        assert sc.roi_align_form(c.dtype, c.C, rois.shape[0], c.P, c.ratio, *c.layouts) == c.form, "the case misses its kernel"
        got = _run_roi_align(dev, c, rois)
        _compare(got, ref.to(c.dtype), cls, "%s %s (%d ROIs)" % (c.id, cls, rois.shape[0]))


LADDER_CASES = [_rc("vec", F32, 64, 7), _rc("vec-sliced", F32, 512, 7), _rc("generic/64", F32, 20, 7, layouts=(True, False))]


@functools.lru_cache(maxsize=None)
def _ladder_expected():
    lad = sc.ceil_ladder(7)
    feat = _feat(512, F32)
    ref = sc.oracle_roi_align(feat, lad.rois, 7, 0)
    alt = {k: torch.from_numpy(sc.roi_align_f64(feat, lad.rois[k:k + 1], 7, 0, grid_h=lad.g[k])[0]).float()
           for k, kind in enumerate(lad.kind) if kind == "up"}
    return lad, ref, alt


@pytest.mark.parametrize("c", LADDER_CASES, ids=lambda c: c.id)
def test_roi_align_ceil_ladder(dev, c):
    """grid = ceil(roi_height / 7) one f32 step around the integer: the exact member bit for bit; the bumped member (count
    g + 1) within 2e-5 of max |feature| and closer to the oracle than to the oracle with the count g"""
    lad, ref, alt = _ladder_expected()
    assert sc.roi_align_form(c.dtype, c.C, lad.rois.shape[0], 7, 0, *c.layouts) == c.form
    got = _run_roi_align(dev, c, lad.rois)
    for k, kind in enumerate(lad.kind):
        want = ref[k][:, :c.C]
        what = "%s ladder g %d %s (grid %d)" % (c.id, lad.g[k], kind, lad.grids[k])
        if kind == "exact":
            sc.assert_bits(got[k], want.contiguous(), what)
        elif kind == "up":
            err, other = float((got[k] - want).abs().max()), float((got[k] - alt[k][:, :c.C]).abs().max())
            print("%s: |got - oracle| %.3g, |got - oracle with grid %d| %.3g" % (what, err, lad.g[k], other))
            assert err <= 2e-5 * 8, what
            assert err < other, what + ": the kernel took the neighbouring grid count"


@pytest.mark.parametrize("c", LADDER_CASES, ids=lambda c: c.id)
def test_roi_align_ceil_ladder_lower_member_bits(dev, c):
    """the member one f32 step below the integer keeps the count g: bit for bit against the oracle"""
    lad, ref, _ = _ladder_expected()
    got = _run_roi_align(dev, c, lad.rois)
    rows = [k for k, kind in enumerate(lad.kind) if kind == "down"]
    for k in rows:
        d = got[k] != ref[k][:, :c.C]
        print("%s ladder g %d down: %d of %d elements differ, max |d| %.3g" % (c.id, lad.g[k], int(d.sum()), d.numel(),
                                                                              float((got[k] - ref[k][:, :c.C]).abs().max())))
    sc.assert_bits(got[rows], ref[rows][:, :, :c.C].contiguous(), "%s ladder, the members one step below" % c.id)


# ===================================================================================================== ROIAlign: planes
PLANES_CASES = [("sep8-planes", 512, 7, 0, 42), ("sep8-planes", 512, 8, 0, None), ("sep8-planes", 512, 4, 0, 64),
                ("vec-planes", 512, 7, 0, 20), ("vec-planes", 32, 7, 0, None), ("vec-sliced-planes", 512, 7, 2, 42)]


@pytest.mark.parametrize("dtype", [BF16, F16], ids=_name)
@pytest.mark.parametrize("form,C,P,ratio,K", PLANES_CASES, ids=lambda v: str(v))
def test_roi_align_planes_lattice(dev, dtype, form, C, P, ratio, K):
    """f32 features, the pooled rows as [hi | lo] planes, against the split of the oracle's f32 rows (cpu_ops.roi_align_planes'
    arithmetic): the hi plane and the lo plane separately"""
    feat = _feat(C, F32).to(dev)
    for cls in (("ratio",) if ratio else ("exact", "ulp")):
        rois, ref = _case(P, cls, C, K)
        n = rois.shape[0]
        assert sc.roi_align_planes_form(C, n, P, ratio) == form, "the case misses its kernel"
        want = cpu_ops._planes(ref.reshape(n, -1), dtype)
        got = _ops().roi_align_planes(feat, rois.to(dev), sc.SCALE, (P, P), ratio, dtype=dtype)
        assert got.C == want.C == P * P * C
        t = got.t.cpu().reshape(n, 2, P * P, C)
        w = want.t.reshape(n, 2, P * P, C)
        for plane, pname in ((0, "hi"), (1, "lo")):
            _compare(t[:, plane].contiguous(), w[:, plane].contiguous(), cls,
                     "%s %s C %d P %d ratio %d %s, %s plane (%d ROIs)" % (form, _name(dtype), C, P, ratio, cls, pname, n))


# ===================================================================================================== pools
def _maxpool_ref(x):
    return F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()


def _avgpool_ref(x):
    return F.avg_pool2d(x.permute(0, 3, 1, 2), 2, 2, ceil_mode=True).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=_name)
def test_maxpool3x3s2_integer_maps(dev, dtype):
    for name, x in sc.pool_cases():
        got = _ops().maxpool3x3s2(x.to(dtype).to(dev)).cpu()
        sc.assert_bits(got, _maxpool_ref(x).to(dtype), "max-pool %s %s" % (name, _name(dtype)))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
def test_avgpool2x2_ceil_integer_maps(dev, dtype):
    """the divisors are 1, 2 and 4 and the sums small integers: bit for bit"""
    for name, x in sc.pool_cases():
        got = _ops().avgpool2x2_ceil(x.to(dtype).to(dev)).cpu()
        sc.assert_bits(got, _avgpool_ref(x).to(dtype), "avg-pool %s %s" % (name, _name(dtype)))


def test_pools_past_the_grid_cap(dev):
    """more one-vector work items than 8192 blocks x 256 threads: the grid-stride loops iterate"""
    x = sc.pool_big()
    assert sc.pool_work_items(tuple(x.shape), 4, "max") > 8192 * 256 and sc.pool_work_items(tuple(x.shape), 4, "avg") > 8192 * 256
    xd = x.to(dev)
    sc.assert_bits(_ops().maxpool3x3s2(xd).cpu(), _maxpool_ref(x), "max-pool %s f32" % (tuple(x.shape),))
    sc.assert_bits(_ops().avgpool2x2_ceil(xd).cpu(), _avgpool_ref(x), "avg-pool %s f32" % (tuple(x.shape),))


# ===================================================================================================== warps
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("hw", sc.WARP_MAPS, ids=lambda v: "%dx%d" % v)
def test_dff_warp_scale_lattice(dev, dtype, hw):
    Hm, Wm = hw
    flows = sc.warp_lattice(Hm, Wm)
    for C in (8, 64):
        feats = sc.int_features(1, Hm, Wm, C, seed=Hm)[0].to(dtype)
        scale = sc.pow2_scale(Hm, Wm, C, seed=Hm).to(dtype)
        for name, flow in zip(sc.WARP_FIELDS, flows):
            want = cpu_ops.dff_warp_scale(feats, flow, scale)
            got = _ops().dff_warp_scale(feats.to(dev), flow.contiguous().to(dev), scale.to(dev)).cpu()
            sc.assert_bits(got, want, "dff warp %d x %d x %d %s, field %s" % (Hm, Wm, C, _name(dtype), name))


FGFA_CHANNELS = {F32: (16, 24), BF16: (64, 128)}
FGFA_TOL = {F32: (1e-5, 2e-5), BF16: (1e-2, 2e-3)}          # output (of the pixel's max |ref|), weights: test_fgfa_warp_aggregate's


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("hw", sc.WARP_MAPS, ids=lambda v: "%dx%d" % v)
def test_fgfa_warp_aggregate_lattice_per_pixel(dev, dtype, hw):
    from oracle import mega_oracle as mo
    Hm, Wm = hw
    Cf, Ce = FGFA_CHANNELS[dtype]
    flows = sc.warp_lattice(Hm, Wm)
    T = flows.shape[0]
    feats = sc.int_features(T, Hm, Wm, Cf + Ce, seed=50 + Hm).to(dtype)
    want, want_w = mo.fgfa_aggregate(feats.float().permute(0, 3, 1, 2), flows, sc.WARP_KEY, nfeat=Cf)
    out, w = _ops().fgfa_warp_aggregate(feats.to(dev), flows.to(dev), Cf, sc.WARP_KEY, want_weights=True)
    tol, wtol = FGFA_TOL[dtype]
    werr = float((w.cpu() - want_w[:, 0]).abs().max())
    worst = sc.assert_per_pixel(out.float().cpu(), want[0].permute(1, 2, 0), tol, "fgfa %d x %d %s" % (Hm, Wm, _name(dtype)))
    print("fgfa %d x %d %s: weights off by %.3g, worst pixel at %.3g of its tolerance" % (Hm, Wm, _name(dtype), werr, worst))
    assert werr < wtol


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("hw", sc.WARP_MAPS, ids=lambda v: "%dx%d" % v)
def test_fgfa_identical_frames_weigh_one_over_T(dev, dtype, hw):
    """T identical frames under T identical flow fields: every weight is 1 / T and the sum is the one warped frame"""
    Hm, Wm = hw
    Cf, Ce = FGFA_CHANNELS[dtype]
    T = 5
    for field in ("mixed", "whole"):
        flow = sc.warp_lattice(Hm, Wm)[sc.WARP_FIELDS.index(field)]
        frame = sc.int_features(1, Hm, Wm, Cf + Ce, seed=60 + Hm).to(dtype)
        out, w = _ops().fgfa_warp_aggregate(frame.expand(T, -1, -1, -1).contiguous().to(dev), flow[None].expand(T, -1, -1, -1).contiguous().to(dev),
                                            Cf, T // 2, want_weights=True)
        one = cpu_ops.dff_warp_scale(frame[0, :, :, :Cf].contiguous(), flow, torch.ones((Hm, Wm, Cf), dtype=dtype))
        werr = float((w.cpu() - 1.0 / T).abs().max())
        assert werr <= 2e-6, werr
        share = sc.assert_one_ulp(out.cpu(), one, "fgfa identical frames %d x %d %s %s" % (Hm, Wm, _name(dtype), field), 1.0)
        print("fgfa identical frames %d x %d %s %s: weights within %.3g of 1/T, %.3g of the outputs 1 ulp off" % (Hm, Wm, _name(dtype), field, werr, share))
