"""The cases of tests/sampling_lattice_cases.py, proved on the CPU with the oracle alone before the GPU file trusts them:
(1) on the exact class the f32 oracle equals the float64 restatement bit for bit (and so do its 16-bit roundings and its
split-precision planes); on the one-ulp class it equals the float64 value rounded to f32; (2) the census: every set puts
samples ON -1, 0, N - 1 and N and beyond both ends, along both axes, and the sets together reach every column-count dispatch
of the separable kernel, odd and even row counts, an empty patch and the oversize fallback; (3) the ceil ladder's grid counts;
(4) the warp lattice is exact and clamps on all four sides; (5) the helpers the GPU file uses reject an answer with one
planted fault.  Each test prints its figures (run with -s to see them)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cpu_ops
import sampling_lattice_cases as sc

POOLED = (4, 7, 8)
C_CPU = 24          # channels of the CPU proofs (the GPU file uses up to 1032 of the same generator's channels)


def _feat(C=C_CPU):
    return sc.int_features(sc.MAP_B, sc.MAP_H, sc.MAP_W, C)


def _f32(x64):
    return torch.from_numpy(x64.astype(np.float32))


def _sets(P):
    return (("exact g %s" % (sc.EXACT_GS,), sc.roi_lattice(P, sc.EXACT_GS), 0), ("one-ulp g %s + 11" % (sc.ULP_GS,), sc.ulp_set(P), 0),
            ("ratio 2 m %s" % (sc.RATIO_MS,), sc.ratio_lattice(P), 2))


def test_features_are_integers_and_no_two_planes_are_equal():
    f = sc.int_features(sc.MAP_B, sc.MAP_H, sc.MAP_W, 1032)
    assert torch.equal(f, f.round()) and float(f.min()) == -8 and float(f.max()) == 8
    planes = f.permute(0, 3, 1, 2).reshape(sc.MAP_B * 1032, -1).numpy()
    assert len(np.unique(planes, axis=0)) == len(planes)
    assert torch.equal(sc.int_features(sc.MAP_B, sc.MAP_H, sc.MAP_W, 1032)[..., :64], f[..., :64])


# ===================================================================================================== ROIAlign: exactness
@pytest.mark.parametrize("P", POOLED)
def test_exact_class_oracle_equals_float64_bit_for_bit(P):
    feat = _feat()
    for name, rois, ratio in (_sets(P)[0], _sets(P)[2]):
        want64 = sc.roi_align_f64(feat, rois, P, ratio)
        assert np.array_equal(want64, want64.astype(np.float32).astype(np.float64)), "%s: not representable in f32" % name
        got = sc.oracle_roi_align(feat, rois, P, ratio)
        sc.assert_bits(got, _f32(want64), "P %d %s: oracle vs float64" % (P, name))
        for dt in (torch.bfloat16, torch.float16):
            sc.assert_bits(got.to(dt), torch.from_numpy(want64).to(dt), "P %d %s rounded to %s" % (P, name, dt))
            pl = cpu_ops.roi_align_planes(feat, rois, sc.SCALE, (P, P), ratio, dtype=dt)
            w32 = _f32(want64).reshape(len(rois), -1)
            hi = w32.to(dt)
            sc.assert_bits(pl.t[:, :pl.C], hi, "P %d %s hi plane %s" % (P, name, dt))
            sc.assert_bits(pl.t[:, pl.C:], (w32 - hi.float()).to(dt), "P %d %s lo plane %s" % (P, name, dt))
        print("P %d %s: %d ROIs, oracle == float64 bit for bit (f32, bf16, f16, planes); %d of %d outputs nonzero" % (
            P, name, len(rois), int((want64 != 0).sum()), want64.size))


@pytest.mark.parametrize("P", POOLED)
def test_one_ulp_class_oracle_equals_rounded_float64(P):
    feat = _feat()
    rois = sc.ulp_set(P)
    want64 = sc.roi_align_f64(feat, rois, P, 0)
    got = sc.oracle_roi_align(feat, rois, P, 0)
    inexact = float((want64 != want64.astype(np.float32).astype(np.float64)).mean())
    share = sc.assert_one_ulp(got, _f32(want64), "P %d one-ulp class: oracle vs f32(float64)" % P, 0.0)
    print("P %d one-ulp class: %d ROIs, %.1f %% of the float64 values are not f32 numbers; oracle vs f32(float64): max 0 ulp, share %g" % (
        P, len(rois), 100 * inexact, share))
    assert inexact > 0.3 and share == 0.0
    # what the separable kernel does instead of the division: the product with the rounded reciprocal, at most 1 ulp away
    counts = np.array([np.prod([g for _, _, g in sc._roi_geometry(r, P, 0)]) for r in rois.numpy()], dtype=np.float64)
    sums64 = sc.roi_align_f64(feat, rois, P, 0, divide=False)
    sums = sums64.astype(np.float32)
    assert np.array_equal(sums.astype(np.float64), sums64)
    prod = torch.from_numpy(sums * (np.float32(1) / counts.astype(np.float32))[:, None, None])
    d = (sc._ordered(prod) - sc._ordered(got)).abs()
    print("P %d one-ulp class: sum * (1 / count) against sum / count: max %d ulp, %.3g of the f32 values differ; %.3g after rounding to bf16, %.3g to f16" % (
        P, int(d.max()), float((d > 0).double().mean()), float((prod.bfloat16() != got.bfloat16()).double().mean()),
        float((prod.half() != got.half()).double().mean())))
    assert int(d.max()) <= 1


# ===================================================================================================== census
def test_census_every_boundary_and_every_dispatch_is_reached():
    ncm, nr = set(), set()
    for P in POOLED:
        for name, rois, ratio in _sets(P):
            counts, patches = sc.census(rois, P, sc.MAP_H, sc.MAP_W, ratio)
            print("P %d %s: x %s  y %s" % (P, name, counts["x"], counts["y"]))
            print("    NCm classes %s, NR %s" % (sorted({sc.ncm_class(c) for _, c in patches}), sorted({r for r, _ in patches})))
            for a in "xy":
                assert all(counts[a][k] > 0 for k in sc.BOUNDARY_KEYS), (P, name, a, counts[a])
            if ratio == 0:
                ncm |= {sc.ncm_class(c) for _, c in patches}
                nr |= {r for r, _ in patches}
                assert (0, 0) in patches, "no ROI with an empty patch"
    assert ncm == {"empty", "<=3", "4", "5-6", "7-10", ">10"}, ncm
    assert any(r % 2 for r in nr) and any(r and r % 2 == 0 for r in nr) and 10 in nr and max(nr) > 10, nr
    # the oversize ROI alone takes the fallback: a patch wider than the 10-slot tables
    for P in POOLED:
        _, patches = sc.census(sc.oversize_roi(P), P, sc.MAP_H, sc.MAP_W)
        assert max(patches[0]) == sc.OVERSIZE_G + 1
        _, patches = sc.census(sc.roi_lattice(P, sc.EXACT_GS + sc.ULP_GS), P, sc.MAP_H, sc.MAP_W)
        assert max(max(p) for p in patches) == 10


def test_ceil_ladder_grid_counts():
    lad = sc.ceil_ladder(7)
    for g in range(1, 9):
        got = [n for n, gg in zip(lad.grids, lad.g) if gg == g]
        assert got == [g, g + 1, g], (g, got)
    feat = _feat()
    # the bumped ('up') ROIs are in general position: no sample within 1e-3 of a skip boundary, and the two grid counts the
    # ladder separates give results far apart compared with the 2e-5 * 8 the GPU file allows; the 'down' ROIs keep the count g
    ref = sc.oracle_roi_align(feat, lad.rois, 7, 0)
    gaps = []
    for k, kind in enumerate(lad.kind):
        if kind == "exact":
            sc.assert_bits(ref[k], _f32(sc.roi_align_f64(feat, lad.rois[k:k + 1], 7, 0))[0], "ladder g %d exact" % lad.g[k])
            continue
        own = _f32(sc.roi_align_f64(feat, lad.rois[k:k + 1], 7, 0))[0]
        assert float((own - ref[k]).abs().max()) < 1e-5
        if kind == "up":
            (_, _, _), (sy, by, gy) = sc._roi_geometry(lad.rois[k].numpy(), 7, 0)
            ys = np.array([sy + p * by + (i + 0.5) * by / gy for p in range(7) for i in range(gy)])
            assert gy == lad.g[k] + 1 and np.abs(ys + 1).min() > 1e-3 and np.abs(ys - sc.MAP_H).min() > 1e-3
            alt = _f32(sc.roi_align_f64(feat, lad.rois[k:k + 1], 7, 0, grid_h=lad.g[k]))[0]
            gaps.append(float((alt - ref[k]).abs().max()))
    print("ceil ladder: grids %s; |oracle - oracle with the neighbouring grid count| >= %.3g" % (lad.grids, min(gaps)))
    assert len(gaps) == 8 and min(gaps) > 0.1


# ===================================================================================================== warps
@pytest.mark.parametrize("H,W", sc.WARP_MAPS)
def test_warp_lattice_is_exact_and_clamps_on_every_side(H, W):
    flows = sc.warp_lattice(H, W)
    feats = sc.int_features(1, H, W, 8, seed=H)[0]
    scale = sc.pow2_scale(H, W, 8, seed=H)
    total = dict.fromkeys(("left", "right", "top", "bottom", "whole_x", "whole_y"), 0)
    for name, flow in zip(sc.WARP_FIELDS, flows):
        cen = sc.warp_census(flow.numpy(), H, W)
        for k in total:
            total[k] += cen[k]
        want64 = sc.warp_f64(feats, flow) * scale.double().numpy()
        assert np.array_equal(want64, want64.astype(np.float32).astype(np.float64))
        sc.assert_bits(cpu_ops.dff_warp_scale(feats, flow, scale), _f32(want64), "%d x %d %s: grid_sample vs float64" % (H, W, name))
        for dt in (torch.bfloat16,):
            sc.assert_bits(cpu_ops.dff_warp_scale(feats.to(dt), flow, scale.to(dt)), torch.from_numpy(want64).to(dt), "%s %s" % (name, dt))
    print("%d x %d: %s; grid_sample == float64 bit for bit on all %d fields" % (H, W, total, len(flows)))
    assert all(v > 0 for v in total.values()), total
    assert not bool(flows[sc.WARP_KEY].any())
    far = sc.warp_census(flows[sc.WARP_FIELDS.index("far")].numpy(), H, W)
    assert far["left"] + far["right"] == H * W and far["top"] + far["bottom"] == H * W


# ===================================================================================================== planted faults
@pytest.mark.parametrize("fault", sc.FAULTS)
def test_planted_roi_align_fault_is_rejected(fault):
    """each fault, built by a modified copy of the restatement, must be rejected by the helper the GPU file uses on the class
    it uses it on, in f32 and after rounding to bf16"""
    feat = _feat()
    for P in POOLED:
        for name, rois, helper in (("exact", sc.roi_lattice(P, sc.EXACT_GS), "bits"), ("one-ulp", sc.ulp_set(P), "ulp")):
            want = _f32(sc.roi_align_f64(feat, rois, P, 0))
            bad = _f32(sc.roi_align_f64(feat, rois, P, 0, fault=fault))
            for dt in (torch.float32, torch.bfloat16):
                with pytest.raises(AssertionError, match="differ|1 ulp"):
                    if helper == "bits":
                        sc.assert_bits(bad.to(dt), want.to(dt), fault)
                    else:
                        sc.assert_one_ulp(bad.to(dt), want.to(dt), fault, 1e-3)
            print("%s, P %d, %s class: rejected in f32 and bf16 (%d of %d f32 outputs differ)" % (
                fault, P, name, int((bad != want).sum()), want.numel()))


def test_planted_warp_fault_is_rejected():
    for H, W in sc.WARP_MAPS:
        feats = sc.int_features(1, H, W, 8, seed=H)[0]
        flows = sc.warp_lattice(H, W)
        hit = 0
        for name, flow in zip(sc.WARP_FIELDS, flows):
            want, bad = _f32(sc.warp_f64(feats, flow)), _f32(sc.warp_f64(feats, flow, fault="clamp_before_unnormalise"))
            if name == "zero":
                continue
            for dt in (torch.float32, torch.bfloat16):
                with pytest.raises(AssertionError, match="differ"):
                    sc.assert_bits(bad.to(dt), want.to(dt), name)
                with pytest.raises(AssertionError, match="pixels off"):
                    sc.assert_per_pixel(bad.to(dt), want.to(dt), 1e-2, name)
            hit += 1
        print("%d x %d: clamp before the un-normalisation rejected on %d fields, in f32 and bf16" % (H, W, hit))


def test_helpers_accept_what_they_should():
    x = torch.tensor([1.0, -2.5, 0.0, 3.0])
    y = x.clone()
    y[0] = float(np.nextafter(np.float32(1), np.float32(2)))
    sc.assert_bits(x, x.clone(), "same")
    assert sc.assert_one_ulp(y, x, "one step", 0.25) == 0.25
    with pytest.raises(AssertionError, match="more than"):
        sc.assert_one_ulp(y, x, "one step", 0.2)
    with pytest.raises(AssertionError, match="more than 1 ulp"):
        sc.assert_one_ulp(x + torch.tensor([0.0, 1e-6, 0.0, 0.0]), x, "two steps", 1.0)
    with pytest.raises(AssertionError, match=r"first at \(1,\)"):
        sc.assert_bits(torch.tensor([0.0, -0.0]), torch.tensor([0.0, 0.0]), "signed zero")


# ===================================================================================================== pools
def test_pool_cases_are_integer_maps_with_exact_answers():
    names = [n for n, _ in sc.pool_cases()]
    assert len(set(names)) == len(names)
    sides = set()
    for name, x in sc.pool_cases():
        assert torch.equal(x, x.round()) and x.shape[3] in (8, 64)
        sides.add(tuple(x.shape[1:3]))
        assert bool((x < 0).all()) == name.startswith("neg-")
        avg = F.avg_pool2d(x.permute(0, 3, 1, 2), 2, 2, ceil_mode=True)
        assert torch.equal(avg * 4, (avg * 4).round()) and torch.equal(avg.bfloat16().float(), avg)
    assert {(a, b) for a in sc.POOL_SIDES for b in sc.POOL_SIDES} <= sides
    for kind in ("max", "avg"):
        assert sc.pool_work_items(sc.POOL_BIG, 4, kind) > 8192 * 256
        assert max(sc.pool_work_items(tuple(x.shape), 4, kind) for _, x in sc.pool_cases()) < 8192 * 256
    print("%d pool maps, sides %s; the big one %s: %d work items against %d" % (
        len(names), sc.POOL_SIDES, sc.POOL_BIG, sc.pool_work_items(sc.POOL_BIG, 4, "max"), 8192 * 256))
