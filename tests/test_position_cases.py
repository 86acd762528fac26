"""tests/position_cases.py checked on the CPU before the GPU file trusts it: (1) every box set is what it claims -- integer
corners, widths, centres and centre differences exact in f32, |log-ratio| <= PM_MAX, the extremes reached; (2) the derived
constants have the values the docstring states, and the 16-bit outward rounding and the probe inverse work; (3) the f32 twin
(cpu_ops.position_logits) meets the precise bounds and the f32 emulation of the fast arithmetic meets the fast bounds with
NO v_sin allowance (libm's sine stands in), on every set, shape and weight family; (4) every planted fault is rejected by
a probe, floor or straddle check, and the message lists the faults the old-style seeded comparison (exp() within 6e-3)
and the seeded per-pair bound alone would miss.  Each test prints its figures (run with -s)."""
import math

import numpy as np
import pytest
import torch

import cpu_ops
import position_cases as pc

CASES = [(s, Nq, Nk) for s in pc.SETS for (Nq, Nk) in pc.SHAPES]


def _id(c):
    return "%s-%dx%d" % c


# ------------------------------------------------------------------------------------------------ (1) the box sets
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_box_set_is_exact(case):
    name, Nq, Nk = case
    bq, bk = pc.box_set(name, Nq, Nk)
    assert tuple(bq.shape) == (Nq, 4) and tuple(bk.shape) == (Nk, 4) and bq.dtype == torch.float32
    for b in (bq, bk):
        assert torch.equal(b, b.round()) and b.min() >= 0 and b.max() <= 2047
        assert (b[:, 2] >= b[:, 0]).all() and (b[:, 3] >= b[:, 1]).all()
    g32, g64 = pc.geometry(bq, bk, torch.float32), pc.geometry(bq, bk, torch.float64)
    for n in g32:
        assert torch.equal(g32[n].double(), g64[n]), n
    pm, _ = pc.reference(name, Nq, Nk)
    assert torch.isfinite(pm).all() and pm.abs().max() <= pc.PM_MAX
    if name == "self":
        assert torch.equal(bq, bk[:Nq])
        i = torch.arange(Nq)
        assert torch.allclose(pm[i, i, :2], torch.full((Nq, 2), math.log(1e-3), dtype=torch.float64)) and (pm[i, i, 2:] == 0).all()
    if name == "concentric" and Nq > 1:
        assert (g64["ddx"] == 0).any() and (g64["ddx"].abs() <= 0.5).all() and pm[:, :, 2].abs().max() > 1
    if name == "equal_size":
        assert (pm[:, :, 2:] == 0).all()
    if name == "ratio999":
        # |dx| / w = 999 / 1000: the f32 sum with 1e-3f rounds to 1.0 and the logarithm is exactly 0
        hit = (g64["ddx"].abs() == 999) & (g64["wq"][:, None] == 1000)
        assert hit.any() and hit[0, 0]
        s = (g32["ddx"] / g32["wq"][:, None]).abs() + np.float32(1e-3)
        assert (s[hit] == 1.0).all() and (s[hit].log() == 0).all()
    if name in ("extremes", "wide1333") and Nk >= 64:
        W = 1000.0 if name == "extremes" else 1333.0
        assert abs(pm[:, :, 2].max() - math.log(W)) < 1e-12 and abs(pm[:, :, 2].min() + math.log(W)) < 1e-12
        assert abs(pm[:, :, 3].max() - math.log(W)) < 1e-12 and abs(pm[:, :, 3].min() + math.log(W)) < 1e-12
        assert pm[:, :, 0].min() == math.log(1e-3) and abs(pm[:, :, 0].max() - math.log(W - 1 + 1e-3)) < 1e-12
    if name == "wide1333" and Nk >= 64:
        assert 100 * pm.abs().max() * pc.INV2PI > 110          # past the figure sin_rev's comment was written with


def test_small_shapes_keep_their_edges():
    """(1, 1) and the first rows of the extreme sets are fixed by hand"""
    pm, _ = pc.reference("extremes", 1, 1)
    assert abs(pm[0, 0, 2] - math.log(1000)) < 1e-12
    pm, _ = pc.reference("extremes", 8, 64)
    assert pm[1, 0, 0] == math.log(1e-3) and abs(pm[1, 2, 0] - math.log(999.001)) < 1e-12 and abs(pm[1, 1, 2] + math.log(1000)) < 1e-12


# ------------------------------------------------------------------------------------------------ (2) constants and helpers
def test_derived_constants():
    print("PM_ERR_PRECISE %.3g PHASE_PRECISE %.3g SINCOS_ABS %.3g REDUCE_ABS %.3g" % (
        pc.PM_ERR_PRECISE, pc.PHASE_PRECISE, pc.SINCOS_ABS, pc.REDUCE_ABS))
    print("PM_ERR_FAST %.3g CREV_REL %.3g PHASE_FAST_I * dim %s V_SIN_ABS %.3g" % (
        pc.PM_ERR_FAST, pc.CREV_REL, ["%.3g" % v for v in (pc.PHASE_FAST_I * pc.DIM).tolist()], pc.V_SIN_ABS))
    print("readback: " + ", ".join("%s %.3g" % (k, pc.readback(k)) for k in pc.KINDS))
    assert abs(pc.PM_ERR_PRECISE - 1.6e-6) < 1e-8 and abs(pc.PHASE_PRECISE - 2.33e-4) < 1e-6
    assert abs(pc.PM_ERR_FAST - 1.21e-6) < 1e-8 and pc.CREV_REL <= 3 * pc.U
    assert abs(pc.REDUCE_ABS - 5.5e-7) < 1e-8
    assert pc.PHASE_FAST + pc.V_SIN_ABS <= 2e-4, "the fast phase bound is past the point where the derivation is suspect"
    assert pc.XREV_MAX > 114 and float(pc.ulp32(pc.XREV_MAX)) == 2.0 ** -17
    assert pc.V_SIN_ABS == 2 * max(0.0, *pc.V_SIN_EXCESS.values())
    assert len(set(pc.FLOOR_BIASES.view(torch.int32).tolist())) == 16


@pytest.mark.parametrize("dtype", [pc.BF16, pc.F16])
def test_round16_is_outward(dtype):
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.randn(4000, generator=g, dtype=torch.float64) * 8, torch.tensor([0.0, -13.815510557964274, 1e-6, -1e-6, 4.6]),
                   torch.randn(100, generator=g).to(dtype).double()])
    lo, hi = pc.round16(x, dtype, True), pc.round16(x, dtype, False)
    assert (lo <= x).all() and (hi >= x).all()
    for v in (lo, hi):
        assert torch.equal(v.to(dtype).double(), v)                 # representable
    exact = x.to(dtype).double() == x
    assert torch.equal(lo[exact], x[exact]) and torch.equal(hi[exact], x[exact]) and exact.sum() >= 100
    # neighbours: nothing representable lies strictly between lo and hi where x is not representable
    up = pc._step16(lo.to(dtype), dtype, False).double()
    assert torch.equal(up[~exact], hi[~exact])


def test_probe_inverse_round_trips():
    e = torch.linspace(-1, 1, 2001, dtype=torch.float64)
    for sign in (1, -1):
        for b in (pc.PROBE_BIAS, 0.0):
            pre = b + sign * e
            ok = pre > -1e-6
            back = pc.embedding_from_logit((pre[ok] + 1e-6).log(), b, sign)
            assert (back - e[ok]).abs().max() < 1e-15
    for r, sign in pc.PROBES:
        wg_t, bg = pc.probe_weights(r, sign)
        assert (wg_t != 0).sum() == 16 and (bg == 2).all()
        for h in range(16):
            assert wg_t[16 * r + h, h] == sign
        for dt in (pc.BF16, pc.F16):
            assert torch.equal(wg_t.to(dt).float(), wg_t)
    assert sorted(int(j) for r in range(4) for j in pc.probed_entries(r)) == list(range(64))


# ------------------------------------------------------------------------------------------------ (3) twin and emulation
def _stand_in(kind, case, fault=None):
    """run(wg_t, bg) of the CPU stand-in of `kind` on the case's boxes: the f32 twin, or the emulation (its embedding once)"""
    bq, bk = pc.box_set(*case)
    if kind == "precise":
        return lambda wg_t, bg: cpu_ops.position_logits(bq, bk, wg_t, bg, pc.dim_mat())[:, :, :bk.shape[0]]
    emb16 = pc.emulate_embedding(bq, bk, kind, fault)
    return lambda wg_t, bg: pc.emulate_fast(bq, bk, wg_t, bg, kind=kind, fault=fault, emb16=emb16)


def _check_all(kind, case, fault=None):
    """every check of the GPU file on the CPU stand-in of `kind`, with NO v_sin allowance -> {check name: worst ratio}"""
    run = _stand_in(kind, case, fault)
    out = {"probe": pc.check_probes(kind, case, run, v_sin_abs=0.0)[0], "floor": pc.check_floor(kind, case, run)[0],
           "straddle": pc.check_straddle(kind, case, run, v_sin_abs=0.0)[0]}
    if case[0] in pc.LATTICE_SETS:
        out["seeded"] = pc.check_seeded(kind, case, run, v_sin_abs=0.0)[0]
        _, emb = pc.reference(*case)
        wg_t, bg = pc.seeded_weights()
        out["old"] = 0.0 if pc.old_style_seeded_ok(run(wg_t, bg), emb, wg_t, bg) else math.inf
    return out


@pytest.mark.parametrize("kind", ["precise", "mfma", "tiled_bf16", "tiled_f16"])
def test_twin_and_emulation_inside_bounds(kind):
    """the stand-ins use libm's sine: the bounds hold with no v_sin allowance at all"""
    worst = {}
    for case in CASES:
        for n, v in _check_all(kind, case).items():
            if n != "old" and v > worst.get(n, (0.0, None))[0]:
                worst[n] = (v, _id(case))
    print("%s worst error / bound: %s" % (kind, ", ".join("%s %.3f (%s)" % ((n,) + worst[n]) for n in sorted(worst))))
    assert set(worst) == {"probe", "floor", "straddle", "seeded"}
    for n, (v, where) in worst.items():
        assert v <= 1.0, (kind, n, v, where)


# ------------------------------------------------------------------------------------------------ (4) planted faults
@pytest.mark.parametrize("kind", ["tiled_bf16", "tiled_f16", "mfma"])
def test_planted_faults_are_caught(kind):
    fault_cases = [c for c in CASES if (c[1], c[2]) == (9, 65)]
    missed_by_seeded, missed_by_old, lines = [], [], []
    for fault in pc.FAULTS:
        worst = {}
        for case in fault_cases:
            for n, v in _check_all(kind, case, fault=fault).items():
                worst[n] = max(worst.get(n, 0.0), v)
        caught_by = [n for n in ("probe", "floor", "straddle") if worst[n] > 1.0]
        lines.append("%-16s probe %9.3g floor %9.3g straddle %9.3g seeded %9.3g old-style %s" % (
            fault, worst["probe"], worst["floor"], worst["straddle"], worst["seeded"], "caught" if worst["old"] > 1 else "MISSED"))
        assert caught_by, "%s: planted fault %s passes every probe, floor and straddle check: %s" % (kind, fault, worst)
        if worst["seeded"] <= 1.0:
            missed_by_seeded.append(fault)
        if worst["old"] <= 1.0:
            missed_by_old.append(fault)
    msg = "%s: every planted fault is caught by a probe, floor or straddle check.\n  %s\n  the seeded per-pair bound alone misses: %s\n" \
          "  the old-style seeded comparison (exp() within 6e-3 / mean 1e-3) misses: %s" % (
              kind, "\n  ".join(lines), missed_by_seeded or "none", missed_by_old or "none")
    print(msg)
    # the gap this suite closes: the comparison the suite had lets the subtle faults through
    for fault in ("cos_shift", "dim_mat"):
        assert fault in missed_by_old, msg
