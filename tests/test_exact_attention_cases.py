"""The two-level softmax cases of tests/exact_attention_cases.py, checked on the CPU before the GPU file trusts them:
(1) every listed case meets the conditions of the theorem and the coverage conditions (check_exact), and the CPU twin of the
kernel (cpu_ops.relation_attention, f32 / bf16 / f16) and a float64 softmax both equal the expected output bit for bit;
(2) a small tile-loop twin -- 32-key tiles, running max, alpha rescale, optional key-range split with combine, optional seam,
reading the very item the GPU gets, NaN fillers included -- is bit-exact when unfaulted; (3) every planted fault makes the
comparison fail on at least one listed geometry, and a dropped or doubled key does so for EVERY key index at EVERY geometry.
Each test prints its figures (run with -s to see them)."""
import pytest
import torch

import cpu_ops
import exact_attention_cases as xa
from exact_conv_cases import convert, rounding_shares

F32, BF16, F16 = xa.F32, xa.BF16, xa.F16
G, DH, C, TILE = xa.G, xa.DH, xa.C, xa.TILE
# "tiled" runs the position-selected cases at EVERY geometry (a "tiled" case is the "pos" case of its geometry: the same
# tensors, another layout of the term), so the "pos" family here is that full list, of which all_geometries("pos") is a part
assert set(xa.all_geometries("pos")) <= set(xa.all_geometries("tiled"))
CASE_KEYS = [(g, v) for v in ("qk", "pos") for g in xa.all_geometries("tiled" if v == "pos" else v)] + \
    [(g, "both") for g in xa.all_geometries("both")]


def _id(key):
    return "%dx%d-%s-%s" % (key[0] + (key[1],))


# ------------------------------------------------------------------------------------------------ (1) the cases
@pytest.mark.parametrize("key", CASE_KEYS, ids=_id)
def test_case_is_exact_and_references_agree(key):
    geom, variant = key
    case = xa.case_for(geom, variant)
    fig = xa.check_exact(case)
    pre = xa.pre_conversion(case)
    soft = xa.softmax_f64(case)
    for dt in (F32, BF16, F16):
        for io_f32 in ((False,) if dt == F32 else (False, True)):
            odt = xa.out_dtype(dt, io_f32)
            want = xa.expected(case, odt)
            assert torch.equal(soft.to(odt), want), "the float64 softmax differs"
            ld = -(-case.Nk // TILE) * TILE
            vt = torch.full((C, ld), xa.NAN, dtype=dt)
            vt[:, :case.Nk] = case.v.t().to(dt)
            got = cpu_ops.relation_attention(case.q.to(dt), case.k.to(dt), vt, case.Nk,
                                             pos=None if case.pos is None else case.pos.float(), resid=case.resid.to(odt),
                                             bias_v=case.bias_v.float())
            assert got.dtype == odt and torch.equal(got, want), "cpu_ops.relation_attention differs (%s, io_f32 %d)" % (dt, io_f32)
    r16 = [rounding_shares(pre, dt) for dt in (BF16, F16)]
    print("%s: m %s, counts %s, gap %g, splits %d; outputs rounded bf16 %.0f %% (ties %.1f %%), f16 %.0f %% (ties %.1f %%)" % (
        _id(key), fig["m"], fig["counts"], fig["gap"], case.nsplit, 100 * r16[0][0], 100 * r16[0][1], 100 * r16[1][0], 100 * r16[1][1]))
    assert r16[0][0] > 0 and r16[0][1] > 0, "the bf16 output conversion never rounds / never meets a tie on this case"


def test_lists():
    """the lists are the ring test's; the variants that need every geometry get every geometry"""
    import test_attention_ring_gpu as ring
    for v in ("qk", "tiled"):
        names = [g for _, gs in xa.launches(v) for g in gs]
        assert names == ring._geometries() + ring.MIXED + ring.SPLIT
    for v in ("pos", "both"):
        gs = xa.all_geometries(v)
        assert {g[1] for g in gs} >= set(ring.NKS) and set(gs) <= set(ring._geometries() + ring.SPLIT)
    for g in ring.SPLIT:
        assert xa.splits(g[0], g[1]) > 1 and xa.split_plan(g[0], g[1])[0] > 1
    assert all(xa.splits(*g[:2]) == 1 for g in ring._geometries())


def test_tiler_against_the_ring_tests_inverse():
    """tile_pos, written from the layout comment in relation.hip (key = 8 rq + 4 h2 + e, stored (h2, rq, e)), is undone by the
    view / permute the ring test applies to the position kernel's own output"""
    Nq, Nk = 5, 97
    pos = torch.arange(G * Nq * Nk, dtype=torch.float64).view(G, Nq, Nk) % 251
    t = xa.tile_pos(pos, F16, fill=-1.0).double()
    nt = -(-Nk // TILE)
    back = t.view(G, nt, Nq, 2, 4, 4).permute(0, 2, 1, 4, 3, 5).reshape(G, Nq, nt * TILE)
    assert torch.equal(back[:, :, :Nk], pos) and bool((back[:, :, Nk:] == -1).all())
    # one element by hand: tile 1, rq 2, h2 1, e 3 -> key 32 + 16 + 4 + 3 = 55, slot 16 + 8 + 3 = 27
    assert torch.equal(t[:, 1, :, 27], pos[:, :, 55])


# ------------------------------------------------------------------------------------------------ (2) the tile-loop twin
FAULTS = ("mask_minus", "mask_plus", "alpha_row", "seam", "w_one", "next_head", "pos_shift", "tile_swap", "bias_col", "rows",
          "trunc")


def tile_twin(item, case, io_f32, fault=None, key=None):
    """Streaming softmax over 32-key tiles in f32, from the algorithm: per (head, query) a running max m, a running sum l and
    an un-normalised output O; every tile rescales l and O by alpha = e^(m_old - m_new).  With a split, every key range keeps
    its own (m, l, O) and a combine weights them by e^(m_s - max m).  Reads `item` as the kernel would: two K / V^T segments
    where it has them, fetched slots past Nk as they lie in the buffers (rows of K past the end read as zeros), the
    position term as rows or in tile order.  fault / key: a planted fault (FAULTS, or "drop" / "double" of key index `key`)."""
    Nq, Nk, N1 = case.Nq, case.Nk, case.N1
    dt = item["q"].dtype
    nt = -(-Nk // TILE)
    W = nt * TILE
    # ---- fetch: K [W, 1024], V [W, 1024] (from V^T), position term [16, Nq, W]
    K = torch.zeros((W, C))
    V = torch.zeros((W, C))
    if N1 is None:
        K[:Nk] = item["k"][:Nk].float()
        V[:] = item["vt"][:, :W].float().t()
    else:
        K[:N1], K[N1:Nk] = item["k"].float(), item["k2"].float()
        w2 = min(W - N1, item["vt2"].shape[1])
        V[:N1] = item["vt"].float().t()
        V[N1:N1 + w2] = item["vt2"][:, :w2].float().t()
        if fault == "seam":                     # key N1 from the column after the first segment's last: a filler column,
            # so this fault is caught through the item's NaN poison (as is "mask_plus": slot Nk of the position term)
            V[N1] = item["_vt_wide"][:, N1].float()
    V[Nk:] = 0                                  # the kernel zeroes the tail keys of V^T
    P = torch.zeros((G, Nq, W))
    pos = item.get("pos")
    if pos is not None and pos.dim() == 3:
        P = pos.float().clone()
    elif pos is not None:
        for kt in range(nt):
            for h2 in range(2):
                for rq in range(4):
                    for e in range(4):
                        slot = 8 * rq + 4 * h2 + e if fault == "tile_swap" else 16 * h2 + 4 * rq + e
                        P[:, :, TILE * kt + 8 * rq + 4 * h2 + e] = pos[:, kt, :, slot].float()
    if fault == "pos_shift":
        P = torch.roll(P, -1, dims=2)
    qh = item["q"].float().view(Nq, G, DH).permute(1, 0, 2)
    Kh = K.view(W, G, DH).permute(1, 0, 2)
    Vh = V.view(W, G, DH).permute(1, 0, 2)
    nk_mask = Nk + {"mask_minus": -1, "mask_plus": 1}.get(fault, 0)
    keys = torch.arange(W)
    # ---- the tile loop, per key-range split
    parts = []
    for s in range(case.nsplit):
        m = torch.full((G, Nq), -float("inf"))
        l = torch.zeros((G, Nq))
        O = torch.zeros((G, Nq, DH))
        for t in range(s * case.tps, min(nt, (s + 1) * case.tps)):
            sl = slice(TILE * t, TILE * t + TILE)
            S = torch.bmm(qh, Kh[:, sl].transpose(1, 2)) * 0.125 + P[:, :, sl]
            S[:, :, keys[sl] >= nk_mask] = -float("inf")
            if fault == "drop" and TILE * t <= key < TILE * t + TILE:
                S[:, :, key - TILE * t] = -float("inf")
            m_new = torch.maximum(m, S.max(dim=2).values)
            alpha = torch.exp(m - m_new)
            p = torch.exp(S - m_new[:, :, None])
            if dt != F32:
                p = p.to(dt).float()            # P reaches the PV product rounded; the row sum is over the rounded values
            if fault == "double" and TILE * t <= key < TILE * t + TILE:
                p[:, :, key - TILE * t] *= 2
            l = l * alpha + p.sum(dim=2)
            a_o = torch.roll(alpha, 4, dims=1) if fault == "alpha_row" else alpha
            O = O * a_o[:, :, None] + torch.bmm(p, Vh[:, sl])
            m = m_new
        parts.append((m, l, O))
    if case.nsplit == 1:
        m, l, O = parts[0]
        o = O * (1.0 / l)[:, :, None]
    else:
        ms, ls = torch.stack([p_[0] for p_ in parts]), torch.stack([p_[1] for p_ in parts])
        if fault == "next_head":
            ms, ls = torch.roll(ms, -1, dims=1), torch.roll(ls, -1, dims=1)
        w = torch.exp(ms - ms.max(dim=0).values)
        if fault == "w_one":
            w = torch.ones_like(w)
        num = sum(w[i][:, :, None] * parts[i][2] for i in range(case.nsplit))
        o = num / (w * ls).sum(dim=0)[:, :, None]
    bias = item["bias_v"].float()
    out = o.permute(1, 0, 2).reshape(Nq, C) + (torch.roll(bias, 1) if fault == "bias_col" else bias) + item["resid"].float()
    if fault == "rows":                         # the rows of a partial last wave are never written
        out[Nq // 32 * 32:] = 0
    return convert(out.double(), xa.out_dtype(dt, io_f32), trunc=fault == "trunc")


@pytest.mark.parametrize("combo", xa.COMBOS, ids=xa.combo_id)
def test_tile_twin_is_exact(combo):
    dt, variant, io_f32 = combo
    for geom in xa.all_geometries(variant):
        case = xa.case_for(geom, variant)
        item = xa.item_for(case, dt, io_f32)
        want = xa.expected(case, xa.out_dtype(dt, io_f32))
        msg = xa.describe_mismatch(case, tile_twin(item, case, io_f32), want, "tile twin")
        assert msg is None, msg


# ------------------------------------------------------------------------------------------------ (3) planted faults
# where each fault is looked for: (dtype, variant, io_f32, geometries); the first geometry that shows it ends the search.
# "seam" and "mask_plus" rest on the NaN poison of the item (the wrongly fetched column / slot is a filler): with "qk" and the
# zero rows the kernel reads for K past the end, an extra key Nk would have logit 0 and go unnoticed, hence "tiled" there.
_SEAMS = [(35, 129, 75), (300, 97, 96), (300, 128, 64), (300, 96, 32)]
_WHERE = {
    "mask_minus": (BF16, "qk", False, [(3, 31, None), (35, 33, None), (129, 97, 75)]),
    "mask_plus": (F16, "tiled", False, [(3, 31, None), (35, 33, None), (129, 97, 75)]),
    "alpha_row": (F32, "qk", False, [(35, 129, 75), (300, 129, 75)]),
    "seam": (BF16, "qk", True, _SEAMS),
    "w_one": (F32, "qk", False, list(xa.SPLIT)),
    "next_head": (BF16, "tiled", False, list(xa.SPLIT)),
    "pos_shift": (F32, "pos", False, None),
    "tile_swap": (BF16, "tiled", True, [(3, 31, None), (129, 129, 32)]),
    "bias_col": (F16, "qk", True, [(3, 31, None)]),
    "rows": (BF16, "qk", False, [(35, 33, None), (129, 97, 75)]),
    "trunc": (BF16, "both", False, None),
}


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_is_caught(fault):
    dt, variant, io_f32, geoms = _WHERE[fault]
    geoms = geoms or xa.all_geometries(variant)
    assert geoms and all(g in xa.all_geometries(variant) for g in geoms), "a geometry that is not in the list"
    caught = []
    for geom in geoms:
        case = xa.case_for(geom, variant)
        item = xa.item_for(case, dt, io_f32)
        want = xa.expected(case, xa.out_dtype(dt, io_f32))
        assert xa.describe_mismatch(case, tile_twin(item, case, io_f32), want, "unfaulted") is None
        msg = xa.describe_mismatch(case, tile_twin(item, case, io_f32, fault=fault), want, fault)
        if msg is not None:
            caught.append(geom)
            print(msg)
    print("%s: caught at %d of %d geometries" % (fault, len(caught), len(geoms)))
    assert caught, "%s passes the comparison on %s" % (fault, geoms)


@pytest.mark.parametrize("key", CASE_KEYS, ids=_id)
def test_every_dropped_or_doubled_key_is_caught(key):
    """in closed form, for every key index j of the case: the 64 outputs of a (head, query) that selects j differ, after the
    conversion to EVERY output type, when j is dropped or counted twice.  (The closed form is tied to the tile-loop twin below:
    on the small geometries the twin itself drops and doubles every j.)"""
    geom, variant = key
    case = xa.case_for(geom, variant)
    for kind in ("drop", "double"):
        h, qi, bad, true = xa.key_fault_rows(case, kind)
        assert torch.equal(true, xa.pre_conversion(case).view(case.Nq, G, DH)[qi, h])
        for odt in (F32, BF16, F16):
            same = (bad.to(odt) == true.to(odt)).all(dim=1)              # (NaN -- the mean of no key -- differs)
            assert not bool(same.any()), "%s of key %s leaves the %s output as it is" % (kind, same.nonzero().flatten().tolist(), odt)


@pytest.mark.parametrize("geom,variant,dt", [((35, 129, 75), "qk", BF16), ((3, 31, None), "tiled", F16), ((40, 1500, 75), "qk", F32),
                                             ((129, 97, 75), "both", F32)], ids=lambda v: str(v).replace("torch.", ""))
def test_closed_form_key_faults_are_the_twins(geom, variant, dt):
    """the closed form above is what the tile-loop twin computes when it drops / doubles a key: first key, last key, the keys at
    the seam and at the first tile boundary"""
    case = xa.case_for(geom, variant)
    item = xa.item_for(case, dt, False)
    want = xa.expected(case, dt)
    js = sorted({0, case.Nk - 1, min(TILE, case.Nk - 1), min(TILE, case.Nk) - 1} | ({case.N1 - 1, case.N1} if case.N1 else set()))
    eps = torch.finfo(dt).eps                  # (a mean over 2^n +- 1 keys is no dyadic number: the twin's O * (1 / l) rounds)
    for kind in ("drop", "double"):
        h, qi, bad, _ = xa.key_fault_rows(case, kind)
        for j in js:
            got = tile_twin(item, case, False, fault=kind, key=j)
            row = got.view(case.Nq, G, DH)[qi[j], h[j]]
            ref = bad[j]
            if not bool(ref.isnan().any()):          # (a lone key dropped: 0 / 0 in closed form, the next-best keys in the twin)
                assert torch.allclose(row.double(), ref, rtol=2 * eps, atol=128 * eps)
            assert not torch.equal(got, want)
            # and only the (head, query) pairs that select j change
            changed = ~(got == want).view(case.Nq, G, DH).all(dim=2).t()          # [16, Nq]
            assert not bool((changed & ~case.sel[:, :, j]).any())


_SMALL = [g for g in xa.all_geometries("qk") if g[0] <= 35]
_SMALL_KEYS = [(g, v, (F32, BF16, F16)[(i + n) % 3] if v == "qk" else (BF16, F16)[(i + n) % 2])
               for n, v in enumerate(("qk", "tiled")) for i, g in enumerate(_SMALL)]


@pytest.mark.parametrize("geom,variant,dt", _SMALL_KEYS, ids=lambda v: str(v).replace("torch.", ""))
def test_twin_catches_every_dropped_or_doubled_key(geom, variant, dt):
    """the fault itself, planted into the tile-loop twin for EVERY key index j of the geometries with Nq <= 35 (every Nk, with
    and without a seam): the comparison fails, in the rows of the (head, query) pairs that select j and nowhere else"""
    case = xa.case_for(geom, variant)
    item = xa.item_for(case, dt, False)
    want = xa.expected(case, dt)
    for kind in ("drop", "double"):
        for j in range(case.Nk):
            got = tile_twin(item, case, False, fault=kind, key=j)
            changed = ~(got == want).view(case.Nq, G, DH).all(dim=2).t()
            assert bool(changed.any()), "%s of key %d passes the comparison" % (kind, j)
            assert not bool((changed & ~case.sel[:, :, j]).any())
