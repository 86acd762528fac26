"""Two-level softmax cases of the relation attention whose result has no tolerance, and their float64 reference (plain module,
CPU only).

Theorem.  Let, for every (head, query), the logits s_k = (q . k_k) / 8 + pos_k take two kinds of value: the SELECTED keys all
have the same logit m, with m = 0 or a power of two and |m| <= 1024, and every other key has s_k <= m - 128.  Let the number
of selected keys be a power of two between 1 and 32, V hold integers of |v| <= 64, bias_v multiples of 1/8, resid multiples of
1/4, and every product and sum below be an f32 number (`check_exact` asserts all of it in float64).  Then a correct streaming-
softmax kernel -- any tile order, any key-range split, one or two key segments, f32 / bf16 / f16 build -- computes

    out[q, 64 h + j] = mean of V[k, 64 h + j] over the selected keys of (h, q)  +  bias_v  +  resid

with NO rounding before the single conversion to the output type (round-to-nearest-even; none at all for an f32 output):
  * e^(s - m) is exactly 1 on a selected key: expf(0) in the f32 build; in the 16-bit builds m * log2(e) is exact for m = 0 or
    a power of two, fma(s, log2e, -m log2e) is exactly 0 and exp2(0) = 1 (and P is rounded to the 16-bit type anyway);
  * e^(s - m) is exactly 0 on every other key: e^-128 lies far below half the smallest f32 denormal (e^-103.97), flushed or not;
  * every running-max rescale factor alpha = e^(m_old - m_new) is therefore exactly 0 or 1.  Whatever a wave accumulated before
    it met its first selected key (partial sums with inexact weights: finite, because every operand is) is wiped by alpha = 0;
  * the row sum l is the number of selected keys, a power of two: 1 / l and o * (1 / l) are exact;
  * in the combine kernel w_s = e^(m_s - M) is exactly 0 or 1 and num / den is an exact quotient (f32 division is correctly
    rounded; the file is built without fast-math);
  * the sum of at most 32 integers of |v| <= 64, times 1 / l, plus bias_v plus resid is a multiple of 1/32 below 2^19.
So a correct kernel equals `expected` BIT FOR BIT, and a key that is dropped, doubled, taken from a neighbouring column, segment
or head, a stale alpha row, a wrong split weight or another rounding mode shows up as a wrong number in the output of every
(head, query) that selects the key concerned.  The coverage conditions of `check_exact` make sure every key index is selected
somewhere (and unselected somewhere else), and that selected sets sit in the first tile, in the last one, across a tile
boundary, across the segment seam and across a split boundary.

Three ways of selecting, each through another fetch path of the kernel:
  "qk"     by Q.K: the keys of a group share a 16-bit +-1 code in 16 of the head's 64 columns, Q holds 512 * the picked group's
           code: a match gives 8192 / 8 = 1024, one differing bit 896.  The other 48 columns of K hold small integers, Q is 0
           there.  Partition, codes and columns differ per head; the picked group per (head, query).
  "pos"    by the f32-row position term: Q = 0, K arbitrary integers, pos = 0 on the selected set and -256 elsewhere.
  "tiled"  the same logits in the 16-bit tile order [16][ceil(Nk / 32)][Nq][32] (`tile_pos`), bf16 / f16 builds only.
  "both"   Q.K and the position term together, as the production local stages use them: the code picks a group (1024), the
           position term takes -256 from half of it (768); other groups stay <= 896, so the surviving half has m = 1024 and
           nothing within 128 of it.  (16-bit builds get the term tiled, the f32 build as rows.)

What this does NOT test: graded softmax weights, i.e. the accuracy of exp, of the P rounding and of the row-sum form.  That
stays the business of the tolerance tests (test_kernels_gpu, test_multi_launch_gpu, test_edge_cases_gpu, the ring test's twin
check).  This construction proves indexing, masking, rescale and combine logic.

Geometries are the ring test's own list (imported, not copied).  A geometry is (Nq, Nk, N1), N1 = first key of the second
segment or None.
"""
from types import SimpleNamespace

import torch

from exact_conv_cases import convert
from test_attention_ring_gpu import MIXED, NKS, NQS, SPLIT, _geometries

G, DH, C, TILE = 16, 64, 1024, 32
GAP = 128.0
NAN = float("nan")
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
VARIANTS = ("qk", "pos", "tiled", "both")
# (dtype, variant, io_f32) of the GPU file: the 16-bit builds with the f32 residual stream on and off; f32 has no tiled term
COMBOS = [(F32, v, False) for v in ("qk", "pos", "both")] + \
    [(dt, v, f) for dt in (BF16, F16) for v in VARIANTS for f in (False, True)]


def combo_id(c):
    return "%s-%s-io%d" % (str(c[0])[6:], c[1], int(c[2]))


def splits(Nq, Nk, groups=G):
    """the library's rule (mega_relation_attention_splits; the GPU file asserts that the two agree)"""
    blocks = -(-Nq // 128) * groups
    s = min(-(-48 // blocks), -(-Nk // TILE) // 4, 16)
    return max(s, 1)


def split_plan(Nq, Nk):
    """-> (number of key-range splits, key tiles per split)"""
    nt = -(-Nk // TILE)
    tps = -(-nt // splits(Nq, Nk))
    return -(-nt // tps), tps


def pos_kind(variant, dtype):
    """how a case's position term reaches the kernel: None, "rows" (f32 [16][Nq][ldp]) or "tiled" (16-bit tile order)"""
    if variant == "qk":
        return None
    if variant == "pos":
        return "rows"
    if variant == "tiled":
        assert dtype != F32
        return "tiled"
    return "rows" if dtype == F32 else "tiled"


# ------------------------------------------------------------------------------------------------ the lists
def _reduced():
    """one geometry of the ring list per Nk, chosen so that N1 walks through None, 32, 64, 75 and Nk - 1 and Nq through its
    values (variants "pos" and "both" need not meet every geometry)"""
    def kind(g):
        return g[2] if g[2] in (None, 64, 75) else ("last" if g[2] == g[1] - 1 else g[2])
    out, kinds, nqs = [], set(), set()
    for Nk in reversed(NKS):
        cand = [g for g in _geometries() if g[1] == Nk]
        best = max(cand, key=lambda g: (kind(g) not in kinds, g[0] not in nqs, g[0]))
        out.append(best)
        kinds.add(kind(best))
        nqs.add(best[0])
    assert kinds >= {None, 32, 64, 75, "last"} and nqs == set(NQS), (kinds, nqs)
    return out[::-1]


def launches(variant):
    """[(name, [geometry, ...])]: one problem per launch except the mixed one"""
    if variant in ("qk", "tiled"):
        out = [("one_%d_%d_%s" % g, [g]) for g in _geometries()]
        out.append(("mixed", list(MIXED)))
        out += [("split_%d_%d_%s" % g, [g]) for g in SPLIT]
        return out
    return [("one_%d_%d_%s" % g, [g]) for g in _reduced()] + [("split_%d_%d_%s" % SPLIT[1], [SPLIT[1]])]


def all_geometries(variant):
    return list(dict.fromkeys(g for _, gs in launches(variant) for g in gs))


# ------------------------------------------------------------------------------------------------ the case builder
def _pow2floor(n):
    return 1 << (int(n).bit_length() - 1)


def _partition(Nk, kind, bounds, lo, g, avoid=()):
    """the keys 0 .. Nk-1 in groups of power-of-two size (<= 32).  kind 0: one group wholly in the last key tile, one wholly in
    the first; kind 1: one group across every boundary of `bounds` (keys b-1, b, b-2, b+1: each half of it straddles b too).
    The other keys are scattered over the remaining groups by a seeded permutation; sizes are drawn from [lo, 32]; a key of
    `avoid` (the keys that stand alone in the other partition) does not become the one left over when their number is odd."""
    used = torch.zeros(Nk, dtype=torch.bool)
    groups = []

    def take(keys):
        groups.append(torch.tensor(list(keys), dtype=torch.long))
        used[groups[-1]] = True

    nt = -(-Nk // TILE)
    if kind == 0:
        take(range(Nk - _pow2floor(min(Nk - TILE * (nt - 1), 4)), Nk))
        if nt > 1:
            take(range(0, 4))
    else:
        for b in bounds:
            if not 1 <= b < Nk or used[b - 1] or used[b]:
                continue
            extra = [k for k in (b - 2, b + 1) if 0 <= k < Nk and not used[k]]
            take([b - 1, b] + extra if len(extra) == 2 else [b - 1, b])
    rest = (~used).nonzero().flatten()
    rest = rest[torch.randperm(rest.numel(), generator=g)]
    if rest.numel() > 1 and int(rest[-1]) in avoid:
        rest = rest.roll(1)
    i = 0
    while i < rest.numel():
        rem = rest.numel() - i
        cand = [s for s in (1, 2, 4, 8, 16, 32) if lo <= s <= rem] or [_pow2floor(rem)]
        s = cand[int(torch.randint(len(cand), (1,), generator=g))]
        take(rest[i:i + s].tolist())
        i += s
    return groups


def make_case(Nq, Nk, N1, variant):
    """All tensors float64 (every value is exact in f32, bf16 and f16): q [Nq, 1024], k [Nk, 1024], v [Nk, 1024] (V^T is what
    the kernel reads), pos [16, Nq, Nk] or None, bias_v [1024], resid [Nq, 1024]; sel [16, Nq, Nk] the intended selection."""
    assert variant in VARIANTS
    g = torch.Generator().manual_seed((Nq * 7919 + Nk * 31 + (N1 or 0)) * 4 + VARIANTS.index(variant))
    nsplit, tps = split_plan(Nq, Nk)
    nt = -(-Nk // TILE)
    bounds = sorted(set(([TILE, TILE * (nt - 1)] if nt > 1 else []) + ([N1] if N1 else []) +
                        [s * tps * TILE for s in range(1, nsplit)]))
    passes = 2 if variant == "both" else 1         # "both": every group is picked with either half removed
    picks = Nq * (G // 2)                          # (head, query) pairs per partition
    gid = torch.zeros((2, Nk), dtype=torch.long)
    rank = torch.zeros((2, Nk), dtype=torch.long)
    sizes, codes, parts = [], [], []
    for p in range(2):
        lo = 2                                     # (a key that only ever stands alone would hide being counted twice)
        while True:
            alone = [int(ks[0]) for ks in parts[0] if ks.numel() == 1] if p else []
            gs = _partition(Nk, p, bounds, lo, g, alone)
            if len(gs) * passes <= picks and len(gs) >= 2:
                break
            lo *= 2
            assert lo <= 32, "no partition of %d keys with every group picked by %d (head, query) pairs" % (Nk, picks)
        parts.append(gs)
        for i, ks in enumerate(gs):
            gid[p, ks] = i
            rank[p, ks] = torch.arange(ks.numel())
        sizes.append(torch.tensor([ks.numel() for ks in gs]))
        bits = torch.randperm(65536, generator=g)[:len(gs)]            # distinct 16-bit codes
        codes.append((((bits[:, None] >> torch.arange(16)) & 1) * 2 - 1).double())
    # the 16 code columns of each head: the first four heads partition the 64 columns, the others draw their own subset
    cover = torch.randperm(DH, generator=g)
    cols = [cover[16 * h:16 * h + 16] if h < 4 else torch.randperm(DH, generator=g)[:16] for h in range(G)]
    cols = torch.stack([c.sort().values for c in cols])

    pick = torch.zeros((Nq, G), dtype=torch.long)
    half = torch.zeros((Nq, G), dtype=torch.long)
    order = [torch.randperm(len(parts[p]), generator=g) for p in range(2)]
    qi = torch.arange(Nq)
    for h in range(G):
        p = h % 2
        i = qi * (G // 2) + h // 2
        pick[:, h] = order[p][i % len(parts[p])]
        half[:, h] = (i // len(parts[p])) % 2
    sel = torch.zeros((G, Nq, Nk), dtype=torch.bool)
    ingroup = torch.zeros((G, Nq, Nk), dtype=torch.bool)
    for h in range(G):
        p = h % 2
        ingroup[h] = gid[p][None, :] == pick[:, h, None]
        if variant == "both":                     # groups of 4 and more lose one half to the position term
            sz = sizes[p][gid[p]]
            first = rank[p] < sz // 2
            keep = (sz < 4)[None, :] | (first[None, :] == (half[:, h, None] == 0))
            sel[h] = ingroup[h] & keep
        else:
            sel[h] = ingroup[h]

    k = torch.randint(-4, 5, (Nk, C), generator=g).double()
    q = torch.zeros((Nq, C), dtype=torch.float64)
    if variant in ("qk", "both"):
        for h in range(G):
            p = h % 2
            k[:, h * DH + cols[h]] = codes[p][gid[p]]
            q[:, h * DH + cols[h]] = 512.0 * codes[p][pick[:, h]]
    pos = None
    if variant in ("pos", "tiled"):
        pos = torch.where(sel, 0.0, -256.0).double()
    elif variant == "both":
        noise = torch.rand((G, Nq, Nk), generator=g) < 0.5
        pos = torch.where(sel | (noise & ~ingroup), 0.0, -256.0).double()
    v = torch.randint(-64, 65, (Nk, C), generator=g).double()
    bias_v = torch.randint(-32, 33, (C,), generator=g).double() / 8
    resid = torch.randint(-127, 128, (Nq, C), generator=g).double() / 4
    return SimpleNamespace(Nq=Nq, Nk=Nk, N1=N1, variant=variant, q=q, k=k, v=v, pos=pos, bias_v=bias_v, resid=resid, sel=sel,
                           cols=cols, nsplit=nsplit, tps=tps)


_CASES = {}


def case_for(geom, variant):
    """make_case, built once per process and never modified.  "pos" and "tiled" share their cases: the same logits"""
    key = (tuple(geom), variant)
    if key not in _CASES and variant == "tiled":
        _CASES[key] = SimpleNamespace(**dict(vars(case_for(geom, "pos")), variant="tiled"))      # (the same tensors)
    elif key not in _CASES:
        _CASES[key] = make_case(geom[0], geom[1], geom[2], variant)
    return _CASES[key]


_CHECKED = {}


def checked_case(geom, variant):
    """case_for, with check_exact asserted once per process: a case that misses a condition is not handed out"""
    key = (tuple(geom), variant)
    if key not in _CHECKED:
        _CHECKED[key] = check_exact(case_for(geom, variant))
    return case_for(geom, variant)


# ------------------------------------------------------------------------------------------------ float64 truth
def _heads(x):
    """[N, 1024] -> [16, N, 64]"""
    return x.view(x.shape[0], G, DH).permute(1, 0, 2)


def logits(case):
    s = torch.bmm(_heads(case.q), _heads(case.k).transpose(1, 2)) / 8.0
    return s if case.pos is None else s + case.pos


def selected(case):
    s = logits(case)
    return s == s.max(dim=2, keepdim=True).values


def pre_conversion(case, sel=None):
    """float64 [Nq, 1024]: mean of V over the selected keys + bias_v + resid"""
    sel = case.sel if sel is None else sel
    o = torch.bmm(sel.double(), _heads(case.v)) / sel.sum(dim=2, keepdim=True).double()
    return o.permute(1, 0, 2).reshape(case.Nq, C) + case.bias_v + case.resid


def out_dtype(dtype, io_f32):
    return F32 if io_f32 else dtype


def expected(case, odt, trunc=False):
    return convert(pre_conversion(case), odt, trunc)


def softmax_f64(case):
    p = torch.softmax(logits(case), dim=2)
    return torch.bmm(p, _heads(case.v)).permute(1, 0, 2).reshape(case.Nq, C) + case.bias_v + case.resid


def _is_pow2(t):
    t = t.double()
    return (t > 0) & (torch.log2(t.clamp(min=1e-300)) == torch.log2(t.clamp(min=1e-300)).round())


def check_exact(case):
    """asserts the conditions of the theorem and the coverage conditions, in float64.  -> dict of figures"""
    Nq, Nk, N1 = case.Nq, case.Nk, case.N1
    s = logits(case)
    m = s.max(dim=2).values
    assert bool(((m == 0) | (_is_pow2(m.abs()) & (m.abs() <= 1024))).all()), "a row maximum is neither 0 nor a power of two"
    sel = s == m[:, :, None]
    assert torch.equal(sel, case.sel), "the logits select other keys than intended"
    gap = (m[:, :, None] - s)[~sel]
    assert gap.numel() and float(gap.min()) >= GAP, "an unselected logit within %g of the maximum" % GAP
    cnt = sel.sum(dim=2)
    assert bool((_is_pow2(cnt) & (cnt <= 32)).all()), "a selected count is no power of two <= 32"
    # every product and sum is an f32 number (and every operand a bf16 and an f16 one)
    for t, unit, top in ((case.q, 512.0, 512.0), (case.k, 1.0, 4.0), (case.v, 1.0, 64.0), (case.bias_v, 0.125, 4.0),
                         (case.resid, 0.25, 31.75)):
        assert torch.equal(t / unit, (t / unit).round()) and float(t.abs().max()) <= top
        for dt in (BF16, F16):
            assert torch.equal(t.to(dt).double(), t)
    if case.pos is not None:
        assert bool(((case.pos == 0) | (case.pos == -256)).all())
    dot = float(torch.bmm(_heads(case.q).abs(), _heads(case.k).abs().transpose(1, 2)).max())
    assert dot < 2 ** 24 and float(s.abs().max()) < 2 ** 24 and torch.equal(s, s.round())
    pre = pre_conversion(case)
    assert torch.equal(pre * 32, (pre * 32).round()) and (32 * 64 + float((case.bias_v.abs().max() + case.resid.abs().max()) * 32)) < 2 ** 24
    assert torch.equal(pre.float().double(), pre)
    # coverage
    assert bool(sel.any(dim=0).any(dim=0).all()), "a key index that no (head, query) selects"
    assert bool((~sel).any(dim=0).any(dim=0).all()), "a key index that every (head, query) selects"
    assert bool((sel & (cnt >= 2)[:, :, None]).any(dim=0).any(dim=0).all()), \
        "a key index selected only where it stands alone (counting it twice would not change that mean)"
    keys = torch.arange(Nk)
    kmin = torch.where(sel, keys, Nk).amin(dim=2)
    kmax = torch.where(sel, keys, -1).amax(dim=2)
    nt = -(-Nk // TILE)
    assert bool((kmin >= TILE * (nt - 1)).any()), "no selected set wholly in the last key tile"
    assert bool((kmax < TILE).any()), "no selected set wholly in the first key tile"
    if nt > 1:
        b = torch.arange(1, nt) * TILE
        assert bool((sel[:, :, b - 1] & sel[:, :, b]).any()), "no selected set with adjacent keys across a tile boundary"
    if N1 is not None:
        assert bool((sel[:, :, N1 - 1] & sel[:, :, N1]).any()), "no selected set across the seam"
    if case.nsplit > 1:
        per = torch.stack([sel[:, :, s_ * case.tps * TILE:(s_ + 1) * case.tps * TILE].any(dim=2) for s_ in range(case.nsplit)])
        assert bool((~per).any(dim=0).any()), "no (head, query) with a split that holds none of its keys"
        assert bool((per.sum(dim=0) >= 2).any()), "no selected set that spans two splits"
        b = torch.arange(1, case.nsplit) * case.tps * TILE
        assert bool((sel[:, :, b - 1] & sel[:, :, b]).any())
    if case.variant in ("qk", "both"):
        used = torch.zeros(DH, dtype=torch.bool)
        for h in range(G):
            used[case.cols[h]] = True
        assert bool(used.all()) and len({tuple(c.tolist()) for c in case.cols}) == G
    return {"gap": float(gap.min()), "counts": sorted(set(cnt.flatten().tolist())), "m": sorted(set(m.flatten().tolist()))}


# ------------------------------------------------------------------------------------------------ layouts
def tile_pos(pos, dtype, fill=NAN):
    """[16, Nq, Nk] logits -> the attention kernel's tile order [16][ceil(Nk / 32)][Nq][32] in `dtype`: the 32 keys of a tile
    are stored (h2, rq, e) with key = 8 rq + 4 h2 + e.  Slots of keys past Nk hold `fill`."""
    Gh, Nq, Nk = pos.shape
    nt = -(-Nk // TILE)
    out = torch.full((Gh, nt, Nq, TILE), fill, dtype=torch.float64)
    for kt in range(nt):
        for h2 in range(2):
            for rq in range(4):
                for e in range(4):
                    key = TILE * kt + 8 * rq + 4 * h2 + e
                    if key < Nk:
                        out[:, kt, :, 16 * h2 + 4 * rq + e] = pos[:, :, key]
    return out.to(dtype).contiguous()


def item_for(case, dtype, io_f32, dev="cpu", fill=NAN):
    """The case as an item of ops.relation_attention_batched.  Every buffer is wider than what the kernel may read and filled
    with NaN around it: pad columns of V^T past Nk, pad columns of the position rows, tail slots of the last position tile, the
    rows around K, and -- with two segments, in the ring test's layout (second V^T block 16-byte aligned when N1 == 64, at an
    odd element otherwise) -- the filler columns and rows around both views.  Keys starting with "_" are for the CPU twin."""
    Nq, Nk, N1 = case.Nq, case.Nk, case.N1
    sdt = out_dtype(dtype, io_f32)
    kfull, vfull = case.k.to(dtype), case.v.t().contiguous().to(dtype)
    kind = pos_kind(case.variant, dtype)
    ld = -(-Nk // TILE) * TILE
    pos = None
    if kind == "rows":
        pos = torch.full((G, Nq, ld + TILE), fill, dtype=F32)      # (a pitch wider than ceil32(Nk): poison at aligned Nk too)
        pos[:, :, :Nk] = case.pos.float()
        assert bool(pos[:, :, Nk:].isnan().all())
    elif kind == "tiled":
        pos = tile_pos(case.pos, dtype, fill)
        assert ld == Nk or bool(pos.isnan().any())
    item = {"q": case.q.to(dtype).to(dev), "Nk": Nk, "resid": case.resid.to(sdt).to(dev), "bias_v": case.bias_v.float().to(dev),
            "pos": None if pos is None else pos.to(dev)}
    if N1 is None:
        vt = torch.full((C, ld + 8), fill, dtype=dtype)
        vt[:, :Nk] = vfull
        kb = torch.full((2 + Nk + 1, C), fill, dtype=dtype)
        kb[2:2 + Nk] = kfull
        item.update(k=kb.to(dev)[2:2 + Nk], vt=vt.to(dev))
        return item
    N2 = Nk - N1
    b_cols, w2 = (8, (8 + N2 + 15) // 8 * 8) if N1 == 64 else (5, 5 + N2 + 11)
    big1 = torch.full((C, (8 + N1 + 16) // 8 * 8), fill, dtype=dtype)
    big1[:, 8:8 + N1] = vfull[:, :N1]
    big2 = torch.full((C, w2), fill, dtype=dtype)
    big2[:, b_cols:b_cols + N2] = vfull[:, N1:]
    kb1 = torch.full((2 + N1 + 1, C), fill, dtype=dtype)
    kb1[2:2 + N1] = kfull[:N1]
    kb2 = torch.full((1 + N2 + 3, C), fill, dtype=dtype)
    kb2[1:1 + N2] = kfull[N1:]
    big1, big2, kb1, kb2 = big1.to(dev), big2.to(dev), kb1.to(dev), kb2.to(dev)
    item.update(k=kb1[2:2 + N1], vt=big1[:, 8:8 + N1], N1=N1, k2=kb2[1:1 + N2], vt2=big2[:, b_cols:b_cols + N2],
                _vt_wide=big1[:, 8:])
    if N1 == 64:
        assert item["vt2"].data_ptr() % 16 == 0 and (big2.stride(0) * big2.element_size()) % 16 == 0
    else:
        assert item["vt2"].data_ptr() % 16 != 0
    return item


# ------------------------------------------------------------------------------------------------ the comparison
def describe_mismatch(case, got, want, what):
    """None when got equals want; otherwise the first wrong (query, head, column), the keys selected there and where they lie"""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.dtype != want.dtype or got.shape != want.shape:
        return "%s: %s %s against %s %s" % (what, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
    if torch.equal(got, want):
        return None
    diff = ~(got == want)                            # (a NaN differs from everything)
    qi, c = (int(x) for x in diff.nonzero()[0])
    h = c // DH
    ks = case.sel[h, qi].nonzero().flatten().tolist()
    where = ["tiles %s of %d" % (sorted({k // TILE for k in ks}), -(-case.Nk // TILE))]
    if case.N1 is not None:
        where.append("segments %s (N1 = %d)" % (sorted({int(k >= case.N1) for k in ks}), case.N1))
    if case.nsplit > 1:
        where.append("splits %s of %d" % (sorted({k // (case.tps * TILE) for k in ks}), case.nsplit))
    return ("%s (%d x %d, N1 %s, %s): %d of %d elements differ, %d rows, %d heads; first at query %d (wave %d of its block), head %d, "
            "column %d: got %r, want %r; selected keys %s: %s" % (
                what, case.Nq, case.Nk, case.N1, case.variant, int(diff.sum()), diff.numel(), int(diff.any(dim=1).sum()),
                int(diff.view(case.Nq, G, DH).any(dim=2).any(dim=0).sum()), qi, qi % 128 // 32, h, c % DH, float(got[qi, c]),
                float(want[qi, c]), ks, ", ".join(where)))


# ------------------------------------------------------------------------------------------------ single-key faults, in closed form
def key_fault_rows(case, kind):
    """For every key j, one (head, query) that selects j and the float64 value its 64 outputs take when key j is dropped
    (kind "drop": the mean over the others; 0 / 0 when j stands alone) or counted twice ("double").
    -> (head [Nk], query [Nk], faulted [Nk, 64], true [Nk, 64])"""
    Nk = case.Nk
    flat = case.sel.view(G * case.Nq, Nk) * case.sel.sum(dim=2).view(G * case.Nq, 1)
    first = flat.argmax(dim=0)                  # the largest set with j in it (check_exact: one of two keys or more exists)
    h, qi = first // case.Nq, first % case.Nq
    vh = _heads(case.v)                                         # [16, Nk, 64]
    rows = case.sel[h, qi].double()                             # [Nk(j), Nk]
    tot = torch.zeros((Nk, DH), dtype=torch.float64)
    for hh in range(G):
        js = (h == hh).nonzero().flatten()
        tot[js] = rows[js] @ vh[hh]
    cnt = rows.sum(dim=1, keepdim=True)
    vj = vh[h, torch.arange(Nk)]
    add = case.bias_v.view(G, DH)[h] + case.resid.view(case.Nq, G, DH)[qi, h]
    sign = -1.0 if kind == "drop" else 1.0
    return h, qi, (tot + sign * vj) / (cnt + sign) + add, tot / cnt + add
