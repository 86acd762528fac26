"""Box sets, probe weights, float64 references and DERIVED error bounds for the position term of the relation module,
w[h,q,k] = log(relu(Wg_h . pe(q,k) + bg_h) + 1e-6) (csrc/relation.hip: pos_logits_kernel<true> / <false>,
pos_logits_mfma_kernel, pos_logits_tiled_batched_kernel<bf16_t> / <f16_t>).  CPU only: numpy, torch, the oracle.
tests/test_position_cases.py proves the facts claimed here and that the checks reject planted faults;
tests/test_position_gpu.py runs the five kernels.

Why lattices and probes.  On real-valued boxes cx_q - cx_k cancels in f32 and the seeded Wg smears 64 roundings into every
logit: the f32 formula is itself 4.8e-3 from float64 there, so no bound below that can be asked of a kernel.  Here every box
has integer corners in [0, 2047]: widths are integers, centres multiples of 1/2, and widths, centres and centre differences
are exact in f32 (test_position_cases.py checks it), so the kernels and float64 start from the same numbers.  With Wg one-hot
(head h reads embedding entry j = 16 r + h with weight +-1.0, bias b) the contraction is exact in every operand type and
the kernel is a readout of ONE embedding entry per head: logit = log(b +- e_j + 1e-6).

Kinds (one per kernel): "precise", "valu" (pos_logits_kernel<false>), "mfma", "tiled_bf16", "tiled_f16".

The bounds, derived from the kernels' arithmetic (u = 2^-24, half an ulp relative; |pm| <= PM_MAX = 7.2 = log 1333 + a
little, asserted for every set; e = a sine or cosine, |e| <= 1; i = frequency index, dim_i = 1000^(i/8)):

  pm, precise arithmetic (precise, valu; also the torch twin): s = |dx / w| + 1e-3f has three relative errors, the division
    (u), the sum (u) and the f32 constant (|1e-3f - 1e-3| / 1e-3 = 4.7e-8, taken against the smallest sum); they enter the
    log as absolute errors.  logf is within LOGF_ULPS = 3 ulp, ulp(7.2) = 2^-21: the OpenCL full-profile bound, which the
    device library is built to.  (Not the 1 ulp of a CPU libm: the device's logf compiles to v_log_f32 times ln 2 in extended
    precision, so it inherits the hardware logarithm's error in log2, and the first GPU run of these tests found it 2.2 ulp
    from float64 at log 918.001.  The torch twin's worst entry sits at a third of the bound.)  PM_ERR_PRECISE = 3 x 2^-21 + 2u + 4.7e-8 = 1.6e-6.
  phase, precise arithmetic: a = (pm * 100) / dim_i.  100 x the pm error, half an ulp of 720 (2^-15) from the product, and
    the division's u |a| <= u 720 / dim_i: PHASE_PRECISE = 1.6e-4 + 3.1e-5 + 4.3e-5 = 2.33e-4 rad, all of it / dim_i.
    sincosf: SINCOS_ULPS = 2 ulp of a value below 1 (2^-24 each), absolute.
    valu only: Cody-Waite.  r = a - n 2 pi in two fmas (each half an ulp of pi: 2^-23), rev = r / 2 pi with the rounded
    constant (u + 3.9e-8 of half a revolution, x 2 pi): REDUCE_ABS = 2^-22 + pi (u + 3.9e-8) = 5.5e-7, then the hardware sine.
  pm, fast arithmetic (mfma, tiled): fast_div = a * v_rcp(b), 1 ulp + half an ulp: 3u.  s: 3u + u + 4.7e-8.  fast_log =
    v_log(s) * ln2f: 1 ulp of log2(s) (|log2| <= 10.4: 2^-20) x ln 2, half an ulp of the product (2^-22), and ln2f's own
    2.8e-9 x 7.2.  PM_ERR_FAST = 6.6e-7 + 2.4e-7 + 2e-8 + 2.9e-7 = 1.21e-6.
  phase, fast arithmetic: x_rev = fma(pm, crev_i, shift), crev_i = (100 * (1 / 2 pi)f) / dim_i in f32.  crev_i's relative error
    is computed here from the same f32 operations (CREV_REL, below 3u) and costs 720 CREV_REL / dim_i rad; the fma rounds
    once, half an ulp of |x_rev| <= 114.6 / dim_i + 1/4 revolutions (2^-18 at i = 0, but NOT falling as 1 / dim_i: the 1/4
    keeps it at 2^-25 revolutions).  v_fract is exact.  PHASE_FAST_I[i] = (100 PM_ERR_FAST + 720 CREV_REL) / dim_i +
    2 pi halfulp(114.6 / dim_i + 1/4); PHASE_FAST = PHASE_FAST_I[0] = 1.87e-4, under the 2e-4 at which the derivation
    would be suspect (|x_rev| reaches 114.5 > 110 on the 1333-wide set).
  v_sin_f32: its absolute error is the one figure here that is MEASURED, not derived (the source says "~1e-6"): the excess of
    the kernels' worst probe error over the derived part on the first GPU run, against the float64 reference, doubled.
    The excess came out negative for every entry (V_SIN_EXCESS below), so V_SIN_ABS = 0: the sum of worst cases above
    already covers the hardware sine.
  16-bit rounding of the entry (mfma, tiled_bf16: 2^-8 |e|; tiled_f16: 2^-11 |e| + 2^-25 for the subnormals), applied to the
    entry the kernel has: RND (|e| + the terms above).
  readback (probes, b = 2: pre = 2 +- e in [1, 3]): one rounding of the accumulator (fma chain: 2^-23; MFMA: a whole ulp,
    2^-22, its internal rounding mode is not documented), the + 1e-6f (2^-23), and the logarithm's error times pre <= 3.
  the stored logit: log_err(kind, y) at logit y -- LOGF_READ_ULPS = 2 ulp of y for logf (what the floor set is asked to
    meet), ulp(y / ln 2) ln 2 + halfulp(y) + 2.8e-9 |y| for fast_log -- after a relative ADD_REL = u + 2.6e-9 from
    max(pre, 0) + 1e-6f.  The tiled kernels round it to 16 bits: `logit_interval` rounds the ends of the interval outwards.
  seeded Wg (`pair_bound`): sum_j |wg_j| entry_j + sum_j |wg_j - round16(wg_j)| |e_j| + 64 roundings (2^-23 each, MFMA
    included) of partial sums below |bg| + sum_j |wg_j e_j|.

Nothing above was fitted to a kernel's output except V_SIN_ABS."""
import functools
import math

import numpy as np
import torch

from oracle import mega_oracle as mo

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
KINDS = ("precise", "valu", "mfma", "tiled_bf16", "tiled_f16")
KIND_DTYPE = {"precise": None, "valu": None, "mfma": BF16, "tiled_bf16": BF16, "tiled_f16": F16}   # operand type of the MFMA
TILED = {"tiled_bf16": BF16, "tiled_f16": F16}                                                        # type of the stored logit
SHAPES = [(1, 1), (8, 64), (9, 65), (19, 130), (5, 257)]
SETS = ("lattice", "self", "concentric", "equal_size", "ratio999", "extremes", "wide1333")
LATTICE_SETS = ("lattice", "self")            # where the seeded weights run
PROBE_BIAS = 2.0
PM_MAX = 7.2


# ===================================================================================================== box sets
def _t(rows):
    return torch.tensor(np.asarray(rows, dtype=np.float64), dtype=F32).reshape(-1, 4)


def _random_lattice(rng, n, W=1000, H=600):
    x = np.sort(rng.randint(0, W, size=(n, 2)), axis=1)
    y = np.sort(rng.randint(0, H, size=(n, 2)), axis=1)
    return np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1)


def _extreme_pools(W, H, rng, n):
    """1-pixel boxes against full-canvas boxes, in both roles.  The first entries fix the small shapes: (q0, k0) = canvas
    against the corner pixel (dw = log W), (q1, k0) the same pixel twice (dx = dy = log 1e-3), (q1, k2) opposite corners
    (dx = log(W - 1 + 1e-3)), (q1, k1) pixel against canvas (dw = -log W)."""
    S = max(W, H)
    canvas, square = [0, 0, W - 1, H - 1], [0, 0, S - 1, S - 1]

    def px(x, y):
        return [x, y, x, y]
    q = [canvas, px(0, 0), px(W - 1, H - 1), square, px(W // 2, H // 2), [0, 0, W - 1, 0], px(0, H - 1), [0, 0, 0, H - 1]]
    k = [px(0, 0), canvas, px(W - 1, H - 1), px(W - 1, 0), square, px(W // 2, H // 2), [0, 0, 0, H - 1], [0, 0, W - 1, 0]]
    for pool in (q, k):
        while len(pool) < n:
            if len(pool) % 4 == 3:
                pool.append(canvas if len(pool) % 8 == 3 else square)
            else:
                pool.append(px(int(rng.randint(0, W)), int(rng.randint(0, H))))
    return q[:n], k[:n]


@functools.lru_cache(maxsize=None)
def box_set(name, Nq, Nk):
    """-> (bq [Nq, 4], bk [Nk, 4]) f32, integer corners in [0, 2047], x2 >= x1, y2 >= y1"""
    rng = np.random.RandomState(7000 + SETS.index(name) * 100 + Nq + Nk)
    if name == "lattice":            # seeded random lattice on a 1000 x 600 canvas, queries and keys drawn apart
        b = _random_lattice(rng, Nq + Nk)
        return _t(b[:Nq]), _t(b[Nq:])
    if name == "self":               # the key set contains the query set (every local stage: the proposals are among the keys)
        b = _random_lattice(rng, max(Nq, Nk))
        return _t(b[:Nq]), _t(b[:Nk])
    if name == "concentric":         # two families, centres (500, 300) and (500.5, 300.5): within one, dx = dy = log 1e-3
        def member(i):
            a, c, odd = int(rng.randint(0, 300)), int(rng.randint(0, 290)), i % 3 == 2
            return [500 - a, 300 - c, 500 + a + odd, 300 + c + odd]
        return _t([member(i) for i in range(Nq)]), _t([member(i) for i in range(Nk)])
    if name == "equal_size":         # one size at different places: dw = dh = 0 exactly
        def place(n):
            x, y = rng.randint(0, 1000 - 37, size=n), rng.randint(0, 600 - 23, size=n)
            return np.stack([x, y, x + 36, y + 22], axis=1)
        return _t(place(Nq)), _t(place(Nk))
    if name == "ratio999":           # 1000 x 1000 queries; key j's centre is 999 px from query (j % 19)'s on both axes
        q = [[i, i, i + 999, i + 999] for i in range(Nq)]
        k = [[1498 + j % 19 - j // 19, 1498 + j % 19 - j // 19, 1499 + j % 19 + j // 19, 1499 + j % 19 + j // 19] for j in range(Nk)]
        return _t(q), _t(k)
    if name == "extremes":
        q, k = _extreme_pools(1000, 600, rng, max(Nq, Nk))
        return _t(q[:Nq]), _t(k[:Nk])
    if name == "wide1333":           # |log-ratio| reaches log 1333 = 7.195: 114.5 revolutions at frequency 0
        q, k = _extreme_pools(1333, 800, rng, max(Nq, Nk))
        return _t(q[:Nq]), _t(k[:Nk])
    raise KeyError(name)


def geometry(bq, bk, dtype):
    """widths, heights, centres and the centre differences in `dtype`, the kernels' operation order"""
    q, k = bq.to(dtype), bk.to(dtype)
    wq, hq = q[:, 2] - q[:, 0] + 1, q[:, 3] - q[:, 1] + 1
    wk, hk = k[:, 2] - k[:, 0] + 1, k[:, 3] - k[:, 1] + 1
    cxq, cyq = 0.5 * (q[:, 0] + q[:, 2]), 0.5 * (q[:, 1] + q[:, 3])
    cxk, cyk = 0.5 * (k[:, 0] + k[:, 2]), 0.5 * (k[:, 1] + k[:, 3])
    return {"wq": wq, "hq": hq, "wk": wk, "hk": hk, "cxq": cxq, "cyq": cyq, "cxk": cxk, "cyk": cyk,
            "ddx": cxq[:, None] - cxk[None, :], "ddy": cyq[:, None] - cyk[None, :]}


# ===================================================================================================== weights
def dim_mat():
    return mo.dim_mat_values()


def probe_weights(r, sign, bias=PROBE_BIAS):
    """(wg_t [64, 16], bg [16]): head h reads embedding entry 16 r + h with weight `sign` (+-1.0), bias `bias`"""
    wg_t = torch.zeros((64, 16), dtype=F32)
    for h in range(16):
        wg_t[16 * r + h, h] = float(sign)
    return wg_t, torch.full((16,), float(bias), dtype=F32)


PROBES = [(r, s) for s in (1, -1) for r in range(4)]


def probed_entries(r):
    """the embedding entry head h reads in run r, [16]"""
    return torch.arange(16) + 16 * r


def embedding_from_logit(logit, bias=PROBE_BIAS, sign=1):
    """the inverse of the probe: logit = log(bias + sign e + 1e-6) -> e, in float64"""
    return float(sign) * (torch.exp(logit.double()) - 1e-6 - float(bias))


_TINY = float(np.float32(1.4e-45))
FLOOR_BIASES = torch.tensor(
    [-1.0, -0.0, 0.0, 1e-7, 1e-6, 1e-3, 0.5, 1.0, 100.0, -1e-7, -1e-6, -100.0,
     float(np.nextafter(np.float32(1e-6), np.float32(0))), float(np.nextafter(np.float32(1e-6), np.float32(1))),
     float(np.nextafter(np.float32(1), np.float32(0))), _TINY], dtype=F32)


def floor_weights():
    """Wg = 0 and 16 different biases: the logit is log(max(b, 0) + 1e-6) whatever the boxes"""
    return torch.zeros((64, 16), dtype=F32), FLOOR_BIASES.clone()


@functools.lru_cache(maxsize=None)
def seeded_weights():
    """(wg_t, bg) of the seeded model's first local relation stage (multi_launch_cases.pos_weights)"""
    import multi_launch_cases as mc
    wg_t, bg, _ = mc.pos_weights()
    return wg_t, bg


# ===================================================================================================== float64 reference
@functools.lru_cache(maxsize=None)
def reference(name, Nq, Nk):
    """-> (pm [Nq, Nk, 4], emb [Nq, Nk, 64]) float64: the oracle's extract_position_matrix / extract_position_embedding in
    double on the f32 dim_mat the kernels are given"""
    bq, bk = box_set(name, Nq, Nk)
    pm = mo.extract_position_matrix(bq.double(), bk.double())
    emb = mo.extract_position_embedding(pm)
    assert pm.dtype == torch.float64 and emb.dtype == torch.float64
    return pm, emb


def preactivation(emb, wg_t, bg):
    """Wg_h . pe + bg_h in float64: [16, Nq, Nk]"""
    return torch.einsum("qkj,jh->hqk", emb, wg_t.double()) + bg.double().view(16, 1, 1)


# ===================================================================================================== bounds
U = 2.0 ** -24
LN2 = math.log(2.0)
LN2_REL = abs(float(np.float32(LN2)) - LN2) / LN2
INV2PI = 1.0 / (2.0 * math.pi)
INV2PI_REL = abs(float(np.float32(0.15915494309189535)) - INV2PI) / INV2PI
C1E3_REL = abs(float(np.float32(1e-3)) - 1e-3) / 1e-3
C1E6_REL = abs(float(np.float32(1e-6)) - 1e-6) / 1e-6
LOGF_ULPS = 3            # logf inside the phase: the OpenCL full-profile bound (see the docstring)
SINCOS_ULPS = 2
LOGF_READ_ULPS = 2       # the last logarithm, as the floor set is asked


def ulp32(x):
    """the f32 ulp at |x| (float64 tensor or scalar)"""
    x = torch.as_tensor(x, dtype=torch.float64).abs().clamp_min(2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(x)) - 23)


def _ulp(x):
    return float(ulp32(x))


DIM = dim_mat().double()                                   # the f32 values of 1000^(i/8)
XREV_MAX = 100.0 * PM_MAX * INV2PI                          # 114.6 revolutions
PM_ERR_PRECISE = LOGF_ULPS * _ulp(PM_MAX) + 2 * U + C1E3_REL
PHASE_PRECISE = 100.0 * PM_ERR_PRECISE + 0.5 * _ulp(100.0 * PM_MAX) + U * 100.0 * PM_MAX
SINCOS_ABS = SINCOS_ULPS * U
REDUCE_ABS = 2 * 0.5 * _ulp(math.pi) + math.pi * (U + INV2PI_REL)


def fast_log_err(y):
    """|fast_log(x) - log x| at y = log x: 1 ulp of log2 x, times ln 2; the product's rounding; ln2f's own error"""
    y = torch.as_tensor(y, dtype=torch.float64)
    return ulp32(y / LN2) * LN2 + 0.5 * ulp32(y) + y.abs() * LN2_REL


def _crev_rel():
    c = np.float32(100.0) * np.float32(0.15915494309189535)
    assert c.dtype == np.float32
    crev = (c / dim_mat().numpy()).astype(np.float64)
    exact = 100.0 * INV2PI / DIM.numpy()
    return float(np.max(np.abs(crev - exact) / exact))


CREV_REL = _crev_rel()
PM_ERR_FAST = float(fast_log_err(PM_MAX)) + 4 * U + C1E3_REL
PHASE_FAST_I = (100.0 * PM_ERR_FAST + 100.0 * PM_MAX * CREV_REL) / DIM + 2 * math.pi * 0.5 * ulp32(XREV_MAX / DIM + 0.25)
PHASE_FAST = float(PHASE_FAST_I[0])
# v_sin_f32 / v_cos_f32, absolute: MEASURED on the first GPU run as the largest excess, over all probes of all sets and
# shapes, of |e_recovered - e_f64| over the derived part of the bound (`probe_excess`: V_SIN_ABS = 0), for the two kernels
# whose f32 rows can be inverted; the allowance is twice the larger (a negative excess counts as 0).  The tiled kernels
# share pos_logits_mfma_kernel's arithmetic up to the operand type.  Measured on an MI355X: no entry of either kernel leaves
# the derived part -- the closest are at frequency 7, 1.4e-6 (valu) and 1.1e-6 (mfma) inside it, where the whole error is
# 6.9e-7 (valu: reduction, v_sin / v_cos and readback together, so v_sin_f32's own error is below that) -- so the allowance
# is 0: the hardware sine's error is covered by the slack of the worst-case sum.
V_SIN_EXCESS = {"valu": -1.435e-6, "mfma": -1.109e-6}
V_SIN_MEASURED = max(0.0, *V_SIN_EXCESS.values())
V_SIN_ABS = 2.0 * V_SIN_MEASURED

RND = {None: 0.0, BF16: 2.0 ** -8, F16: 2.0 ** -11}
RND_ABS = {None: 0.0, BF16: 0.0, F16: 2.0 ** -25}


def entry_phase(kind):
    """[64] float64: the part of the entry bound that is a phase error (sin and cos are 1-Lipschitz), entry j at frequency j % 8"""
    per = PHASE_FAST_I if kind in ("mfma", "tiled_bf16", "tiled_f16") else PHASE_PRECISE / DIM
    return per.repeat(8)


def entry_abs(kind, v_sin_abs=None):
    v = V_SIN_ABS if v_sin_abs is None else v_sin_abs
    return {"precise": SINCOS_ABS, "valu": REDUCE_ABS + v}.get(kind, v)


def entry_bound(kind, emb, v_sin_abs=None):
    """|e_kernel - e_f64| allowed per embedding entry, before any readback: emb [..., 64] float64 -> [..., 64]"""
    base = entry_phase(kind) + entry_abs(kind, v_sin_abs)
    dt = KIND_DTYPE[kind]
    return base + RND[dt] * (emb.abs() + base) + RND_ABS[dt]


def acc_rounding(kind, mag):
    """the probes' single accumulator rounding at magnitude `mag`"""
    return _ulp(mag) * (0.5 if kind in ("precise", "valu") else 1.0)


def log_err(kind, y):
    """the last logarithm's absolute error at logit y"""
    if kind in ("precise", "valu"):
        return LOGF_READ_ULPS * ulp32(y)
    return fast_log_err(y)


ADD_REL = U + C1E6_REL


def readback(kind, bias=PROBE_BIAS):
    """what inverting the f32 logit of a probe costs on the entry: pre = bias +- e <= bias + 1"""
    top = bias + 1.0
    return acc_rounding(kind, top) + top * ADD_REL + top * float(log_err(kind, math.log(top)))


def _step16(c, dtype, down):
    """the 16-bit neighbour of c (a tensor of `dtype`) below / above"""
    bits = c.view(torch.int16).to(torch.int32) & 0xFFFF
    neg = bits >= 0x8000
    mag = bits & 0x7FFF
    away = neg == down                       # stepping away from zero
    mag2 = torch.where(away, mag + 1, mag - 1)
    sign = torch.where(neg, 0x8000, 0)
    cross = (~away) & (mag == 0)             # from +-0 towards the other sign: the smallest subnormal of that sign
    out = torch.where(cross, torch.where(neg, 1, 0x8001), sign | mag2)
    out = torch.where(out >= 0x8000, out - 0x10000, out).to(torch.int16)
    return out.view(dtype)


def round16(x, dtype, down):
    """float64 -> the largest `dtype` value <= x (down) or the smallest >= x, as float64"""
    c = x.float().to(dtype)
    bad = (c.double() > x) if down else (c.double() < x)
    return torch.where(bad, _step16(c, dtype, down), c).double()


def logit_interval(pre_lo, pre_hi, kind):
    """the interval the stored logit must lie in when the exact pre-activation of the kernel's own embedding is known to
    lie in [pre_lo, pre_hi] (float64 tensors): relu, + 1e-6f, the logarithm with log_err, and for the tiled kernels the
    rounding to the output type, the ends rounded outwards"""
    x_lo = (pre_lo.clamp_min(0) + 1e-6) * (1 - ADD_REL)
    x_hi = (pre_hi.clamp_min(0) + 1e-6) * (1 + ADD_REL)
    lo, hi = x_lo.log(), x_hi.log()
    lo, hi = lo - log_err(kind, lo), hi + log_err(kind, hi)
    if kind in TILED:
        lo, hi = round16(lo, TILED[kind], True), round16(hi, TILED[kind], False)
    return lo, hi


def interval_ratio(got, lo, hi):
    """-> (worst |got - mid| / halfwidth, index of it): <= 1 inside.  A NaN counts as outside."""
    g = got.double()
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    r = (g - mid).abs() / half.clamp_min(1e-300)
    r = torch.where((g >= lo) & (g <= hi), r.clamp_max(1.0), torch.where(torch.isnan(r), torch.full_like(r, math.inf), r.clamp_min(1.0 + 1e-12)))
    i = int(torch.argmax(r))
    return float(r.flatten()[i]), tuple(int(v) for v in np.unravel_index(i, tuple(r.shape)))


# ----------------------------------------------------------------------------------------------------- the checks
def probe_interval(kind, emb, r, sign, bias=PROBE_BIAS, v_sin_abs=None):
    """interval of the logit [16, Nq, Nk] of probe run (r, sign): pre = bias + sign e_j, j = 16 r + h"""
    j = probed_entries(r)
    e = emb[:, :, j].permute(2, 0, 1)
    eb = entry_bound(kind, emb, v_sin_abs)[:, :, j].permute(2, 0, 1)
    pre = float(bias) + sign * e
    if bias != 0:
        eb = eb + acc_rounding(kind, abs(bias) + 1.0)
    return logit_interval(pre - eb, pre + eb, kind)


def probe_entry_error(kind, got, emb, r, sign, v_sin_abs=None):
    """f32 rows of probe run (r, sign) -> (|e_recovered - e_f64|, its bound), both [16, Nq, Nk]"""
    j = probed_entries(r)
    e = emb[:, :, j].permute(2, 0, 1)
    bound = entry_bound(kind, emb, v_sin_abs)[:, :, j].permute(2, 0, 1) + readback(kind)
    return (embedding_from_logit(got, PROBE_BIAS, sign) - e).abs(), bound


def exp_error(kind, got, pre, pre_err):
    """f32 rows compared through exp(): -> (|exp(got) - 1e-6 - relu(pre)|, its bound) for a float64 pre-activation known
    to pre_err.  relu is 1-Lipschitz; the sum with 1e-6f and the logarithm cost a relative ADD_REL + expm1(log_err) of x."""
    x = pre.clamp_min(0) + pre_err + 1e-6
    bound = pre_err + x * (ADD_REL + torch.expm1(log_err(kind, x.log())))
    return (got.double().exp() - 1e-6 - pre.clamp_min(0)).abs(), bound


def floor_interval(kind, Nq, Nk):
    pre = FLOOR_BIASES.double().view(16, 1, 1).expand(16, Nq, Nk)
    return logit_interval(pre, pre, kind)


def pair_bound(kind, emb, wg_t, bg, v_sin_abs=None):
    """-> (bound [16, Nq, Nk] on the pre-activation with real-valued Wg, {term name: [16, Nq, Nk]})"""
    dt = KIND_DTYPE[kind]
    w = wg_t.double()
    terms = {"entries": torch.einsum("qkj,jh->hqk", entry_bound(kind, emb, v_sin_abs), w.abs())}
    if dt is not None:
        terms["wg16"] = torch.einsum("qkj,jh->hqk", emb.abs(), (w - wg_t.to(dt).double()).abs())
    size = bg.double().abs().view(16, 1, 1) + torch.einsum("qkj,jh->hqk", emb.abs(), w.abs())
    terms["accumulation"] = 64 * 2.0 ** -23 * size
    return sum(terms.values()), terms


def old_style_seeded_ok(got, emb, wg_t, bg):
    """the comparison the suite had: max |exp(got) - exp(ref)| < 6e-3 and mean < 1e-3"""
    ref = (preactivation(emb, wg_t, bg).clamp_min(0) + 1e-6)
    err = (got.double().exp() - ref).abs()
    return bool(err.max() < 6e-3 and err.mean() < 1e-3)


# Each check takes run(wg_t, bg) -> f32 [16, Nq, Nk] (the logits of one kernel, or of a CPU stand-in, on the case's boxes; a
# tiled kernel's stored values widened) and returns (worst error / bound, text naming the worst element): above 1 fails.
def _worst(ratio, what):
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    i = int(torch.argmax(ratio))
    h, q, k = (int(v) for v in np.unravel_index(i, tuple(ratio.shape)))
    return float(ratio.flatten()[i]), "%s head %d q %d k %d" % (what, h, q, k)


def _ratio(err, bound):
    return err / bound


def check_probes(kind, case, run, v_sin_abs=None):
    """all 64 entries, both signs.  f32 rows: the recovered entry within entry_bound + readback of float64; tiled: the
    stored logit inside probe_interval"""
    _, emb = reference(*case)
    best = (0.0, "")
    for r, sign in PROBES:
        got = run(*probe_weights(r, sign))
        if kind in TILED:
            ratio, at = interval_ratio(got, *probe_interval(kind, emb, r, sign, v_sin_abs=v_sin_abs))
            res = (ratio, "run %d sign %+d head %d q %d k %d" % ((r, sign) + at))
        else:
            err, bound = probe_entry_error(kind, got, emb, r, sign, v_sin_abs=v_sin_abs)
            res = _worst(_ratio(err, bound), "run %d sign %+d" % (r, sign))
        best = max(best, res)
    return best


def probe_excess(kind, case, run):
    """f32 rows only: the largest |e_recovered - e_f64| - bound with NO v_sin allowance (what V_SIN_EXCESS records)"""
    _, emb = reference(*case)
    worst = -math.inf
    for r, sign in PROBES:
        err, bound = probe_entry_error(kind, run(*probe_weights(r, sign)), emb, r, sign, v_sin_abs=0.0)
        worst = max(worst, float((err - bound).max()))
    return worst


def check_floor(kind, case, run):
    """Wg = 0: log(max(b, 0) + 1e-6) at every (q, k), within log_err (f32 rows: 2 ulp for logf, the fast_log allowance for
    the fast kernels) after the sum's rounding; tiled: the 16-bit neighbours of that"""
    got = run(*floor_weights())
    ratio, at = interval_ratio(got, *floor_interval(kind, case[1], case[2]))
    return ratio, "bias %g q %d k %d" % (float(FLOOR_BIASES[at[0]]), at[1], at[2])


def check_straddle(kind, case, run, v_sin_abs=None):
    """bg = 0, one-hot: the pre-activation is +-e_j itself.  f32 rows: exp(logit) - 1e-6 within the entry bound of
    relu(+-e_j), and where float64 says +-e_j < -bound the logit is the floor's; tiled: the stored logit's interval"""
    _, emb = reference(*case)
    best = (0.0, "")
    for r, sign in PROBES:
        got = run(*probe_weights(r, sign, bias=0.0))
        lo, hi = probe_interval(kind, emb, r, sign, bias=0.0, v_sin_abs=v_sin_abs)
        ratio, at = interval_ratio(got, lo, hi)
        res = (ratio, "run %d sign %+d head %d q %d k %d (interval)" % ((r, sign) + at))
        if kind not in TILED:
            j = probed_entries(r)
            pre = sign * emb[:, :, j].permute(2, 0, 1)
            eb = entry_bound(kind, emb, v_sin_abs)[:, :, j].permute(2, 0, 1)
            err, bound = exp_error(kind, got, pre, eb)
            res = max(res if ratio > 1 else (0.0, ""), _worst(_ratio(err, bound), "run %d sign %+d exp()" % (r, sign)))
        best = max(best, res)
    return best


def check_seeded(kind, case, run, v_sin_abs=None):
    """the seeded model's Wg within the per-pair bound.  A failure names the first (head, q, k) over bound, its four
    log-ratios and the bound's largest term."""
    pm, emb = reference(*case)
    wg_t, bg = seeded_weights()
    got = run(wg_t, bg)
    pre = preactivation(emb, wg_t, bg)
    b, terms = pair_bound(kind, emb, wg_t, bg, v_sin_abs)
    lo, hi = logit_interval(pre - b, pre + b, kind)
    g = got.double()
    bad = ~((g >= lo) & (g <= hi))
    ratio, at = interval_ratio(got, lo, hi)
    what = "head %d q %d k %d (interval)" % at
    if kind not in TILED:
        err, bound = exp_error(kind, got, pre, b)
        r = torch.nan_to_num(_ratio(err, bound), nan=math.inf)
        bad = bad | (r > 1)
        ratio, what = max((ratio if ratio > 1 else 0.0, what), _worst(r, "exp()"))
    if bad.any():
        h, q, k = (int(v) for v in bad.nonzero()[0])
        big = max(terms, key=lambda n: float(terms[n][h, q, k]))
        what = "first over bound: head %d q %d k %d, got %r in [%r, %r], log-ratios (dx, dy, dw, dh) %s, pre %.9g +- %.3g, " \
               "largest term %s %.3g" % (h, q, k, float(got[h, q, k]), float(lo[h, q, k]), float(hi[h, q, k]),
                                         ["%.6f" % v for v in pm[q, k].tolist()], float(pre[h, q, k]), float(b[h, q, k]),
                                         big, float(terms[big][h, q, k]))
    return ratio, what


def values_in_interval(kind, lo, hi):
    """tiled kinds: how many values of the output type lie in [lo, hi] (both representable), per element.  2 is the least an
    interval round a value that is not representable can hold: the check then allows the two neighbours and nothing else."""
    def ordinal(x):
        bits = x.float().to(TILED[kind]).view(torch.int16).to(torch.int64) & 0xFFFF
        return torch.where(bits >= 0x8000, -(bits & 0x7FFF), bits)
    return ordinal(hi) - ordinal(lo) + 1


# ===================================================================================================== f32 emulation
FAULTS = ("dx_floor", "logit_floor", "cos_shift", "dim_mat", "sincos_swapped", "delta01_swapped", "no_relu", "heads_permuted")


def _fast_log(x):
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.log2(x.astype(np.float32)) * np.float32(LN2)).astype(np.float32)


def emulate_embedding(bq, bk, kind="tiled_bf16", fault=None):
    """the 64 embedding entries as the fast kernels form them, in numpy f32, operation by operation: fast_div (a * rcp),
    fast_log (log2 * ln2f), crev, the fma into revolutions, fract, the sine, the rounding to the operand type.  libm stands
    in for v_rcp, v_log and v_sin.  -> f32 [Nq, Nk, 64] holding operand-type values.  `fault`: one of FAULTS."""
    assert kind in ("mfma", "tiled_bf16", "tiled_f16") and (fault is None or fault in FAULTS)
    f = np.float32
    g = {n: v.numpy() for n, v in geometry(bq, bk, F32).items()}

    def fdiv(a, b):
        return (a * (f(1) / b)).astype(f)
    dxf = f(1.01e-3 if fault == "dx_floor" else 1e-3)
    pm = [_fast_log(np.abs(fdiv(g["ddx"], g["wq"][:, None])) + dxf),
          _fast_log(np.abs(fdiv(g["ddy"], g["hq"][:, None])) + dxf),
          _fast_log(fdiv(g["wq"][:, None], g["wk"][None, :])),
          _fast_log(fdiv(g["hq"][:, None], g["hk"][None, :]))]
    if fault == "delta01_swapped":
        pm[0], pm[1] = pm[1], pm[0]
    dm = dim_mat().numpy()
    if fault == "dim_mat":
        dm = (dm.astype(np.float64) * (1 + 1e-5)).astype(f)
    crev = ((f(100.0) * f(0.15915494309189535)) / dm).astype(f)
    cshift = f(0.2501 if fault == "cos_shift" else 0.25)
    Nq, Nk = g["ddx"].shape
    emb = np.zeros((Nq, Nk, 64), dtype=f)
    for d in range(4):
        for half, shift in ((0, f(0)), (1, cshift)):
            blk = half if not (fault == "sincos_swapped" and d == 2) else 1 - half
            for i in range(8):
                x = (pm[d].astype(np.float64) * np.float64(crev[i]) + np.float64(shift)).astype(f)      # fma: one rounding
                fr = (x - np.floor(x)).astype(f)
                emb[:, :, d * 16 + blk * 8 + i] = np.sin(2.0 * np.pi * fr.astype(np.float64)).astype(f)
    return _to16(emb, KIND_DTYPE[kind])


def _to16(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dt).float().numpy()


def emulate_fast(bq, bk, wg_t, bg, kind="tiled_bf16", fault=None, emb16=None):
    """pos_logits_tiled_body / pos_logits_mfma_kernel from the boxes to the stored logit: emulate_embedding (or its result,
    `emb16`), Wg rounded to the operand type, the contraction, relu, + 1e-6f, fast_log and, for the tiled kinds, the rounding
    of the logit.  -> f32 [16, Nq, Nk] (a tiled kind: the stored 16-bit values, widened)."""
    f = np.float32
    emb = emulate_embedding(bq, bk, kind, fault) if emb16 is None else emb16
    w16 = _to16(wg_t.numpy(), KIND_DTYPE[kind])
    acc = (np.einsum("qkj,jh->hqk", emb.astype(np.float64), w16.astype(np.float64)) +
           bg.numpy().astype(np.float64).reshape(16, 1, 1)).astype(f)
    if fault == "heads_permuted":
        acc = np.roll(acc, 1, axis=0)
    pre = acc if fault == "no_relu" else np.maximum(acc, f(0))
    out = _fast_log((pre + f(1e-5 if fault == "logit_floor" else 1e-6)).astype(f))
    t = torch.from_numpy(out)
    return t.to(TILED[kind]).float() if kind in TILED else t
