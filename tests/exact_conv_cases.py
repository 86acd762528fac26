"""Integer-valued conv cases whose result has no tolerance, and their float64 reference (plain module, CPU only).

The argument.  Operands are small integers, the FrozenBN scale is a power of two per channel, bias and residual are
integers.  Every product and every partial sum of the contraction is then a multiple of one power of two g, and as long as
bound / g < 2^24 each of them is an f32 number: the f32 accumulation is exact in ANY order, on any MFMA, with or without
split-K, and acc * scale + bias (+ residual) is exact whether or not the compiler contracts it to an fma.  The only rounding
left is the single conversion to the output type, which is round-to-nearest-even (csrc/common.h).  A correct kernel therefore
equals `reference` BIT FOR BIT; one lost or doubled contraction element, a stale k-step, a neighbouring channel's bias or
residual, or another rounding mode shows up as a wrong integer.  `check_exact` asserts the condition, so that "bit-equal" is a
theorem and not a hope; tests/test_exact_conv_cases.py proves on the CPU that the check bites (planted faults).

The split-precision kernels add the roundings their operand forms document -- the hi / lo splits of activations, weights,
residual and output, the one fp16 rounding of an h2 weight -- and `reference_sp` / `reference_sp_block` perform exactly those
(SP_FORMS, SP_TABLE): the same theorem, with the terms of the documented contraction as the products.

Layouts are the kernels' own: activations NHWC, weights OHWI.  A shape is (N, H, W, Cin, Cout, R, stride, pad, dil).
"""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

LIMIT = 2 ** 24
MAX_FINITE = {torch.float16: 65504.0, torch.bfloat16: float(torch.finfo(torch.bfloat16).max),
              torch.float32: float(torch.finfo(torch.float32).max)}
_INT = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}


def _ints(g, shape, a, lo=None):
    return torch.randint(-a if lo is None else lo, a + 1, shape, generator=g).double()


def conv_f64(x, w, stride=1, pad=0, dil=1):
    """float64 convolution of NHWC x with OHWI w -> NHWC"""
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), stride=stride, padding=pad, dilation=dil)
    return y.permute(0, 2, 3, 1).contiguous()


def out_hw(shape):
    N, H, W, Cin, Cout, R, stride, pad, dil = shape
    return (H + 2 * pad - dil * (R - 1) - 1) // stride + 1, (W + 2 * pad - dil * (R - 1) - 1) // stride + 1


# ------------------------------------------------------------------------------------------------ one conversion, two ways
def convert(v, dtype, trunc=False):
    """float64 -> dtype: round to nearest even (torch's own cast, one rounding: float64 holds every value here exactly), or,
    as a planted fault, truncation towards zero."""
    r = v.to(dtype)
    if not trunc or dtype == torch.float32:
        return r
    over = r.double().abs() > v.abs()              # rounded away from zero: one step back in sign-magnitude order
    return (r.view(torch.int16) - over.to(torch.int16)).view(dtype)


def rounding_shares(v, dtype):
    """(share of elements of float64 v not representable in dtype, share that are exact half-way ties)"""
    if dtype == torch.float32:
        return 0.0, 0.0
    near = v.to(dtype).double()
    inexact = near != v
    lo = convert(v, dtype, trunc=True)
    hi = (lo.view(torch.int16) + inexact.to(torch.int16)).view(dtype).double()     # the neighbour away from zero
    tie = inexact & ((v - lo.double()).abs() == (hi - v).abs())
    return inexact.double().mean().item(), tie.double().mean().item()


def activation(v, relu):
    """relu: 0 none, 1 ReLU, 2 LeakyReLU(0.1).  The leaky branch is float32(v) * float32(0.1), computed in f32 as the kernels'
    epilogue (x > 0 ? x : x * 0.1f) and splitk_finalize_kernel do: v is an f32 number (check_exact), the product is rounded to
    f32 once, and the conversion to the output type follows -- two roundings, the same two on both sides."""
    relu = int(relu)
    if relu == 1:
        return v.clamp(min=0)
    if relu == 2:
        v32 = v.float()
        assert torch.equal(v32.double(), v)
        return torch.where(v32 > 0, v32, v32 * torch.tensor(0.1, dtype=torch.float32)).double()
    return v


def epilogue(acc, scale, bias, res, relu, out_dtype, trunc=False):
    v = acc * scale.double() + bias.double()
    if res is not None:
        v = v + res.double()
    return convert(activation(v, relu), out_dtype, trunc)


def exactness(acc_abs_max, g_in, scale, bias, res_abs_max=0.0, g_res=1.0):
    """(bound, g) of one layer: bound = max conv(|x|, |w|) * max scale + max |bias| + max |res|; g = the common power-of-two
    granularity of all terms (g_in: that of the accumulator, i.e. of the layer's input; the weights are integers)."""
    smax, smin = float(scale.max()), float(scale.min())
    bound = acc_abs_max * smax + float(bias.abs().max()) + res_abs_max
    g = min(g_in, g_in * smin, 1.0, g_res)
    assert acc_abs_max / g_in < LIMIT, "accumulator not exact: %g / %g" % (acc_abs_max, g_in)
    return bound, g


# ------------------------------------------------------------------------------------------------ single conv
_OPERANDS = {}


def make_case(shape, dtype, out_dtype, relu, use_res, seed, ax=8, aw=4, ab=16, ar=8, exps=None):
    """One conv + FrozenBN (+ residual) + activation on integer operands.  x, w: integers uniform in +-ax, +-aw; scale: 2^e
    per channel, e uniform in `exps`; bias: integers in +-ab per channel; residual: integers in +-ar -- everything exactly
    representable in its own dtype (bf16 holds integers up to 256, f16 up to 2048), everything varying per channel so that a
    channel index error is visible.  exps = None: (-2 .. 1) -- quarter-integers, which bf16 stops holding at 64; for an f16
    OUTPUT the exponents are taken from the accumulator's own range so that |y| reaches well past 2048 (where f16 starts to
    round integers) and stays below 65504."""
    N, H, W, Cin, Cout, R, stride, pad, dil = shape
    assert max(ax, aw, ar) <= (256 if dtype == torch.bfloat16 else 2048)
    g = torch.Generator().manual_seed(seed)
    key = (tuple(shape), seed, ax, aw)
    if key not in _OPERANDS:                      # (the integers do not depend on the dtype that holds them)
        x = _ints(g, (N, H, W, Cin), ax)
        w = _ints(g, (Cout, R, R, Cin), aw)
        _OPERANDS[key] = (x, w, conv_f64(x, w, stride, pad, dil), g.get_state())
    x, w, acc, state = _OPERANDS[key]
    g.set_state(state)
    if exps is None:
        if out_dtype == torch.float16:
            top = int(math.floor(math.log2(24000.0 / max(float(acc.abs().max()), 1.0))))
            exps = (top - 3, top)
        else:
            exps = (-2, 1)
    scale = torch.pow(2.0, torch.randint(exps[0], exps[1] + 1, (Cout,), generator=g).double()).float()
    bias = _ints(g, (Cout,), ab).float()
    res = _ints(g, acc.shape, ar).to(dtype) if use_res else None
    return SimpleNamespace(shape=tuple(shape), dtype=dtype, out_dtype=out_dtype, relu=int(relu), x=x.to(dtype), w=w.to(dtype),
                           scale=scale, bias=bias, res=res, acc=acc)


def reference(case, fault=None):
    """(y, bound): float64 F.conv2d, acc * scale + bias (+ res), the activation, ONE conversion to out_dtype.
    fault (tests of the check itself): "drop_x" one non-zero x element dropped, "move_w" one w element moved to the neighbouring
    input channel, "swap_bias" the bias of two channels swapped, "trunc" the final conversion by truncation."""
    N, H, W, Cin, Cout, R, stride, pad, dil = case.shape
    acc, bias = case.acc, case.bias
    if fault == "drop_x":
        n, h, wv = N - 1, H // 2 // stride * stride, W // 2 // stride * stride      # (a pixel some output's taps reach)
        c = int((case.x[n, h, wv] != 0).nonzero()[0])
        x = case.x[n:n + 1].clone()
        x[0, h, wv, c] = 0
        acc = acc.clone()
        acc[n:n + 1] = conv_f64(x, case.w, stride, pad, dil)
    elif fault == "move_w":
        o, r = Cout // 2, R // 2
        c = int((case.w[o, r, r, :-1] != 0).nonzero()[0])
        w = case.w[o:o + 1].clone()
        w[0, r, r, c + 1] += w[0, r, r, c]
        w[0, r, r, c] = 0
        acc = acc.clone()
        acc[..., o:o + 1] = conv_f64(case.x, w, stride, pad, dil)
    elif fault == "swap_bias":
        a = Cout // 3
        b = a + 1 + int((bias[a + 1:] != bias[a]).nonzero()[0])
        bias = bias.clone()
        bias[a], bias[b] = case.bias[b], case.bias[a]
    else:
        assert fault in (None, "trunc")
    y = epilogue(acc, case.scale, bias, case.res, case.relu, case.out_dtype, trunc=fault == "trunc")
    bound = _abs_bound(case) * float(case.scale.max()) + float(case.bias.abs().max()) \
        + (float(case.res.double().abs().max()) if case.res is not None else 0.0)
    return y, bound


def _abs_bound(case):
    """max conv(|x|, |w|): no partial sum of the contraction, in any order, exceeds it"""
    if getattr(case, "_absacc", None) is None:
        N, H, W, Cin, Cout, R, stride, pad, dil = case.shape
        case._absacc = float(conv_f64(case.x.double().abs(), case.w.double().abs(), stride, pad, dil).max())
    return case._absacc


def check_exact(case):
    """asserts the condition of the theorem: bound / g < 2^24 (g: common power-of-two granularity of every term), and |y| below
    the output type's largest finite value.  Returns bound / g."""
    y, bound = reference(case)
    g = min(1.0, float(case.scale.min()))
    assert _abs_bound(case) < LIMIT, "accumulator not exact: %g" % _abs_bound(case)
    assert bound / g < LIMIT, "not exact in f32: bound %g / g %g = %g >= 2^24" % (bound, g, bound / g)
    v = activation(case.acc * case.scale.double() + case.bias.double() + (0 if case.res is None else case.res.double()), case.relu)
    assert float(v.abs().max()) < MAX_FINITE[case.out_dtype] and torch.isfinite(y.float()).all()
    return bound / g


# ------------------------------------------------------------------------------------------------ the comparison
def assert_bits_equal(got, want, what, relu=0, tile=None):
    """got == want as integer views (int16 / int32).  A -0 in `got` counts as +0 only where want is +0 after ReLU (relu == 1: the
    kernels' x * 0.f of a negative x is -0, their max-on-the-rounded-bits form gives +0; both are "zero after ReLU").
    tile = (BM, BN) of the kernel, when known, lets the report say whether the first difference lies in the last M- or N-tile.
    (An output element belongs to every K range, so a K-range seam shows up as a wrong integer anywhere; the report gives the
    integer difference, from which the lost or doubled product can be read.)"""
    got = got.detach().cpu()
    want = want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s against %s %s" % (
        what, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
    it = _INT[got.dtype]
    gi, wi = got.contiguous().view(it).clone(), want.contiguous().view(it)
    if int(relu) == 1:
        neg0 = torch.iinfo(it).min
        gi[(gi == neg0) & (wi == 0)] = 0
    diff = gi != wi
    nd = int(diff.sum())
    if nd == 0:
        return
    idx = tuple(int(i) for i in diff.nonzero()[0])
    C = got.shape[-1]
    c = idx[-1]
    m = 0
    for i, s in zip(idx[:-1], got.shape[:-1]):
        m = m * s + i
    M = got.numel() // C
    where = []
    if got.dim() == 4:
        _, Ho, Wo, _ = got.shape
        where += [n for n, f in (("first row", idx[1] == 0), ("last row", idx[1] == Ho - 1), ("first column", idx[2] == 0),
                                 ("last column", idx[2] == Wo - 1)) if f]
    if tile is not None:
        bm, bn = tile
        if m >= (M - 1) // bm * bm:
            where.append("last M-tile of %d" % bm)
        if c >= (C - 1) // bn * bn:
            where.append("last N-tile of %d" % bn)
    g, w = float(got[idx]), float(want[idx])
    raise AssertionError("%s: %d of %d elements differ; first at pixel %s (GEMM row %d of %d), channel %d of %d [%s]: got %r "
                         "(bits %d), want %r (bits %d), got - want = %r" % (
                             what, nd, got.numel(), idx[:-1], m, M, c, C, ", ".join(where) or "interior", g, int(gi[idx]), w,
                             int(wi[idx]), g - w))


# ------------------------------------------------------------------------------------------------ the two fused bottlenecks
def make_bottleneck_case(hw, dtype, seed, ds=False):
    """layer1's bottleneck on integers: x >= 0 (it follows a ReLU) [N,H,W,256] (ds: 64), w1 / w2 / w3 (/ wd) integers, scales
    powers of two chosen so that the block's output is of the order of its residual (a residual channel error is visible)."""
    N, H, W = hw
    g = torch.Generator().manual_seed(seed)
    cin = 64 if ds else 256
    x = _ints(g, (N, H, W, cin), 4, lo=0)
    ws = [_ints(g, s, 2) for s in ((64, 1, 1, cin), (64, 3, 3, 64), (256, 1, 1, 64))]
    if ds:
        ws.append(_ints(g, (256, 1, 1, 64), 2))
    exps = [(-1, 0), (-5, -4), (-4, -3), (-2, -1)]
    sb = []
    for i, wt in enumerate(ws):
        n = wt.shape[0]
        sb.append((torch.pow(2.0, torch.randint(exps[i][0], exps[i][1] + 1, (n,), generator=g).double()).float(),
                   _ints(g, (n,), 8).float()))
    return SimpleNamespace(hw=tuple(hw), dtype=dtype, ds=ds, x=x.to(dtype), w=[t.to(dtype) for t in ws], sb=sb)


def reference_bottleneck(case):
    """(y, [bound / g per layer]): the three (ds: four) layers in float64, each rounded ONCE to the operand dtype, as the
    conv2d_nhwc launches the fused kernels replace do; the exactness condition is asserted for every layer (g shrinks by each
    layer's smallest scale: a rounded value stays a multiple of the granularity it had)."""
    dt = case.dtype
    x = case.x.double()
    ratios = []

    def layer(inp, g_in, i, pad, res, g_res, relu):
        w, (sc, bi) = case.w[i].double(), case.sb[i]
        acc = conv_f64(inp, w, 1, pad, 1)
        amax = float(conv_f64(inp.abs(), w.abs(), 1, pad, 1).max())
        bound, g = exactness(amax, g_in, sc, bi, 0.0 if res is None else float(res.abs().max()), g_res)
        assert bound / g < LIMIT, "layer %d not exact: %g / %g" % (i, bound, g)
        ratios.append(bound / g)
        y = epilogue(acc, sc, bi, res, relu, dt)
        assert float(y.double().abs().max()) < MAX_FINITE[dt]
        return y.double(), g

    if case.ds:
        ident, g_id = layer(x, 1.0, 3, 0, None, 1.0, 0)
    else:
        ident, g_id = x, 1.0
    t1, g1 = layer(x, 1.0, 0, 0, None, 1.0, 1)
    t2, g2 = layer(t1, g1, 1, 1, None, 1.0, 1)
    y, _ = layer(t2, g2, 2, 0, ident, g_id, 1)
    return y.to(dt), ratios


# ------------------------------------------------------------------------------------------------ the stem
STEM_MEAN = (103.0, 116.0, 123.0)          # three different integers: u8 - mean is an integer of |.| <= 255, exact in bf16 / f16


def make_stem_case(hw, seed):
    """u8 pixels, integer 7x7 weights of magnitude <= 2, power-of-two scale, integer bias"""
    N, H, W = hw
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    w = _ints(g, (64, 3, 7, 7), 2).float()                      # OIHW, as conv1.weight
    scale = torch.pow(2.0, torch.randint(-3, 0, (64,), generator=g).double()).float()
    bias = _ints(g, (64,), 16).float()
    return SimpleNamespace(hw=tuple(hw), u8=u8, w=w, scale=scale, bias=bias, mean=STEM_MEAN)


def stem_image(case, to_bgr=True):
    """the preprocessed image, f32 NCHW: channel c = u8[..., 2 - c if to_bgr else c] - mean[c]"""
    x = case.u8.permute(0, 3, 1, 2).double()
    if to_bgr:
        x = x.flip(1)
    return (x - torch.tensor(case.mean, dtype=torch.float64).view(1, 3, 1, 1)).float().contiguous()


def reference_stem(case, out_dtype, to_bgr=True, pool=False):
    """(y NHWC, bound / g): conv 7x7 stride 2 pad 3 of the mean-subtracted image -- the zero padding is applied AFTER the mean is
    subtracted (a padded pixel is 0, not -mean) --, scale, bias, ReLU, one conversion; pool: max_pool2d(3, 2, 1) of that."""
    img = stem_image(case, to_bgr).double()
    acc = F.conv2d(img, case.w.double(), stride=2, padding=3)
    amax = float(F.conv2d(img.abs(), case.w.double().abs(), stride=2, padding=3).max())
    bound, g = exactness(amax, 1.0, case.scale, case.bias)
    assert bound / g < LIMIT
    v = (acc * case.scale.double().view(1, -1, 1, 1) + case.bias.double().view(1, -1, 1, 1)).clamp(min=0)
    assert float(v.max()) < MAX_FINITE[out_dtype]
    y = v.to(out_dtype)
    if pool:
        y = F.max_pool2d(y.float(), 3, 2, 1).to(out_dtype)      # (max commutes with the monotone rounding; y >= 0)
    return y.permute(0, 2, 3, 1).contiguous(), bound / g


# ------------------------------------------------------------------------------------------------ split precision
# operand form of ops.conv2d_sp -> (dtype T of planes and weights, blocks of the K axis per tap).  The documented contractions:
#   "x3"  x_hi.Wh + x_lo.Wh + x_hi.Wl   (x_lo.Wl is not part of it), planes and weight split by two bf16 roundings each
#   "h2"  (x_hi + x_lo) . f16(W)        f16 planes, W rounded to fp16 ONCE
#   "hi"  x_hi . bf16(W)                only the hi plane is read (from planes, or -- plain_x -- from a plain bf16 tensor)
SP_FORMS = {"x3": (torch.bfloat16, 3), "h2": (torch.float16, 2), "hi": (torch.bfloat16, 1)}
SP_OUT_MODES = ("planes", "f32", "plain")
_WIDE_W = {torch.bfloat16: (257.0, 259.0, 515.0),        # bf16: 256 / 260 / 516, lo part -+1
           torch.float16: (2049.0, 2051.0, 4099.0)}      # not fp16 numbers: 2048 / 2052 / 4100


def split_hi_lo(v, dtype=torch.bfloat16, trunc_lo=False):
    """the two roundings of a split: hi = dtype(v), lo = dtype(v - hi) (v f32; v - hi is an f32 number).  trunc_lo: the
    second one by truncation (a planted fault)."""
    v = v.float()
    hi = v.to(dtype)
    return hi, convert((v - hi.float()).double(), dtype, trunc=trunc_lo)


def make_sp_case(shape, wide_w, relu, use_res, seed, form="x3", plain_x=False, xbig=4096, pbig=None, xband=None,
                 pwide=0.03125, sexp=(-1, 0), ab=16, abig=None, ar=1024):
    """conv2d_sp on integers.  x: mostly |x| <= 8, a share pbig (default one element in eight; wide_w: in 32) up to +-xbig (4096:
    13 bits, the lo plane is needed in bf16 and in f16, and x = hi + lo holds exactly); w: |w| <= 4, or (wide_w) one element in 32
    from +-_WIDE_W, which T does not hold (bf16: hi part 256 / 260 / 516, lo part +-1; f16: one rounding to 2048 / 2052 / 4100);
    xband = (lo, hi): the wide activations are odd integers of magnitude lo .. hi instead (every one of them needs its lo plane,
    at the least magnitude: long-K cases).  pwide: the share of wide weights.  scale 2^e, e uniform in sexp; integer bias up to
    +-ab -- abig = (lo, hi): on about half of the channels of magnitude lo .. hi, which moves those channels' outputs into
    the binades where the SECOND rounding of an output split is inexact; integer residual up to +-ar.  form "h2": the product
    of a 13-bit x and a 12-bit w alone would exceed 2^24, so wide weights sit on the input channels c % 8 == 0 and wide
    activations on the others.  plain_x ("hi" only): x is a bf16 tensor, not planes."""
    N, H, W, Cin, Cout, R, stride, pad, dil = shape
    T = SP_FORMS[form][0]
    assert not plain_x or form == "hi"
    g = torch.Generator().manual_seed(seed)
    x = _ints(g, (N, H, W, Cin), 8)
    if pbig is None:
        pbig = 0.03125 if wide_w else 0.125
    big = torch.rand(x.shape, generator=g) < pbig
    wc = (torch.arange(Cin) % 8 == 0) if (form == "h2" and wide_w) else torch.zeros(Cin, dtype=torch.bool)
    if xband is None:
        wide_x = _ints(g, x.shape, xbig)
    else:
        wide_x = (_ints(g, x.shape, xband[1], lo=xband[0]).long() | 1).double() * (2 * torch.randint(0, 2, x.shape, generator=g) - 1)
    x = torch.where(big & ~wc, wide_x, x)
    w = _ints(g, (Cout, R, R, Cin), 4)
    if wide_w:
        pick = torch.rand(w.shape, generator=g) < (8 * pwide if form == "h2" else pwide)
        if form == "h2":
            pick = pick & wc
        mags = torch.tensor(_WIDE_W[T], dtype=torch.float64)
        vals = torch.cat([mags, -mags])
        w = torch.where(pick, vals[torch.randint(0, 6, w.shape, generator=g)], w)
    scale = torch.pow(2.0, torch.randint(sexp[0], sexp[1] + 1, (Cout,), generator=g).double()).float()
    bias = _ints(g, (Cout,), ab).float()
    Ho, Wo = out_hw(shape)
    res = _ints(g, (N, Ho, Wo, Cout), ar).float() if use_res else None
    if abig is not None:
        wide_b = _ints(g, (Cout,), abig[1], lo=abig[0]) * (2 * torch.randint(0, 2, (Cout,), generator=g) - 1)
        bias = torch.where(torch.rand((Cout,), generator=g) < 0.5, wide_b.float(), bias)
    if plain_x:
        x = x.to(T).double()
    return SimpleNamespace(shape=tuple(shape), form=form, pdt=T, plain_x=plain_x, relu=int(relu), x=x.float(), w=w.float(),
                           scale=scale, bias=bias, res=res, _sp=None)


SP_FAULTS = ("drop_xlo_wh", "drop_xhi_wl", "add_xlo_wl", "drop_res_lo", "trunc_lo", "shift_lo", "w_unrounded", "wrap_early",
             "hi_reads_lo", "trunc_plain")


def sp_fault_applies(case, out_mode, fault):
    """whether the planted fault is one this case can show (it has that term / operand / output)"""
    form = getattr(case, "form", "x3")
    return {"drop_xlo_wh": form in ("x3", "h2"), "drop_xhi_wl": form == "x3" and bool(_sp_setup(case).wl_any),
            "add_xlo_wl": form == "x3" and bool(_sp_setup(case).wl_any), "drop_res_lo": case.res is not None,
            "trunc_lo": out_mode == "planes", "shift_lo": out_mode == "planes",
            "w_unrounded": form == "h2" and not torch.equal(case.w.to(torch.float16).float(), case.w),
            "wrap_early": form == "x3", "hi_reads_lo": form == "hi" and not case.plain_x,
            "trunc_plain": out_mode == "plain"}[fault]


def _sp_setup(case):
    """the case's operands as the kernel contracts them, computed once: blocks [(a_i, b_i)] of the K axis per tap (f64), the exact
    accumulator, max conv(|a|, |b|), the residual as hi + lo"""
    if getattr(case, "_sp", None) is not None:
        return case._sp
    form = getattr(case, "form", "x3")
    T = SP_FORMS[form][0]
    geo = case.shape[6:]
    xh, xl = split_hi_lo(case.x, T)
    assert torch.equal(xh.double() + xl.double(), case.x.double()) and float(case.x.abs().max()) < MAX_FINITE[T]
    if form == "x3":
        wh, wl = split_hi_lo(case.w, T)
        blocks = [(xh, wh), (xl, wh), (xh, wl)]
    else:
        wh, wl = case.w.to(T), None
        blocks = [(xh, wh), (xl, wh)] if form == "h2" else [(xh, wh)]
    blocks = [(a.double(), b.double()) for a, b in blocks]
    A = torch.cat([a for a, _ in blocks], dim=-1)
    Wk = torch.cat([b for _, b in blocks], dim=-1)
    s = SimpleNamespace(T=T, geo=geo, xh=xh.double(), xl=xl.double(), wh=wh.double(), wl=None if wl is None else wl.double(),
                        wl_any=wl is not None and bool((wl != 0).any()), blocks=blocks, A=A, Wk=Wk)
    s.acc = conv_f64(A, Wk, *geo)
    s.amax = float(conv_f64(A.abs(), Wk.abs(), *geo).max())
    s.res = s.res_hi = None
    if case.res is not None:
        rh, rl = split_hi_lo(case.res, T)
        s.res_hi = rh.double()
        s.res = rh.double() + rl.double()
        assert torch.equal(s.res, case.res.double())
    bound, g = exactness(s.amax, 1.0, case.scale, case.bias, 0.0 if s.res is None else float(s.res.abs().max()))
    assert bound / g < LIMIT, "SP case not exact: %g" % (bound / g)
    s.ratio = bound / g
    case._sp = s
    return s


def sp_value(case, fault=None):
    """the exact f32 value y before the output stage, as float64 (fault: one of the contraction / residual faults of SP_FAULTS)"""
    s = _sp_setup(case)
    acc, res = s.acc, s.res
    if fault == "drop_xlo_wh":
        acc = acc - conv_f64(s.xl, s.wh, *s.geo)
    elif fault == "drop_xhi_wl":
        acc = acc - conv_f64(s.xh, s.wl, *s.geo)
    elif fault == "add_xlo_wl":
        acc = acc + conv_f64(s.xl, s.wl, *s.geo)
    elif fault == "hi_reads_lo":                           # the "hi" form contracting the lo plane as well
        acc = acc + conv_f64(s.xl, s.wh, *s.geo)
    elif fault == "w_unrounded":
        acc = acc + conv_f64(s.xh + s.xl, case.w.double() - s.wh, *s.geo)
    elif fault == "wrap_early":
        # the kernel's K index of one tap runs over [hi | lo | hi'] with hi' = source channel k - kwrap, kwrap = 2C.  Wrapped one
        # 64-element K-tile early (kwrap = 2C - 64) in the centre tap: k in [2C - 64, 3C) reads source channel k - 2C + 64
        C = case.shape[3]
        src = torch.cat([s.xh, s.xl], dim=-1)
        k = torch.arange(3 * C)
        bad = src[..., torch.where(k >= 2 * C - 64, k - (2 * C - 64), k)]
        r = case.shape[5] // 2
        wt = torch.zeros_like(s.Wk)
        wt[:, r, r] = s.Wk[:, r, r]
        acc = acc + conv_f64(bad - s.A, wt, *s.geo)
    elif fault == "drop_res_lo":
        res = s.res_hi
    v = activation(acc * case.scale.double() + case.bias.double() + (0 if res is None else res), case.relu)
    if fault is None:
        assert torch.equal(v.float().double(), v)
    return v


def sp_output(v, T, out_mode, fault=None):
    """the output stage: "f32" the value; "planes" [T(y) | T(y - T(y))] along the channel axis; "plain" ONE nearest-even conversion.
    faults: "trunc_lo" the lo plane by truncation, "shift_lo" the lo plane taken from the neighbouring 8-column vector,
    "trunc_plain" the plain conversion by truncation."""
    y = v.float()
    if out_mode == "f32":
        return y
    if out_mode == "plain":
        return convert(v, T, trunc=fault == "trunc_plain")
    assert out_mode == "planes"
    hi, lo = split_hi_lo(y, T, trunc_lo=fault == "trunc_lo")
    if fault == "shift_lo":
        lo = lo.roll(8, dims=-1)
    return torch.cat([hi, lo], dim=-1)


def reference_sp(case, out_mode, fault=None):
    """(y, bound / g): the documented contraction of the case's operand form in float64 (SP_FORMS), the residual entering as
    hi + lo of its own split, FrozenBN, the activation, then the output stage of `out_mode` (sp_output).  The exactness
    condition (and, for f16, |y| < 65504) is asserted.  The fault-free result is computed once per (case, out_mode)."""
    s = _sp_setup(case)
    cache = s.__dict__.setdefault("out", {})
    if fault is None and out_mode in cache:
        return cache[out_mode], s.ratio
    v = sp_value(case, fault if fault not in ("trunc_lo", "shift_lo", "trunc_plain") else None)
    if fault is None:
        case.acc_v = v
    y = sp_output(v, s.T, out_mode, fault)
    if fault is None:
        if out_mode != "f32":          # (f16 planes and plain outputs: every value below 65504)
            assert float(v.abs().max()) < MAX_FINITE[s.T], "the output leaves %s's finite range: %g" % (s.T, float(v.abs().max()))
        cache[out_mode] = y
    return y, s.ratio


def sp_shares(case, out_mode):
    """shares of elements that exercise the fault classes: in_lo / res_lo -- input / residual elements with a non-zero lo plane;
    for a planes output,
    out_lo -- outputs with a non-zero lo, out_inexact2 -- outputs whose second rounding is inexact (hi + lo != y); for a 16-bit
    plain output, rounded / ties as rounding_shares"""
    s = _sp_setup(case)
    v = sp_value(case)
    d = {"in_lo": (s.xl != 0).double().mean().item()}
    if s.res is not None:
        d["res_lo"] = (s.res != s.res_hi).double().mean().item()
    if out_mode == "planes":
        hi, lo = split_hi_lo(v.float(), s.T)
        d["out_lo"] = (lo != 0).double().mean().item()
        d["out_inexact2"] = (hi.double() + lo.double() != v).double().mean().item()
    elif out_mode == "plain":
        d["rounded"], d["ties"] = rounding_shares(v, s.T)
    return d


# ------------------------------------------------------------------------------------------------ Bottleneck.run_sp
# mode -> (operand form of the 1x1 convs, dtype of planes, dtype of the plain tensors inside the block or None)
SP_BLOCK_MODES = {"x3": ("x3", torch.bfloat16, None), "h2": ("h2", torch.float16, None), "wide": ("hi", torch.bfloat16, torch.bfloat16)}
# kind -> (Cin, mid, Cout, stride, dilation, downsample)
SP_BLOCK_KINDS = {"identity": (256, 64, 256, 1, 1, False), "down-s2": (128, 64, 256, 2, 1, True),
                  "down-dil2": (128, 64, 256, 2, 2, True)}


def make_sp_block_case(kind, hw, seed, plain_x=False):
    """a bottleneck on integers for Bottleneck.run_sp: x >= 0 (it follows a ReLU), mostly 0 .. 4, one element in 16 up to 4095
    (twelve bits: the lo plane of the block's input -- its identity -- is non-zero in bf16 and in f16); sparse weights in
    {-1, 0, 1} (three in four are zero: the accumulators grow slowly enough for three exact layers on 12-bit inputs);
    power-of-two scales, integer bias.  plain_x: x is rounded to bf16 (the stem's output in "wide" mode)."""
    Cin, mid, Cout, stride, dil, ds = SP_BLOCK_KINDS[kind]
    N, H, W = hw
    g = torch.Generator().manual_seed(seed)
    x = _ints(g, (N, H, W, Cin), 4, lo=0)
    x = torch.where(torch.rand(x.shape, generator=g) < 1.0 / 16, _ints(g, x.shape, 4095, lo=0), x)
    if plain_x:
        x = x.to(torch.bfloat16).double()
    shapes = [(mid, 1, 1, Cin), (mid, 3, 3, mid), (Cout, 1, 1, mid)] + ([(Cout, 1, 1, Cin)] if ds else [])
    ws = [torch.where(torch.rand(s, generator=g) < 0.25, _ints(g, s, 1), torch.zeros(s, dtype=torch.float64)) for s in shapes]
    exps = [(-2, -1), (-2, -1), (-2, -1), (-1, 0)]
    sb = []
    for i, wt in enumerate(ws):
        n = wt.shape[0]
        sb.append((torch.pow(2.0, torch.randint(exps[i][0], exps[i][1] + 1, (n,), generator=g).double()).float(),
                   _ints(g, (n,), 8).float()))
    return SimpleNamespace(kind=kind, hw=tuple(hw), plain_x=plain_x, x=x.float(), w=[t.float() for t in ws], sb=sb)


def reference_sp_block(case, mode, plain_out, fault=None):
    """(y, [bound / g per layer], [share of non-zero lo per hand-off]): the block in float64 with the hand-off of `mode` between
    the layers -- a planes mode ("x3", "h2"): every layer's f32 result is split [T(y) | T(y - T(y))] and the next layer reads
    exactly hi and lo, through that mode's contraction; "wide": conv1 reads the hi plane of x (or the plain x) and writes ONE
    bf16 conversion, conv2 is the plain bf16 conv, conv3 reads that tensor, adds the identity's hi + lo and splits.  The weights
    are integers that T holds, so W = T(W) and the x3 lo part is zero: a block checks where the planes go, the conv table
    the contraction's terms.  plain_out: the block's result as the mode's plain output (x3 / h2: f32; wide: one bf16 conversion)
    instead of planes.  The exactness condition is asserted for every layer.
    fault (tests of the check): "identity_hi" the identity's lo plane dropped, "ds_dense" the downsample taken from the
    pixel to the right of the one its stride reads."""
    form, T, plain = SP_BLOCK_MODES[mode]
    Cin, mid, Cout, stride, dil, ds = SP_BLOCK_KINDS[case.kind]
    cstride = 1 if dil > 1 else stride                      # (a dilated block runs at stride 1: conv1 and the downsample)
    ratios, lo_shares = [], []

    def planes(v):                                          # f32 value -> (hi, lo) as float64
        hi, lo = split_hi_lo(v.float(), T)
        lo_shares.append((lo != 0).double().mean().item())
        return hi.double(), lo.double()

    def layer(inp, g_in, i, st, pad, dl, res, g_res, relu):
        """inp: (hi, lo) planes or a plain tensor; the contraction of the mode's form with integer weights"""
        w, (sc, bi) = case.w[i].double(), case.sb[i]
        assert torch.equal(w.to(T).double(), w)
        if isinstance(inp, tuple):
            a = inp[0] if form == "hi" else inp[0] + inp[1]
        else:
            a = inp
        acc = conv_f64(a, w, st, pad, dl)
        amax = float(conv_f64(a.abs() if form == "hi" or not isinstance(inp, tuple) else inp[0].abs() + inp[1].abs(), w.abs(),
                              st, pad, dl).max())
        r = None if res is None else res[0] + res[1]
        bound, g = exactness(amax, g_in, sc, bi, 0.0 if r is None else float(r.abs().max()), g_res)
        assert bound / g < LIMIT, "layer %d not exact: %g / %g" % (i, bound, g)
        ratios.append(bound / g)
        v = acc * sc.double() + bi.double() + (0 if r is None else r)
        v = v.clamp(min=0) if relu else v
        assert torch.equal(v.float().double(), v) and float(v.abs().max()) < MAX_FINITE[T]
        return v, g

    x = case.x.double()
    xin = x if case.plain_x else planes(x)
    if case.plain_x:
        assert mode == "wide" and ds and torch.equal(x.to(T).double(), x)
    if ds:
        if fault == "ds_dense":
            v, g_id = layer(xin, 1.0, 3, 1, 0, 1, None, 1.0, False)
            v = v.roll(-1, dims=2)[:, ::cstride, ::cstride]
        else:
            v, g_id = layer(xin, 1.0, 3, cstride, 0, 1, None, 1.0, False)
        ident = planes(v)
    else:
        ident, g_id = xin, 1.0
    if fault == "identity_hi":
        ident = (ident[0], torch.zeros_like(ident[1]))
    v1, g1 = layer(xin, 1.0, 0, cstride, 0, 1, None, 1.0, True)
    if plain is None:
        v2, g2 = layer(planes(v1), g1, 1, 1, dil, dil, None, 1.0, True)
        t2 = planes(v2)
    else:
        v2, g2 = layer(v1.to(plain).double(), g1, 1, 1, dil, dil, None, 1.0, True)
        t2 = v2.to(plain).double()
    v3, _ = layer(t2, g2, 2, 1, 0, 1, ident, g_id, True)
    if plain_out:
        y = v3.float() if plain is None else v3.to(plain)
    else:
        y = torch.cat(split_hi_lo(v3.float(), T), dim=-1)
    return y, ratios, lo_shares


# ------------------------------------------------------------------------------------------------ 4x4 stride-2 deconvolution
def make_deconv_case(N, H, W, Cin, C, dtype, seed):
    """ConvTranspose2d(Cin, C, 4, stride=2) on integers: x [N,H,W,Cin], weight [Cin,C,4,4] (torch's layout), integer bias"""
    g = torch.Generator().manual_seed(seed)
    return SimpleNamespace(dtype=dtype, x=_ints(g, (N, H, W, Cin), 8).to(dtype), wt=_ints(g, (Cin, C, 4, 4), 4).float(),
                           bias=_ints(g, (C,), 16).float())


def reference_deconv(case, relu, H2, W2):
    """(y [N,H2,W2,C], bound): integer conv_transpose2d + bias, activation, crop_like's crop (one row / column off the top / left
    unless the target is the full (2H+2) x (2W+2) map), one conversion"""
    x = case.x.double().permute(0, 3, 1, 2)
    N, _, H, W = x.shape
    full = F.conv_transpose2d(x, case.wt.double(), stride=2)
    bound = float(F.conv_transpose2d(x.abs(), case.wt.double().abs(), stride=2).max()) + float(case.bias.abs().max())
    assert bound < LIMIT
    crop = 0 if (2 * H + 2, 2 * W + 2) == (H2, W2) else 1
    v = activation(full.permute(0, 2, 3, 1) + case.bias.double(), relu)[:, crop:crop + H2, crop:crop + W2]
    assert float(v.abs().max()) < MAX_FINITE[case.dtype]
    return convert(v.contiguous(), case.dtype), bound


# ------------------------------------------------------------------------------------------------ the cases of the GPU file
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32

# (shape, relu, use_res, f32 output for the 16-bit operand types)
TILE_CASES = [
    ((1, 19, 23, 64, 72, 3, 1, 1, 1), 1, False, False),          # M and N tails, 9 K-tiles
    ((2, 13, 15, 128, 192, 3, 1, 2, 2), 2, False, False),        # dilation, LeakyReLU
    ((1, 21, 17, 256, 136, 1, 2, 0, 1), 1, True, False),         # stride-2 1x1, residual + ReLU
    ((3, 9, 13, 192, 128, 4, 1, 3, 1), 0, False, True),          # 4x4, pad 3, f32 output
    ((1, 7, 9, 64, 60, 1, 1, 0, 1), 0, True, False),             # Cout % 8 != 0: the element-wise store path, residual
    ((300, 1, 1, 1024, 155, 1, 1, 0, 1), 0, False, False),       # the same on a linear, M and N tails
]
IGEMM8_CASES = [
    ((1, 19, 23, 128, 320, 3, 1, 1, 1), 2, False, False),        # N tail, 18 K-tiles, LeakyReLU
    ((1, 17, 29, 192, 264, 1, 1, 0, 1), 0, False, True),         # odd K-tile count, f32 output
    ((1, 13, 15, 64, 320, 1, 1, 0, 1), 1, False, False),         # one K-tile
    ((1, 13, 15, 128, 256, 1, 1, 0, 1), 1, True, False),         # residual, M below one tile
]
# (shape, relu, use_res, expected kind)
NATURAL_CASES = [
    ((3, 38, 63, 64, 1024, 3, 1, 1, 1), 1, False, 8),            # matrix class
    ((2, 30, 51, 128, 2048, 1, 1, 0, 1), 1, True, 7),            # streaming class, eight N tiles, row tail
]
CONV64_SHAPE = (5, 70, 90, 64, 64, 3, 1, 1, 1)
LINEAR_SPLITK_SHAPE = (37, 1, 1, 32768 + 1024, 72, 1, 1, 0, 1)   # the library's rule: K >= 32768 -> three K ranges
CALLER_SPLITK_SHAPE = (2, 6, 8, 512, 128, 3, 1, 1, 1)
BOTTLENECK_SIZES = [(3, 37, 53), (1, 8, 16)]
STEM_SIZES = [(2, 31, 33), (1, 9, 7), (1, 17, 130)]
# (shape, wide weights, relu, use_res)
SP_CASES = [
    ((1, 19, 23, 64, 64, 3, 1, 1, 1), False, 1, False),
    ((1, 13, 15, 128, 264, 1, 1, 0, 1), True, 0, True),
]
# The split-precision table: every operand form, launch class x row count, output mode x residual, activation, Cout class and
# geometry of the SP kernels at least once.  kind 7 streaming / 8 matrix and the rows are what the library's own rule must give
# (mega_conv2d_nhwc_sp_plan; asserted on the CPU and again before every GPU comparison).  The 256-row instantiation is chosen
# only where it saves a round of the 256 CUs: Cout 2048 with 6144 < M <= 8192.
# form "hi-plain": the "hi" form fed a plain bf16 tensor.  pad_cols > 0: the caller's out= buffer, ldo = Cout + pad_cols.
# knobs: make_sp_case's ranges where the defaults would break a condition (exactness; |y| < 65504 in f16; the 1 % shares).
_P = dict
_B18 = (1 << 17, 1 << 18)
_H2 = _P(sexp=(-9, -8), ab=64, ar=4095, pbig=0.125)                   # g = 2^-9: bound / g < 2^24 keeps every |y| below 32768
# (id, shape, form, wide_w, relu, use_res, out_mode, pad_cols, kind, rows, knobs)
SP_TABLE = [
    # 256 rows, streaming (K = 192): split residual and split output through the MF1 = 2 residual prefetch
    ("s256-x3-res-planes", (1, 50, 124, 64, 2048, 1, 1, 0, 1), "x3", True, 1, True, "planes", 0, 7, 256, _P(abig=_B18)),
    # 256 rows, matrix (K = 576): f32 output with a residual (the h4[d] / h4[2 + d] unpack)
    ("m256-x3-res-f32", (1, 50, 124, 192, 2048, 1, 1, 0, 1), "x3", True, 0, True, "f32", 0, 8, 256, _P()),
    # 256 rows in f16: [W | W] weights, no wrap, f16 lo plane written
    ("s256-h2-planes", (1, 50, 124, 64, 2048, 1, 1, 0, 1), "h2", True, 1, False, "planes", 0, 7, 256, _P(_H2, abig=(17000, 24000))),
    # Cout 64 with a residual: the waves whose columns do not exist are skipped (use_b0 / use_b1); 3x3 at C = 64
    ("m192-x3-3x3-cout64-res", (1, 19, 23, 64, 64, 3, 1, 1, 1), "x3", False, 1, True, "planes", 0, 8, 192, _P(abig=_B18)),
    # 3x3 at C = 128: the tap / plane wrap runs over two K-tiles per plane; Cout 128 with a residual; LeakyReLU
    ("m192-x3-3x3-c128-leaky", (2, 13, 15, 128, 128, 3, 1, 1, 1), "x3", True, 2, True, "f32", 0, 8, 192, _P()),
    # dilated 3x3, Cout 264 (second N tile of 8 columns), planes without a residual, no activation
    ("m192-x3-dil2-planes", (1, 13, 15, 64, 264, 3, 1, 2, 2), "x3", True, 0, False, "planes", 0, 8, 192, _P(abig=_B18)),
    # stride-2 1x1 on odd H and W (the downsample's stride on planes), M tail
    ("s192-x3-stride2-res", (1, 13, 15, 128, 264, 1, 2, 0, 1), "x3", True, 1, True, "planes", 0, 7, 192, _P(abig=_B18)),
    # f32 into the caller's buffer, ldo > Cout: nothing is written behind column Cout
    ("s192-x3-f32-ldo", (1, 7, 9, 64, 136, 1, 1, 0, 1), "x3", True, 0, False, "f32", 8, 7, 192, _P()),
    # "wide" conv1: the hi plane of planes whose lo plane is NOT zero, one plain bf16 conversion, Cout 8
    ("s192-hi-plain-cout8", (1, 13, 15, 256, 8, 1, 1, 0, 1), "hi", True, 1, False, "plain", 0, 7, 192, _P(xbig=511, pbig=0.125)),
    # "wide" conv3: a plain bf16 tensor in (ldi = C), split residual, split output
    ("s192-hiplain-res-planes", (1, 13, 15, 64, 256, 1, 1, 0, 1), "hi-plain", True, 1, True, "planes", 0, 7, 192, _P(abig=_B18)),
    # "wide" downsample of a dilated block: hi plane, matrix class (K = 576), planes without a residual, LeakyReLU
    ("m192-hi-planes-leaky", (1, 9, 11, 576, 72, 1, 1, 0, 1), "hi", True, 2, False, "planes", 0, 8, 192, _P(abig=_B18)),
    # plain bf16 with a residual into the caller's buffer
    ("s192-hi-res-plain-ldo", (1, 7, 9, 128, 72, 1, 1, 0, 1), "hi", True, 0, True, "plain", 24, 7, 192, _P(xbig=511, pbig=0.125)),
    # h2, 3x3 (K = 1152, matrix class): f16 split residual + f16 split output
    ("m192-h2-3x3-res-planes", (1, 9, 11, 64, 72, 3, 1, 1, 1), "h2", True, 1, True, "planes", 0, 8, 192, _P(_H2, abig=(17000, 22000))),
    # h2, f32 output with a residual, Cout 520 (third N tile of 8 columns), LeakyReLU
    ("s192-h2-res-f32-leaky", (1, 13, 15, 128, 520, 1, 1, 0, 1), "h2", True, 2, True, "f32", 0, 7, 192, _P(_H2)),
    # h2, plain f16 with a residual into the caller's buffer
    ("s192-h2-res-plain-ldo", (1, 13, 15, 64, 72, 1, 1, 0, 1), "h2", True, 0, True, "plain", 8, 7, 192, _P(sexp=(-3, -2), ar=4095, pbig=0.125)),
    # h2, plain f16, no residual, ReLU
    ("s192-h2-plain", (1, 7, 9, 128, 264, 1, 1, 0, 1), "h2", False, 1, False, "plain", 0, 7, 192, _P(sexp=(-3, -2))),
]
# linear_sp above the library's split-K threshold (R S Cw >= 32768 -> three K ranges + finalize): (M, K, Nout), M = 37 and
# Nout = 72 as LINEAR_SPLITK_SHAPE; wide activations are rare so that 10944 / 16384 products stay below 2^24
SP_SPLITK = {"x3": (37, 10944, 72), "h2": (37, 16384, 72)}
# (linear_sp has no FrozenBN scale: sexp = (0, 0) makes it 1)
SP_SPLITK_KNOBS = {"x3": _P(pbig=1.0 / 32, xband=(257, 511), sexp=(0, 0)),
                   "h2": _P(pbig=1.0 / 48, xband=(2049, 2303), pwide=1.0 / 128, sexp=(0, 0))}
SP_LINEAR_T = (37, 192, 136, 64)                 # ops.linear / ops.linear_transposed through an X3Weight: (M, K, Nout, ld)
# Bottleneck.run_sp: (kind, (N, H, W), plain_x) -- the downsample kinds on 13 x 15 (odd: the stride-2 tail); the last row is
# "wide" only (a downsample block fed the stem's plain bf16 tensor)
SP_BLOCKS = [("identity", (1, 9, 12), False), ("down-s2", (1, 13, 15), False), ("down-dil2", (1, 13, 15), False),
             ("down-s2", (1, 13, 15), True)]

# (N, H, W, Cin, C, Cs): the two smallest entries of test_kernels_gpu.DECONV_CASES
DECONV_SHAPES = [(1, 4, 6, 386, 64, 128), (2, 7, 9, 770, 128, 256)]

_CASES = {}


def conv_case(shape, dtype, out_dtype, relu, use_res):
    """make_case with the seed taken from the shape, built once per process and never modified"""
    key = (tuple(shape), dtype, out_dtype, int(relu), bool(use_res))
    if key not in _CASES:
        _CASES[key] = make_case(shape, dtype, out_dtype, relu, use_res, seed=sum(shape) % 1009)
    return _CASES[key]


def _odt(dtype, f32o):
    return F32 if f32o else dtype


def all_conv_cases():
    """every (shape, dtype, out_dtype, relu, use_res) tests/test_exact_conv_gpu.py runs through make_case / reference"""
    keys = []
    for shape, relu, res, f32o in TILE_CASES:
        keys += [(shape, dt, _odt(dt, f32o), relu, res) for dt in (F32, BF16, F16)]
    for shape, relu, res, f32o in IGEMM8_CASES:
        keys += [(shape, dt, _odt(dt, f32o), relu, res) for dt in (BF16, F16)]
    for shape, relu, res, _ in NATURAL_CASES:
        keys += [(shape, dt, dt, relu, res) for dt in (BF16, F16)]
    keys += [(CONV64_SHAPE, dt, dt, relu, False) for dt in (BF16, F16) for relu in (1, 0, 2)]
    keys += [(LINEAR_SPLITK_SHAPE, dt, dt, 1, False) for dt in (F32, BF16, F16)]
    keys += [(CALLER_SPLITK_SHAPE, dt, dt, 2, True) for dt in (F32, BF16, F16)]
    keys += [(CALLER_SPLITK_SHAPE, BF16, F32, 2, True)]
    return keys


def bottleneck_case(hw, dtype, ds):
    return make_bottleneck_case(hw, dtype, seed=sum(hw) + int(ds), ds=ds)


def stem_case(hw):
    return make_stem_case(hw, seed=sum(hw))


def sp_case(spec):
    shape, wide_w, relu, use_res = spec
    return make_sp_case(shape, wide_w, relu, use_res, seed=sum(shape))


_SP_BUILT = {}


def sp_table_case(row):
    """the case of one SP_TABLE row, built once per process and never modified"""
    name, shape, form, wide_w, relu, use_res, out_mode, pad_cols, kind, rows, knobs = row
    if name not in _SP_BUILT:
        _SP_BUILT[name] = make_sp_case(shape, wide_w, relu, use_res, seed=sum(shape) + len(name), form=form.split("-")[0],
                                       plain_x=form == "hi-plain", **knobs)
    return _SP_BUILT[name]


def sp_gemm_shape(shape, form):
    """(M, Cout, K, taps) of the launch: K = R S (blocks of the form) Cin, what mega_conv2d_nhwc_sp_plan takes"""
    N, H, W, Cin, Cout, R, stride, pad, dil = shape
    Ho, Wo = out_hw(shape)
    return N * Ho * Wo, Cout, R * R * SP_FORMS[form.split("-")[0]][1] * Cin, R * R


def sp_splitk_case(form):
    M, K, Nout = SP_SPLITK[form]
    key = "splitk-" + form
    if key not in _SP_BUILT:
        _SP_BUILT[key] = make_sp_case((M, 1, 1, K, Nout, 1, 1, 0, 1), True, 1, False, seed=K % 1009, form=form,
                                      **SP_SPLITK_KNOBS[form])
    return _SP_BUILT[key]


def sp_linear_case(with_bias):
    """the X3Weight case: scale 1; with_bias False (ops.linear_transposed takes none): bias 0"""
    M, K, Nout, ld = SP_LINEAR_T
    key = "linear-bias" if with_bias else "linear-t"
    if key not in _SP_BUILT:
        _SP_BUILT[key] = make_sp_case((M, 1, 1, K, Nout, 1, 1, 0, 1), True, 0, False, seed=M + K + int(with_bias), form="x3",
                                      sexp=(0, 0), ab=16 if with_bias else 0)
    return _SP_BUILT[key]


def sp_block_case(spec):
    kind, hw, plain_x = spec
    key = ("block", kind, hw, plain_x)
    if key not in _SP_BUILT:
        _SP_BUILT[key] = make_sp_block_case(kind, hw, seed=sum(hw) + len(kind) + int(plain_x), plain_x=plain_x)
    return _SP_BUILT[key]


def deconv_case(shape, dtype):
    N, H, W, Cin, C, Cs = shape
    return make_deconv_case(N, H, W, Cin, C, dtype, seed=sum(shape))
