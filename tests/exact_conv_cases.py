"""Integer-valued conv cases whose result has no tolerance, and their float64 reference (plain module, CPU only).

The argument.  Operands are small integers, the FrozenBN scale is a power of two per channel, bias and residual are
integers.  Every product and every partial sum of the contraction is then a multiple of one power of two g, and as long as
bound / g < 2^24 each of them is an f32 number: the f32 accumulation is exact in ANY order, on any MFMA, with or without
split-K, and acc * scale + bias (+ residual) is exact whether or not the compiler contracts it to an fma.  The only rounding
left is the single conversion to the output type, which is round-to-nearest-even (csrc/common.h).  A correct kernel therefore
equals `reference` BIT FOR BIT; one lost or doubled contraction element, a stale k-step, a neighbouring channel's bias or
residual, or another rounding mode shows up as a wrong integer.  `check_exact` asserts the condition, so that "bit-equal" is a
theorem and not a hope; tests/test_exact_conv_cases.py proves on the CPU that the check bites (planted faults).

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


# ------------------------------------------------------------------------------------------------ split precision (x3)
def split_hi_lo(v, dtype=torch.bfloat16):
    """the two roundings of a split: hi = dtype(v), lo = dtype(v - hi) (v f32)"""
    v = v.float()
    hi = v.to(dtype)
    return hi, (v - hi.float()).to(dtype)


def make_sp_case(shape, wide_w, relu, use_res, seed):
    """conv2d_sp(operands="x3") on integers.  x: mostly small, one element in eight (wide_w: in 32) up to +-4096 (13 bits: the lo plane is needed and
    x = hi + lo holds exactly); w: |w| <= 4, or (wide_w) one element in 32 from +-{257, 259, 515}, whose bf16 hi part is
    256 / 260 / 516 and whose lo part is +-1; scale in {1/2, 1}, integer bias, integer residual up to +-1024."""
    N, H, W, Cin, Cout, R, stride, pad, dil = shape
    g = torch.Generator().manual_seed(seed)
    x = _ints(g, (N, H, W, Cin), 8)
    big = torch.rand(x.shape, generator=g) < (0.03125 if wide_w else 0.125)
    x = torch.where(big, _ints(g, x.shape, 4096), x)
    w = _ints(g, (Cout, R, R, Cin), 4)
    if wide_w:
        pick = torch.rand(w.shape, generator=g) < 0.03125
        vals = torch.tensor([257.0, 259.0, 515.0, -257.0, -259.0, -515.0], dtype=torch.float64)
        w = torch.where(pick, vals[torch.randint(0, 6, w.shape, generator=g)], w)
    scale = torch.pow(2.0, torch.randint(-1, 1, (Cout,), generator=g).double()).float()
    bias = _ints(g, (Cout,), 16).float()
    Ho, Wo = out_hw(shape)
    res = _ints(g, (N, Ho, Wo, Cout), 1024).float() if use_res else None
    return SimpleNamespace(shape=tuple(shape), relu=int(relu), x=x.float(), w=w.float(), scale=scale, bias=bias, res=res)


def reference_sp(case, out_mode):
    """(y, bound / g): the DOCUMENTED contraction x_hi.Wh + x_lo.Wh + x_hi.Wl in float64 (x_lo.Wl is not part of it), planes and
    weight split computed here by the same two roundings; the residual enters as hi + lo; out_mode "f32": the f32 value, "planes":
    [bf16(y) | bf16(y - bf16(y))] along the channel axis."""
    N, H, W, Cin, Cout, R, stride, pad, dil = case.shape
    xh, xl = split_hi_lo(case.x)
    wh, wl = split_hi_lo(case.w)
    assert torch.equal(xh.double() + xl.double(), case.x.double()) and bool((xl != 0).any())
    terms = ((xh, wh), (xl, wh), (xh, wl))
    acc = sum(conv_f64(a, b, stride, pad, dil) for a, b in terms)
    amax = float(sum(conv_f64(a.double().abs(), b.double().abs(), stride, pad, dil) for a, b in terms).max())
    res = None
    if case.res is not None:
        rh, rl = split_hi_lo(case.res)
        res = rh.double() + rl.double()
        assert torch.equal(res, case.res.double())
    bound, g = exactness(amax, 1.0, case.scale, case.bias, 0.0 if res is None else float(res.abs().max()))
    assert bound / g < LIMIT, "SP case not exact: %g" % (bound / g)
    v = case.acc_v = activation(acc * case.scale.double() + case.bias.double() + (0 if res is None else res), case.relu)
    y = v.float()
    assert torch.equal(y.double(), v)
    if out_mode == "planes":
        hi, lo = split_hi_lo(y)
        y = torch.cat([hi, lo], dim=-1)
    return y, bound / g


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


def deconv_case(shape, dtype):
    N, H, W, Cin, C, Cs = shape
    return make_deconv_case(N, H, W, Cin, C, dtype, seed=sum(shape))
