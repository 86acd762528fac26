"""Integer-valued FP8 conv cases whose result has no tolerance, and their float64 reference (plain module, CPU only).

The argument is exact_conv_cases.py's.  The activation codes and the weight codes are small integers (exact in e4m3: every
integer of magnitude <= 16), a bf16 input holds code * s_in with s_in a power of two (so the kernel's f32 multiply by 1 / s_in
and its conversion give the code back without rounding), scale[o] is a power of two that DIFFERS per channel, the bias is an
integer and out_inv_scale a power of two.  Every partial sum of the contraction is an integer below 2^24 and, per channel, every
epilogue value is a multiple of one power of two g with bound / g < 2^24: the f32 accumulation is exact in any order on any
MFMA, acc * scale + bias is exact with or without contraction, and the multiply by out_inv_scale is exact.  The only rounding
left is the ONE conversion to the output type -- round to nearest even, after the clamp to +-448 for an fp8 output -- so a
correct kernel equals `reference` byte for byte (the zero codes 0x00 and 0x80 compare equal).  `check_exact` asserts the
condition per case; tests/test_f8_conv_cases.py proves on the CPU that the comparison bites (planted faults) and that the
fp8-output cases put at least 1 % of their elements into every rounding class (rounding_shares).

A shape is (N, H, W, Cin, Cout, R): R = 1 is the 1x1 / pad 0 conv, R = 3 the 3x3 / pad 1 conv, stride 1.  Channels come in eight
kinds (o % 8) so that one case reaches every class: sparse weight rows (a few non-zero codes: small accumulators on a coarse
lattice, where ties live), dense rows scaled into the subnormal range, into saturation on both sides, and into the binades
between.
"""
from types import SimpleNamespace

import torch

from exact_conv_cases import conv_f64, convert

FP8 = torch.float8_e4m3fn
BF16 = torch.bfloat16
LIMIT = 2 ** 24
FP8_MAX = 448.0

# (N, H, W, Cin, Cout, R)
SHAPES = [
    (1, 5, 7, 128, 64, 1),          # one K step, 35 rows: fewer than any tile
    (2, 13, 11, 1024, 256, 1),      # conv1's K and Cout, 286 rows: crosses a 256-row edge
    (1, 5, 7, 256, 256, 3),         # conv2's shape on a small map: most windows touch a border
    (2, 9, 17, 256, 256, 3),        # 306 rows, a tile edge inside an image row, odd width
    (1, 3, 3, 384, 192, 3),         # 27 K steps of 128 (an odd count), Cout not a multiple of 128
]
ALL_COMBOS = (0, 2)                  # the shapes every in x out combination runs on
FAULTS = ("truncate", "no_saturate", "fnuz_bias", "k_permuted", "transposed_out", "per_tensor_wscale", "pad_wraps_row",
          "drop_last_kstep", "relu_after_quant_sign")
CLASSES = ("exact", "up", "down", "tie_to_even_below", "tie_to_even_above", "sat_hi", "sat_lo_before_relu", "subnormal")

# channel kind o % 8 -> (non-zero weight codes per row or None = dense, target magnitude of the pre-rounding value or None =
# the fixed exponent that follows, exponent of the scale, bias allowed)
_KINDS = [(4, None, 0, True), (8, None, -1, True), (None, 2.0 ** -7, None, False), (None, 1500.0, None, True),
          (None, 3.0, None, True), (None, 40.0, None, True), (None, 200.0, None, True), (2, None, 1, True)]


def _natural(R):
    """conv1 (1x1) reads the bf16 trunk and writes codes; conv2 (3x3) reads codes and writes bf16"""
    return ("bf16", "f8") if R == 1 else ("f8", "bf16")


def case_keys():
    """[(shape, in_kind, out_kind, relu)]: all four in x out combinations on shapes 0 and 2, the natural one on the rest; the
    natural combination has the block's ReLU, the others alternate (without ReLU the negative saturation is stored)"""
    keys = []
    for i, shape in enumerate(SHAPES):
        nat = _natural(shape[5])
        if i in ALL_COMBOS:
            for ik in ("bf16", "f8"):
                for ok in ("bf16", "f8"):
                    keys.append((shape, ik, ok, 1 if (ik, ok) == nat or (ik, ok) == nat[::-1] else 0))
        else:
            keys.append((shape, nat[0], nat[1], 1))
    return keys


def case_id(key):
    shape, ik, ok, relu = key
    return "%s-%sin-%sout-relu%d" % ("x".join(str(v) for v in shape), ik, ok, relu)


def make_case(shape, in_kind, out_kind, relu, seed):
    N, H, W, Cin, Cout, R = shape
    pad = R // 2
    g = torch.Generator().manual_seed(seed)
    # activation codes: mostly the non-negative integers a post-ReLU trunk has, one in four negative; -5 .. 12
    a = torch.randint(0, 13, (N, H, W, Cin), generator=g).double()
    a = torch.where(torch.rand(a.shape, generator=g) < 0.25, -torch.randint(1, 6, a.shape, generator=g).double(), a)
    # weight codes: integers in -16 .. 16
    w = torch.randint(-16, 17, (Cout, R, R, Cin), generator=g).double()
    Krow = R * R * Cin
    for o in range(Cout):
        nnz = _KINDS[o % 8][0]
        if nnz is not None:
            keep = torch.zeros(Krow, dtype=torch.bool)
            keep[torch.randperm(Krow, generator=g)[:nnz]] = True
            w[o] = torch.where(keep.view(R, R, Cin), torch.where(w[o] == 0, torch.ones_like(w[o]), w[o]), torch.zeros_like(w[o]))
    ein = int(torch.randint(1, 4, (1,), generator=g))                 # s_in = 2, 4 or 8
    s_in = 2.0 ** ein
    eout = -int(torch.randint(1, 3, (1,), generator=g))               # out_inv_scale = 1/2 or 1/4
    out_inv = 2.0 ** eout if out_kind == "f8" else 1.0
    acc = conv_f64(a, w, 1, pad, 1)
    sigma = acc.flatten(0, 2).std(dim=0).clamp(min=1.0)               # per channel
    exps, bias = torch.zeros(Cout), torch.zeros(Cout)
    for o in range(Cout):
        _, target, e, has_bias = _KINDS[o % 8]
        if target is not None:
            e = int(torch.round(torch.log2(torch.tensor(target / out_inv) / sigma[o])))
        exps[o] = e - (o // 8) % 2
        if has_bias:
            b = int(torch.randint(1, 17, (1,), generator=g))
            bias[o] = b if int(torch.randint(0, 2, (1,), generator=g)) else -b
    scale = torch.pow(2.0, exps.double()).float()
    x = (a * s_in).to(BF16) if in_kind == "bf16" else a.float().to(FP8)
    assert torch.equal(x.double(), a * (s_in if in_kind == "bf16" else 1.0))
    wq = w.float().to(FP8)
    assert torch.equal(wq.double(), w)
    return SimpleNamespace(shape=tuple(shape), pad=pad, in_kind=in_kind, out_kind=out_kind, relu=int(relu), a=a, w=w, x=x, wq=wq,
                           in_scale=s_in, out_scale=(1.0 / out_inv) if out_kind == "f8" else None, out_inv=out_inv, scale=scale,
                           bias=bias.float(), acc=acc, _absacc=None)


_CASES = {}


def conv_case(key):
    """the case of one case_keys() entry, built once per process and never modified"""
    if key not in _CASES:
        shape, ik, ok, relu = key
        _CASES[key] = make_case(shape, ik, ok, relu, seed=sum(shape) + 7 * len(ik) + 3 * len(ok) + relu)
    return _CASES[key]


def check_exact(case):
    """asserts the condition of the theorem, per channel: every partial sum below 2^24, (bound / g)[o] < 2^24 with g[o] the
    common granularity of channel o's epilogue terms, and a bf16 output inside bf16's range.  Returns max bound / g."""
    if case._absacc is None:
        case._absacc = conv_f64(case.a.abs(), case.w.abs(), 1, case.pad, 1).flatten(0, 2).max(dim=0).values
    absacc = case._absacc
    assert float(absacc.max()) < LIMIT, "accumulator not exact: %g" % float(absacc.max())
    sc = case.scale.double()
    bound = absacc * sc + case.bias.double().abs()
    gran = torch.minimum(sc, torch.ones_like(sc))
    ratio = float((bound / gran).max())
    assert ratio < LIMIT, "not exact in f32: bound / g = %g >= 2^24" % ratio
    v = case.acc * sc + case.bias.double()
    assert torch.equal(v.float().double(), v)
    q = v * case.out_inv
    assert torch.equal(q.float().double(), q) and float(q.abs().max()) < 3e38
    return ratio


def _quant(q, trunc=False, saturate=True):
    """float64 (exactly f32) -> e4m3fn: clamp, one round-to-nearest-even conversion (trunc: towards zero, a planted fault)"""
    if saturate:
        q = q.clamp(-FP8_MAX, FP8_MAX)
    r = q.float().to(FP8)
    if not trunc:
        return r
    over = r.double().abs() > q.abs()          # rounded away from zero: one code back in sign-magnitude order
    return (r.view(torch.uint8) - over.to(torch.uint8)).view(FP8)


def _conv_wrapping(a, w, pad):
    """the 3x3 conv whose taps address the image as one flat row of pixels: a tap that leaves the row on the left or right
    reads the neighbouring row's pixel instead of zero (taps above / below the image still read zero)"""
    N, H, W, C = a.shape
    R = w.shape[1]
    flat = torch.cat([torch.zeros(N, (pad + 1) * W, C, dtype=a.dtype), a.reshape(N, H * W, C),
                      torch.zeros(N, (pad + 1) * W, C, dtype=a.dtype)], dim=1)
    acc = torch.zeros(N, H * W, w.shape[0], dtype=torch.float64)
    for r in range(R):
        for s in range(R):
            off = (pad + 1) * W + (r - pad) * W + (s - pad)
            acc += flat[:, off:off + H * W] @ w[:, r, s].t()
    return acc.reshape(N, H, W, -1)


def pre_rounding(case, fault=None):
    """(q, q_before_relu): the float64 values handed to the output conversion (after ReLU and out_inv_scale) and the same
    before ReLU"""
    N, H, W, Cin, Cout, R = case.shape
    a, w, acc, scale = case.a, case.w, case.acc, case.scale.double()
    if fault == "k_permuted":                  # A's 32 codes of a lane fragment reversed, B's not
        a = a.reshape(N, H, W, Cin // 32, 32).flip(-1).reshape(N, H, W, Cin)
        acc = conv_f64(a, w, 1, case.pad, 1)
    elif fault == "pad_wraps_row":
        acc = _conv_wrapping(a, w, case.pad)
    elif fault == "drop_last_kstep":
        w = w.clone()
        w[:, R - 1, R - 1, Cin - 128:] = 0
        acc = conv_f64(a, w, 1, case.pad, 1)
    elif fault == "fnuz_bias":                 # the weight codes read with an exponent bias of 8: every product halves
        acc = acc * 0.5
    elif fault == "per_tensor_wscale":
        scale = torch.full_like(scale, float(scale.max()))
    v = acc * scale + case.bias.double()
    if fault == "transposed_out":              # every full 32 x 32 fragment of the [M][Cout] result transposed
        M = N * H * W
        v2 = v.reshape(M, Cout).clone()
        mb = M // 32 * 32
        blk = v2[:mb].reshape(M // 32, 32, Cout // 32, 32).transpose(1, 3)
        v2[:mb] = blk.reshape(mb, Cout)
        v = v2.reshape(N, H, W, Cout)
    q0 = v * case.out_inv
    q = q0.clamp(min=0) if case.relu and fault != "relu_after_quant_sign" else q0
    return q, q0


def reference(case, fault=None):
    """the conv's output, byte for byte: float8_e4m3fn codes or bf16 [N,H,W,Cout]"""
    q, _ = pre_rounding(case, fault)
    trunc = fault == "truncate"
    if case.out_kind == "f8":
        y = _quant(q, trunc=trunc, saturate=fault != "no_saturate")
        if fault == "relu_after_quant_sign" and case.relu:      # "ReLU" on the codes by clearing the sign bit
            y = (y.view(torch.uint8) & 0x7f).view(FP8)
        return y
    y = convert(q, BF16, trunc=trunc)
    if fault == "relu_after_quant_sign" and case.relu:
        y = (y.view(torch.int16) & 0x7fff).view(BF16)
    return y


def fault_applies(case, fault):
    return {"no_saturate": case.out_kind == "f8", "pad_wraps_row": case.shape[5] == 3,
            "relu_after_quant_sign": bool(case.relu)}.get(fault, True)


def rounding_shares(case):
    """share of the elements of an fp8-output case in each class of CLASSES, judged on the pre-rounding value q"""
    q, q0 = pre_rounding(case)
    inr = q.abs() <= FP8_MAX
    near = _quant(q).double()
    low = _quant(q, trunc=True)
    lowd = low.double()
    inexact = inr & (near != q)
    high = (low.view(torch.uint8) + 1).view(FP8).double()               # the neighbour away from zero (q inexact: below 448)
    tie = inexact & ((q - lowd).abs() == (high - q).abs())
    low_even = (low.view(torch.uint8) & 1) == 0
    d = {"exact": inr & (near == q) & (q != 0), "up": inexact & ~tie & (near.abs() > q.abs()),
         "down": inexact & ~tie & (near.abs() < q.abs()), "tie_to_even_below": tie & low_even, "tie_to_even_above": tie & ~low_even,
         "sat_hi": q > FP8_MAX, "sat_lo_before_relu": q0 < -FP8_MAX, "subnormal": (q != 0) & (q.abs() < 2.0 ** -6)}
    return {k: v.double().mean().item() for k, v in d.items()}


def assert_codes_equal(got, want, what):
    """got == want as bytes, the zero codes 0x80 and 0x00 taken as equal (fp8 codes), or as int16 with -0 == +0 (bf16)"""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s against %s %s" % (
        what, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
    if got.dtype == FP8:
        gi, wi = got.view(torch.uint8).clone(), want.view(torch.uint8).clone()
        gi[gi == 0x80] = 0
        wi[wi == 0x80] = 0
    else:
        gi, wi = got.view(torch.int16).clone(), want.view(torch.int16).clone()
        gi[gi == -32768] = 0
        wi[wi == -32768] = 0
    diff = gi != wi
    nd = int(diff.sum())
    if nd == 0:
        return
    idx = tuple(int(i) for i in diff.nonzero()[0])
    raise AssertionError("%s: %d of %d elements differ; first at %s: got %r (bits %d), want %r (bits %d)" % (
        what, nd, got.numel(), idx, float(got[idx].float()), int(gi[idx]), float(want[idx].float()), int(wi[idx])))
