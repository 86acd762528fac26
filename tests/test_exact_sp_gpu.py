"""-m gpu: the split-precision (SP) conv family against a truth without tolerance -- section h of tests/test_exact_conv_gpu.py,
grown into its own file.

The SP kernels (igemm8_kernel<.., SP = 1, ..> behind mega_conv2d_nhwc_sp_dt: ops.conv2d_sp, linear_sp, linear_transposed_x3,
X3Weight, Bottleneck.run_sp) serve the x3, wide and h2 rows of CONV_MODES.  tests/exact_conv_cases.py builds integer-valued
operands for which the f32 accumulation is exact in any order; what is left are the roundings the operand forms DOCUMENT -- the
hi / lo splits of activations, weights, residual and output, one fp16 rounding of an h2 weight, one conversion of a plain
output -- and the float64 reference performs exactly those.  A correct kernel equals it BIT FOR BIT
(tests/test_exact_conv_cases.py checks the conditions, and that the comparison rejects ten planted faults, on the CPU).

ec.SP_TABLE lists the cases: every operand form (x3, h2, hi from planes, hi from a plain tensor), both launch classes at 192 and
at 256 rows, every output mode with and without a residual, the caller's out= buffer, the three activations, the narrow and
ragged Cout, 3x3 / dilated / stride-2 geometry.  Every test first asserts the launch class and row count its case is meant for,
from mega_conv2d_nhwc_sp_plan -- the function the launch itself uses.  No number in this file is a tolerance."""
import pytest
import torch

import exact_conv_cases as ec
from exact_conv_cases import BF16, F16, F32, assert_bits_equal

pytestmark = pytest.mark.gpu

_MODE = {"plain": 0, "planes": 1, "f32": 2}
_OPS_MODE = {"plain": "bf16", "planes": "planes", "f32": "f32"}      # (ops.conv2d_sp calls the plain 16-bit output "bf16")
SENTINEL = -7.0


def _ops():
    from mega.pytorch_amd import ops
    return ops


def _lib():
    from mega.pytorch_amd import _lib
    return _lib.load()


def _sp_plan(M, Cout, K, taps, out_mode, has_ws=0):
    t = _lib().mega_conv2d_nhwc_sp_plan(M, Cout, K, taps, _MODE[out_mode], has_ws)
    return t // 1000000, t % 1000000 // 1000, t % 1000


def _weight(case):
    ops = _ops()
    if case.form == "x3":
        return ops.split_conv_weight_x3(case.w)
    if case.form == "h2":
        return ops.split_conv_weight_h2(case.w)
    return case.w.to(case.pdt)


def _planes(dev, v, T):
    return None if v is None else _ops().split_planes(v.to(dev), T)


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("row", ec.SP_TABLE, ids=[r[0] for r in ec.SP_TABLE])
def test_conv2d_sp_table_exact(dev, row):
    name, shape, form, wide_w, relu, use_res, out_mode, pad_cols, kind, rows, knobs = row
    N, H, W, Cin, Cout, R, stride, pad, dil = shape
    case = ec.sp_table_case(row)
    M, _, K, taps = ec.sp_gemm_shape(shape, form)
    assert _sp_plan(M, Cout, K, taps, out_mode) == (kind, rows, 256), name
    want, _ = ec.reference_sp(case, out_mode)
    T = case.pdt
    x = case.x.to(T).to(dev) if case.plain_x else _planes(dev, case.x, T)
    out = None
    if pad_cols:
        out = torch.full((M, Cout + pad_cols), SENTINEL, dtype=F32 if out_mode == "f32" else T, device=dev)
    y = _ops().conv2d_sp(x, _weight(case).to(dev), case.scale.to(dev), case.bias.to(dev), residual=_planes(dev, case.res, T),
                         stride=stride, pad=pad, dil=dil, relu=relu, out_mode=_OPS_MODE[out_mode], operands=case.form, out=out)
    if out_mode == "planes":
        y = y.t
    if pad_cols:
        y = y.cpu()
        it = torch.int32 if y.dtype == F32 else torch.int16
        assert bool((y[:, Cout:].contiguous().view(it) == torch.full((1,), SENTINEL, dtype=y.dtype).view(it)).all()), \
            name + ": written behind column Cout"
        y = y[:, :Cout].contiguous().view(want.shape)
    assert_bits_equal(y, want, "conv2d_sp %s %s -> %s" % (name, shape, out_mode), relu=relu, tile=(rows, 256))


# ------------------------------------------------------------------------------------------------ split-K
@pytest.mark.parametrize("form", ["x3", "h2"])
def test_linear_sp_split_k_exact(dev, form):
    """R S Cw >= 32768: the library's rule splits K three ways, the SP kernels write raw partial sums (matrix class) and the
    finalize kernel applies bias and ReLU"""
    ops = _ops()
    case = ec.sp_splitk_case(form)
    M, K, Nout = ec.SP_SPLITK[form]
    Kk = ec.SP_FORMS[form][1] * K
    assert Kk >= 32768 and _lib().mega_conv2d_nhwc_workspace_bytes(M, Nout, Kk) == 3 * M * Nout * 4
    assert _sp_plan(M, Nout, Kk, 1, "f32", has_ws=1) == (8, 192, 256)
    want, _ = ec.reference_sp(case, "f32")
    assert bool((case.scale == 1).all())
    xp = _planes(dev, case.x.view(M, K), case.pdt)
    got = ops.linear_sp(xp, _weight(case).view(Nout, Kk).to(dev), case.bias.to(dev), relu=True, operands=form)
    assert_bits_equal(got.view(want.shape), want, "linear_sp split-K %s" % form, relu=1)


# ------------------------------------------------------------------------------------------------ the wrappers
def test_x3weight_linear_exact(dev):
    """ops.linear with an X3Weight: split_planes + linear_sp on the packed [Wh | Wh | Wl]"""
    ops = _ops()
    M, K, Nout, ld = ec.SP_LINEAR_T
    case = ec.sp_linear_case(True)
    assert _sp_plan(M, Nout, 3 * K, 1, "f32") == (8, 192, 256)
    want, _ = ec.reference_sp(case, "f32")
    w = ops.X3Weight(case.w.view(Nout, K), dev)
    wh, wl = ec.split_hi_lo(case.w.view(Nout, K))
    assert_bits_equal(w.w3, torch.cat([wh, wh, wl], dim=-1), "X3Weight.w3")
    got = ops.linear(case.x.view(M, K).to(dev), w, case.bias.to(dev))
    assert_bits_equal(got.view(want.shape), want, "ops.linear(X3Weight)")


def test_linear_transposed_x3_exact(dev):
    """ops.linear_transposed with an X3Weight at M = 37, ld = 64: the weight rows are the GEMM's A operand in the "hi" form, the
    activations [xh | xl | xh] its B operand (mega_split_f32_to_bf16x3, three zero pad rows up to M8 = 40), f32 into the caller's
    [Nout, ld] buffer: the same three terms, so the reference transposed; pad columns exactly zero"""
    ops = _ops()
    M, K, Nout, ld = ec.SP_LINEAR_T
    case = ec.sp_linear_case(False)
    assert _sp_plan(Nout, (M + 7) // 8 * 8, 3 * K, 1, "f32") == (8, 192, 256)
    want, _ = ec.reference_sp(case, "f32")
    assert bool((case.scale == 1).all()) and bool((case.bias == 0).all())
    x = case.x.view(M, K).to(dev)
    xh, xl = ec.split_hi_lo(case.x.view(M, K))
    assert_bits_equal(ops.split_bf16x3(x), torch.cat([xh, xl, xh], dim=-1), "split_bf16x3")
    got = ops.linear_transposed(ops.X3Weight(case.w.view(Nout, K), dev), x, ld).cpu()
    assert got.shape == (Nout, ld) and got.dtype == F32
    assert bool((got[:, M:].contiguous().view(torch.int32) == 0).all()), "pad columns are not zero"
    assert_bits_equal(got[:, :M].t().contiguous().view(want.shape), want, "ops.linear_transposed(X3Weight)")


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_split_planes_exact(dev, dtype):
    """split_planes equals the CPU split bit for bit: a table input (13-bit integers) and a block input, as planes of both types"""
    for v in (ec.sp_table_case(ec.SP_TABLE[3]).x, ec.sp_block_case(ec.SP_BLOCKS[0]).x):
        p = _ops().split_planes(v.to(dev), dtype)
        assert p.dtype == dtype and p.C == v.shape[-1]
        assert_bits_equal(p.t, torch.cat(ec.split_hi_lo(v, dtype), dim=-1), "split_planes(%s) %s" % (dtype, tuple(v.shape)))


# ------------------------------------------------------------------------------------------------ Bottleneck.run_sp
def _block(case, mode):
    from mega.pytorch_amd import modeling
    Cin, mid, Cout, stride, dil, ds = ec.SP_BLOCK_KINDS[case.kind]
    blk = modeling.Bottleneck(Cin, mid, Cout, stride, dilation=dil, mode=modeling.CONV_MODES[mode])
    assert (blk.downsample is not None) == ds
    convs = [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2), (blk.conv3, blk.bn3)] + ([tuple(blk.downsample)] if ds else [])
    with torch.no_grad():
        for (conv, bn), w, (sc, bi) in zip(convs, case.w, case.sb):
            conv.weight.copy_(w.permute(0, 3, 1, 2))             # OHWI -> OIHW
            bn.weight.copy_(sc)                                  # running_mean 0, running_var 1: folded() = (scale, bias)
            bn.bias.copy_(bi)
            s, b = bn.folded()
            assert torch.equal(s, sc) and torch.equal(b, bi)
    blk.invalidate()
    return blk


# (only the "trunk" mode feeds a block a plain tensor)
BLOCK_RUNS = [(spec, mode) for spec in ec.SP_BLOCKS for mode in ("x3", "h2", "wide") if mode == "wide" or not spec[2]]


@pytest.mark.parametrize("plain_out", [False, True], ids=["planes", "plain"])
@pytest.mark.parametrize("spec,mode", BLOCK_RUNS, ids=["%s%s-%s" % (s[0], "-plain-x" if s[2] else "", m) for s, m in BLOCK_RUNS])
def test_bottleneck_run_sp_exact(dev, spec, mode, plain_out):
    """modeling.Bottleneck.run_sp on the integer block: which plane goes where, the downsample's stride on planes, the identity
    as planes, the mode's hand-off between the layers; out_mode "planes" and the mode's plain output"""
    from mega.pytorch_amd import modeling, ops
    kind, hw, plain_x = spec
    case = ec.sp_block_case(spec)
    m = modeling.CONV_MODES[mode]
    form, T, plain = ec.SP_BLOCK_MODES[mode]
    assert (m.operands, m.plane_dtype) == (form, T)
    want, _, _ = ec.reference_sp_block(case, mode, plain_out)
    # the SP launches of the block: 1x1 convs of K = (blocks of the form) x Cin, streaming class up to K = 512, 192 rows
    Cin, mid, Cout, stride, dil, ds = ec.SP_BLOCK_KINDS[kind]
    N, H, W = hw
    s = 1 if dil > 1 else stride
    Mo = N * ((H - 1) // s + 1) * ((W - 1) // s + 1)
    kmul = ec.SP_FORMS[form][1]
    launches = [(mid, kmul * Cin, "planes" if plain is None else "plain"), (Cout, kmul * mid, "plain" if plain_out else "planes")]
    launches += [(Cout, kmul * Cin, "planes")] if ds else []
    for co, K, om in launches:
        assert _sp_plan(Mo, co, K, 1, "f32" if (om == "plain" and plain is None) else om) == (7 if K <= 512 else 8, 192, 256)
    blk = _block(case, mode)
    x = case.x.to(T).to(dev) if plain_x else ops.split_planes(case.x.to(dev), T)
    y = blk.run_sp(x, out_mode=m.plain if plain_out else "planes")
    assert isinstance(y, ops.Planes) != plain_out
    assert_bits_equal(y if plain_out else y.t, want, "Bottleneck.run_sp %s %s %s" % (kind, mode, "plain" if plain_out else "planes"),
                      relu=1)
