"""-m gpu: the conv kernel family against a truth without tolerance.

tests/exact_conv_cases.py builds integer-valued operands (power-of-two FrozenBN scales, integer bias and residual) for which
the f32 accumulation is exact in any order and the only rounding is the one nearest-even conversion to the output type; a correct
kernel equals the float64 reference BIT FOR BIT (tests/test_exact_conv_cases.py checks those conditions, and that the comparison
catches planted faults, on the CPU).  Every assertion here is assert_bits_equal against that reference: the register-staged tiles,
igemm8 (matrix and streaming class, 256 and 192 rows), conv64, the two fused bottlenecks, split-K + finalize, the sub-pixel
deconvolution, the four stem entry points and two small x3 cases of the split-precision kernels.  No number in this file is a
tolerance.

A new conv-family kernel or dispatch class adds its shapes here (testing).  The split-precision family -- every
operand form (x3, h2, hi), launch class and row count, output mode, split-K, the X3Weight wrappers and Bottleneck.run_sp -- has
its own table in tests/test_exact_sp_gpu.py, which grew out of section h below."""
import pytest
import torch

import exact_conv_cases as ec
from exact_conv_cases import BF16, F16, F32, assert_bits_equal

pytestmark = pytest.mark.gpu


def _ops():
    from mega.pytorch_amd import ops
    return ops


def _lib():
    from mega.pytorch_amd import _lib
    return _lib.load()


def _plan(case):
    """(kind, BM, BN) the launch path's own rule gives this case under the current MEGA_IGEMM_TILE"""
    from mega.pytorch_amd.ops import _DT
    N, H, W, Cin, Cout, R, stride, pad, dil = case.shape
    t = _lib().mega_conv2d_nhwc_plan_ex(N, H, W, Cin, Cout, R, R, stride, pad, dil, Cout, int(case.res is not None),
                                        _DT[case.dtype], _DT[case.out_dtype])
    return t // 1000000, t % 1000000 // 1000, t % 1000


def _conv(dev, case, **kw):
    N, H, W, Cin, Cout, R, stride, pad, dil = case.shape
    return _ops().conv2d_nhwc(case.x.to(dev), case.w.to(dev), case.scale.to(dev), case.bias.to(dev),
                              None if case.res is None else case.res.to(dev), stride=stride, pad=pad, dil=dil, relu=case.relu,
                              out_dtype=case.out_dtype, **kw)


def _check(dev, case, what, plan=None, **kw):
    want, _ = ec.reference(case)
    got = _conv(dev, case, **kw)
    assert_bits_equal(got, want, "%s %s %s->%s" % (what, case.shape, case.dtype, case.out_dtype), relu=case.relu,
                      tile=None if plan is None else plan[1:])


# ------------------------------------------------------------------------------------------------ a. register-staged tiles
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("tile", ["64x64", "128x64", "128x128", "256x128", "256x256"])
def test_register_staged_tile_exact(dev, tile, dtype, monkeypatch):
    monkeypatch.setenv("MEGA_IGEMM_TILE", tile)
    bm, bn = (int(v) for v in tile.split("x"))
    for shape, relu, use_res, f32o in ec.TILE_CASES:
        case = ec.conv_case(shape, dtype, F32 if f32o else dtype, relu, use_res)
        plan = _plan(case)
        assert plan == (0, bm, bn), (shape, plan)
        _check(dev, case, "tile " + tile, plan)


# ------------------------------------------------------------------------------------------------ b. igemm8
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("force", ["8:256", "8:192"])
def test_igemm8_forced_exact(dev, force, dtype, monkeypatch):
    monkeypatch.setenv("MEGA_IGEMM_TILE", force)
    rows = int(force[2:])
    for shape, relu, use_res, f32o in ec.IGEMM8_CASES:
        case = ec.conv_case(shape, dtype, F32 if f32o else dtype, relu, use_res)
        plan = _plan(case)
        assert plan[0] in (7, 8) and plan[1:] == (rows, 256), (shape, plan)
        assert (plan[0] == 7) == (shape[5] == 1 and shape[3] <= 512)       # streaming class: 1x1, K <= 512
        _check(dev, case, "igemm8 " + force, plan)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("spec", ec.NATURAL_CASES, ids=["matrix", "streaming"])
def test_igemm8_natural_dispatch_exact(dev, spec, dtype, monkeypatch):
    monkeypatch.delenv("MEGA_IGEMM_TILE", raising=False)
    shape, relu, use_res, kind = spec
    case = ec.conv_case(shape, dtype, dtype, relu, use_res)
    plan = _plan(case)
    print("natural dispatch %s %s: kind %d, tile %dx%d" % (shape, dtype, plan[0], plan[1], plan[2]))
    assert plan[0] == kind and plan[2] == 256 and plan[1] in (192, 256), plan
    _check(dev, case, "igemm8 natural kind %d" % kind, plan)


# ------------------------------------------------------------------------------------------------ c. conv64
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_conv64_exact(dev, dtype, monkeypatch):
    monkeypatch.delenv("MEGA_IGEMM_TILE", raising=False)
    for relu in (1, 0, 2):
        case = ec.conv_case(ec.CONV64_SHAPE, dtype, dtype, relu, False)
        plan = _plan(case)
        print("natural dispatch %s %s: kind %d, tile %dx%d" % (case.shape, dtype, plan[0], plan[1], plan[2]))
        assert plan[0] == 6, plan
        _check(dev, case, "conv64 relu=%d" % relu)


# ------------------------------------------------------------------------------------------------ d. fused bottlenecks
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("ds", [False, True], ids=["identity", "downsample"])
@pytest.mark.parametrize("hw", ec.BOTTLENECK_SIZES)
def test_fused_bottleneck_exact(dev, hw, ds, dtype):
    ops = _ops()
    case = ec.bottleneck_case(hw, dtype, ds)
    want, _ = ec.reference_bottleneck(case)
    args = [case.x.to(dev)]
    for i in range(3):
        args += [case.w[i].to(dev), case.sb[i][0].to(dev), case.sb[i][1].to(dev)]
    if ds:
        got = ops.bottleneck64_ds(*args, case.w[3].to(dev), case.sb[3][0].to(dev), case.sb[3][1].to(dev))
    else:
        got = ops.bottleneck64(*args)
    assert_bits_equal(got, want, "bottleneck64%s %s %s" % ("_ds" if ds else "", hw, dtype), relu=1)


# ------------------------------------------------------------------------------------------------ e. split-K
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_linear_library_split_k_exact(dev, dtype, monkeypatch):
    """K >= 32768: the library's own rule splits K three ways and the finalize kernel applies scale, bias and ReLU"""
    monkeypatch.delenv("MEGA_IGEMM_TILE", raising=False)
    case = ec.conv_case(ec.LINEAR_SPLITK_SHAPE, dtype, dtype, 1, False)
    M, _, _, K, Cout = case.shape[:5]
    assert _lib().mega_conv2d_nhwc_workspace_bytes(M, Cout, K) == 3 * M * Cout * 4
    want, _ = ec.reference(case)
    got = _ops().linear(case.x.view(M, K).to(dev), case.w.view(Cout, K).to(dev), case.bias.to(dev), relu=True,
                        scale=case.scale.to(dev))
    assert_bits_equal(got.view(M, 1, 1, Cout), want, "linear split-K %s" % dtype, relu=1)


@pytest.mark.parametrize("dtype,out_dtype", [(F32, F32), (BF16, BF16), (F16, F16), (BF16, F32)],
                         ids=["f32", "bf16", "f16", "bf16-f32out"])
def test_caller_split_k_exact(dev, dtype, out_dtype, monkeypatch):
    """the caller's count (4), a count clamp_ksplit reduces through its loop (10 -> 9 ranges of the 72 bf16 K-tiles) and one far
    past the K-tile count; LeakyReLU and the residual in the finalize kernel"""
    monkeypatch.delenv("MEGA_IGEMM_TILE", raising=False)
    from mega.pytorch_amd.ops import _DT
    case = ec.conv_case(ec.CALLER_SPLITK_SHAPE, dtype, out_dtype, 2, True)
    want, _ = ec.reference(case)
    M, Cout, K = want.numel() // want.shape[-1], want.shape[-1], 9 * case.shape[3]
    nkt = K // (32 if dtype == F32 else 64)
    ranges = {}
    for ks in (4, 10, 1000):
        ranges[ks] = _lib().mega_conv2d_nhwc_ks_workspace_bytes(M, Cout, K, _DT[dtype], ks) // (M * Cout * 4)
        got = _conv(dev, case, ksplit=ks)
        assert_bits_equal(got, want, "caller split-K %d (%d ranges) %s->%s" % (ks, ranges[ks], dtype, out_dtype), relu=2)
    assert ranges[4] == 4 and ranges[1000] == nkt and ranges[10] == (10 if dtype == F32 else 9), ranges


# ------------------------------------------------------------------------------------------------ f. sub-pixel deconvolution
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", ec.DECONV_SHAPES)
def test_deconv_subpixel_exact(dev, shape, dtype):
    """deconv4x4s2_into with crop 0 (the full map) and crop 1, one and two K ranges, into the channel slice [Cs, Cs + C) of a
    sentinel-filled concatenation buffer: the slice equals the integer conv_transpose2d reference, nothing else is written"""
    ops = _ops()
    N, H, W, Cin, C, Cs = shape
    case = ec.deconv_case(shape, dtype)
    mult = 32 if dtype == F32 else 64
    cp = (Cin + mult - 1) // mult * mult
    xp = torch.zeros((N, H, W, cp), dtype=dtype)
    xp[..., :Cin] = case.x
    w4 = ops.pack_deconv4x4s2(case.wt, dtype, mult)
    ldo = (Cs + C + 2 + mult - 1) // mult * mult
    it = torch.int32 if dtype == F32 else torch.int16
    for (H2, W2) in ((2 * H + 2, 2 * W + 2), (2 * H + 1, 2 * W)):
        want, _ = ec.reference_deconv(case, 2, H2, W2)
        for ks in (1, 2):
            out = torch.full((N, H2, W2, ldo), -7.0, dtype=dtype, device=dev)
            ops.deconv4x4s2_into(xp.to(dev), w4.to(dev), case.bias.repeat(4).to(dev), out, Cs, relu=2, ksplit=ks)
            got = out.cpu()
            what = "deconv %s %s target %dx%d ksplit %d" % (shape, dtype, H2, W2, ks)
            assert_bits_equal(got[..., Cs:Cs + C].contiguous(), want, what, relu=2)
            sentinel = torch.full((1,), -7.0, dtype=dtype).view(it)
            assert bool((got[..., :Cs].contiguous().view(it) == sentinel).all()), what + ": written below the slice"
            assert bool((got[..., Cs + C:].contiguous().view(it) == sentinel).all()), what + ": written above the slice"


# ------------------------------------------------------------------------------------------------ g. stem
@pytest.mark.parametrize("hw", ec.STEM_SIZES)
def test_stem_entry_points_exact(dev, hw):
    """the direct f32 stem, the bf16 matrix-core stem, stem_u8 (both channel orders) and stem_pool (u8 and f32 input, bf16 and
    f16) against the stem reference: integer mean, zero padding applied after the mean is subtracted"""
    ops = _ops()
    case = ec.stem_case(hw)
    u8, sc, bi = case.u8.to(dev), case.scale.to(dev), case.bias.to(dev)
    wt = case.w.permute(1, 2, 3, 0).reshape(147, 64).contiguous().to(dev)
    w160 = {dt: ops.pack_stem_weight_bf16(case.w, dt).to(dev) for dt in (BF16, F16)}
    img = ec.stem_image(case, True).to(dev)
    want32, _ = ec.reference_stem(case, F32, True)
    assert_bits_equal(ops.stem(img, wt, sc, bi, F32), want32, "stem f32 direct %s" % (hw,), relu=1)
    want16, _ = ec.reference_stem(case, BF16, True)
    assert_bits_equal(ops.stem(img, wt, sc, bi, BF16), want16, "stem direct, bf16 output %s" % (hw,), relu=1)
    assert_bits_equal(ops.stem(img, wt, sc, bi, BF16, w_n160=w160[BF16]), want16, "stem bf16 matrix-core %s" % (hw,), relu=1)
    for to_bgr in (True, False):
        want, _ = ec.reference_stem(case, BF16, to_bgr)
        assert_bits_equal(ops.stem_u8(u8, w160[BF16], sc, bi, case.mean, to_bgr), want, "stem_u8 to_bgr=%s %s" % (to_bgr, hw), relu=1)
        for dt in (BF16, F16):
            wantp, _ = ec.reference_stem(case, dt, to_bgr, pool=True)
            assert_bits_equal(ops.stem_pool(u8, w160[dt], sc, bi, case.mean, to_bgr), wantp,
                              "stem_pool u8 to_bgr=%s %s %s" % (to_bgr, dt, hw), relu=1)
    for dt in (BF16, F16):
        wantp, _ = ec.reference_stem(case, dt, True, pool=True)
        assert_bits_equal(ops.stem_pool(img, w160[dt], sc, bi), wantp, "stem_pool f32 input %s %s" % (dt, hw), relu=1)


# ------------------------------------------------------------------------------------------------ h. split precision
@pytest.mark.parametrize("out_mode", ["f32", "planes"])
@pytest.mark.parametrize("spec", ec.SP_CASES, ids=["3x3-small-w", "1x1-wide-w"])
def test_conv2d_sp_x3_exact(dev, spec, out_mode):
    """conv2d_sp(operands="x3"): the documented contraction x_hi.Wh + x_lo.Wh + x_hi.Wl, x up to 4096 (the lo plane is used), weights
    whose lo part is zero / non-zero; ops.split_planes and the weight packing equal the CPU split bit for bit"""
    ops = _ops()
    shape, wide, relu, use_res = spec
    N, H, W, Cin, Cout, R, stride, pad, dil = shape
    case = ec.sp_case(spec)
    xp = ops.split_planes(case.x.to(dev))
    assert_bits_equal(xp.t, torch.cat(ec.split_hi_lo(case.x), dim=-1), "split_planes(x) %s" % (shape,))
    wh, wl = ec.split_hi_lo(case.w)
    w3 = ops.split_conv_weight_x3(case.w)
    assert_bits_equal(w3, torch.cat([wh, wh, wl], dim=-1), "split_conv_weight_x3 %s" % (shape,))
    rp = None
    if use_res:
        rp = ops.split_planes(case.res.to(dev))
        assert_bits_equal(rp.t, torch.cat(ec.split_hi_lo(case.res), dim=-1), "split_planes(residual) %s" % (shape,))
    want, _ = ec.reference_sp(case, out_mode)
    y = ops.conv2d_sp(xp, w3.to(dev), case.scale.to(dev), case.bias.to(dev), residual=rp, stride=stride, pad=pad, dil=dil,
                      relu=relu, out_mode=out_mode, operands="x3")
    assert_bits_equal(y.t if out_mode == "planes" else y, want, "conv2d_sp x3 %s -> %s" % (shape, out_mode), relu=relu)
