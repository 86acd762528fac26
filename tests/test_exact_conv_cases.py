"""The integer-valued conv cases of tests/exact_conv_cases.py, checked on the CPU before the GPU file trusts them:
(1) every case meets the exactness condition and torch's f32 convolution equals the float64 one bit for bit (the accumulation
order cannot matter); (2) the output conversion really rounds, ties included; (3) assert_bits_equal catches four planted faults
in every case.  Each test prints its figures (run with -s to see them)."""
import pytest
import torch
import torch.nn.functional as F

import exact_conv_cases as ec

CONV_KEYS = ec.all_conv_cases()
FAULTS = ("drop_x", "move_w", "swap_bias", "trunc")


def _id(key):
    shape, dt, odt, relu, res = key
    return "%s-%s-%s-act%d%s" % ("x".join(str(v) for v in shape), str(dt)[6:], str(odt)[6:], relu, "-res" if res else "")


def _pre_conversion(case):
    v = case.acc * case.scale.double() + case.bias.double()
    if case.res is not None:
        v = v + case.res.double()
    return ec.activation(v, case.relu)


@pytest.mark.parametrize("key", CONV_KEYS, ids=_id)
def test_case_is_exact_and_f32_conv_equals_f64(key):
    case = ec.conv_case(*key)
    N, H, W, Cin, Cout, R, stride, pad, dil = case.shape
    for t in (case.x, case.w) + ((case.res,) if case.res is not None else ()):
        assert t.dtype == case.dtype and torch.equal(t.double(), t.double().round())       # integers, held exactly
    assert torch.equal(case.scale.log2(), case.scale.log2().round()) and torch.equal(case.bias, case.bias.round())
    assert case.scale.unique().numel() > 1 and case.bias.unique().numel() > 2             # they vary per channel
    ratio = ec.check_exact(case)
    acc32 = F.conv2d(case.x.float().permute(0, 3, 1, 2), case.w.float().permute(0, 3, 1, 2), stride=stride, padding=pad,
                     dilation=dil).permute(0, 2, 3, 1)
    assert torch.equal(acc32.double(), case.acc), "f32 accumulation is not exact on this case"
    rounded, ties = ec.rounding_shares(_pre_conversion(case), case.out_dtype)
    print("%s: bound / g = %.4g (< 2^24 = %.4g), rounded %.1f %%, ties %.1f %%" % (_id(key), ratio, ec.LIMIT, 100 * rounded,
                                                                                 100 * ties))
    if case.out_dtype != torch.float32:
        assert rounded > 0, "the output conversion never rounds on this case"


@pytest.mark.parametrize("odt", [torch.bfloat16, torch.float16])
def test_output_rounding_is_exercised(odt):
    """for each 16-bit output type at least one case has >= 10 % of its outputs not representable and >= 5 % exact ties (where
    nearest-even and half-away differ)"""
    best = (0.0, 0.0, None)
    for key in CONV_KEYS:
        if key[2] == odt:
            r, t = ec.rounding_shares(_pre_conversion(ec.conv_case(*key)), odt)
            if r >= 0.10 and t >= 0.05 and t > best[1]:
                best = (r, t, key)
    print("%s: best case %s: rounded %.1f %%, ties %.1f %%" % (odt, best[2] and _id(best[2]), 100 * best[0], 100 * best[1]))
    assert best[2] is not None


@pytest.mark.parametrize("key", CONV_KEYS, ids=_id)
def test_planted_faults_are_detected(key):
    """the reference recomputed with one fault at a time must differ from the true one under assert_bits_equal: one x element
    dropped, one w element moved to the neighbouring channel, two channels' bias swapped, the conversion by truncation (the last
    one only where there is a conversion: 16-bit outputs)"""
    case = ec.conv_case(*key)
    want, _ = ec.reference(case)
    ec.assert_bits_equal(want.clone(), want, "self", relu=case.relu)
    caught = []
    for fault in FAULTS:
        if fault == "trunc" and case.out_dtype == torch.float32:
            continue
        bad, _ = ec.reference(case, fault=fault)
        with pytest.raises(AssertionError, match="elements differ"):
            ec.assert_bits_equal(bad, want, fault, relu=case.relu)
        caught.append("%s (%d)" % (fault, int((bad.view(torch.int32 if bad.dtype == torch.float32 else torch.int16)
                                               != want.view(torch.int32 if bad.dtype == torch.float32 else torch.int16)).sum())))
    print("%s: caught %s" % (_id(key), ", ".join(caught)))


def test_truncation_and_nearest_even_helpers():
    v = torch.tensor([257.0, 259.0, -257.0, -259.0, 258.0, 1.0, 2049.0, 2051.0, -2051.0], dtype=torch.float64)
    assert ec.convert(v, torch.bfloat16).double().tolist() == [256.0, 260.0, -256.0, -260.0, 258.0, 1.0, 2048.0, 2048.0, -2048.0]
    assert ec.convert(v, torch.bfloat16, trunc=True).double().tolist() == [256.0, 258.0, -256.0, -258.0, 258.0, 1.0, 2048.0, 2048.0,
                                                                          -2048.0]
    assert ec.convert(v, torch.float16).double().tolist() == [257.0, 259.0, -257.0, -259.0, 258.0, 1.0, 2048.0, 2052.0, -2052.0]
    assert ec.convert(v, torch.float16, trunc=True).double().tolist() == [257.0, 259.0, -257.0, -259.0, 258.0, 1.0, 2048.0, 2050.0,
                                                                         -2050.0]
    assert ec.rounding_shares(v[:4], torch.bfloat16) == (1.0, 1.0) and ec.rounding_shares(v[4:6], torch.bfloat16) == (0.0, 0.0)
    assert ec.rounding_shares(torch.tensor([2049.0, 2050.0, 4097.0], dtype=torch.float64), torch.float16) == (2 / 3, 1 / 3)


def test_assert_bits_equal_sign_of_zero_and_report():
    want = torch.tensor([[[[0.0, 1.0, 2.0, 0.0]]]]).bfloat16().expand(1, 3, 5, 4).contiguous()
    got = want.clone()
    got[0, 1, 2, 0] = -0.0
    ec.assert_bits_equal(got, want, "relu", relu=1)                    # -0 against +0 after ReLU: equal
    for relu in (0, 2):
        with pytest.raises(AssertionError, match="1 of 60 elements differ"):
            ec.assert_bits_equal(got, want, "no relu", relu=relu)      # ... and nowhere else
    with pytest.raises(AssertionError):
        ec.assert_bits_equal(want, got, "want is -0", relu=1)          # only got is canonicalised, only against +0
    got = want.clone()
    got[0, 2, 4, 3] = 1.0
    with pytest.raises(AssertionError) as e:
        ec.assert_bits_equal(got, want, "corner", relu=1, tile=(8, 2))
    msg = str(e.value)
    for part in ("corner: 1 of 60", "(0, 2, 4)", "channel 3 of 4", "last row", "last column", "last M-tile of 8", "last N-tile of 2",
                 "got 1.0", "want 0.0", "got - want = 1.0"):
        assert part in msg, (part, msg)
    with pytest.raises(AssertionError):
        ec.assert_bits_equal(want.float(), want, "dtype")


@pytest.mark.parametrize("ds", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("hw", ec.BOTTLENECK_SIZES)
def test_bottleneck_reference_is_exact_per_layer(hw, dtype, ds):
    """reference_bottleneck asserts bound / g < 2^24 for every layer; here also: every layer in f32 equals float64, the block's
    residual matters at the integer level (taken from the neighbouring channel, the result changes)"""
    case = ec.bottleneck_case(hw, dtype, ds)
    y, ratios = ec.reference_bottleneck(case)
    print("bottleneck%s %s %s: bound / g per layer %s" % ("_ds" if ds else "", hw, dtype, ["%.4g" % r for r in ratios]))
    assert len(ratios) == (4 if ds else 3) and max(ratios) < ec.LIMIT

    def layer32(inp, i, pad, res, relu):          # the same block with f32 arithmetic throughout
        acc = F.conv2d(inp.permute(0, 3, 1, 2), case.w[i].float().permute(0, 3, 1, 2), padding=pad).permute(0, 2, 3, 1)
        v = acc * case.sb[i][0] + case.sb[i][1]
        if res is not None:
            v = v + res
        return (v.clamp(min=0) if relu else v).to(dtype).float()
    x = case.x.float()
    ident = layer32(x, 3, 0, None, False) if ds else x
    y32 = layer32(layer32(layer32(x, 0, 0, None, True), 1, 1, None, True), 2, 0, ident, True)
    assert torch.equal(y32, y.float())
    y_wrong = layer32(layer32(layer32(x, 0, 0, None, True), 1, 1, None, True), 2, 0, ident.roll(1, dims=-1), True)
    with pytest.raises(AssertionError, match="elements differ"):
        ec.assert_bits_equal(y_wrong.to(dtype), y, "residual from the neighbouring channel", relu=1)


@pytest.mark.parametrize("hw", ec.STEM_SIZES)
def test_stem_reference(hw):
    case = ec.stem_case(hw)
    assert len(set(case.mean)) == 3 and float(case.w.abs().max()) == 2
    for to_bgr in (True, False):
        img = ec.stem_image(case, to_bgr)
        src = case.u8.flip(-1) if to_bgr else case.u8
        assert torch.equal(img[:, 1], src[..., 1].float() - case.mean[1]) and torch.equal(img[:, 0], src[..., 0].float() - case.mean[0])
        for odt in (torch.float32, torch.bfloat16, torch.float16):
            y, ratio = ec.reference_stem(case, odt, to_bgr)
            yp, _ = ec.reference_stem(case, odt, to_bgr, pool=True)
            assert ratio < ec.LIMIT and y.shape[1:3] == ((hw[1] + 1) // 2, (hw[2] + 1) // 2)
            assert torch.equal(yp.float().permute(0, 3, 1, 2), F.max_pool2d(y.float().permute(0, 3, 1, 2), 3, 2, 1))
        print("stem %s to_bgr=%s: bound / g = %.4g" % (hw, to_bgr, ratio))
    # padding AFTER the mean: a conv over the zero-padded u8 image minus the mean is another function at the border
    img = ec.stem_image(case, True).double()
    wrong = F.conv2d(F.pad(img + torch.tensor(case.mean).view(1, 3, 1, 1), (3, 3, 3, 3)) - torch.tensor(case.mean).view(1, 3, 1, 1),
                     case.w.double(), stride=2)
    right = F.conv2d(img, case.w.double(), stride=2, padding=3)
    assert not torch.equal(wrong, right) and torch.equal(wrong[:, :, 2:-2, 2:-2], right[:, :, 2:-2, 2:-2])


@pytest.mark.parametrize("spec", ec.SP_CASES, ids=lambda s: "x".join(str(v) for v in s[0]))
def test_sp_reference(spec):
    shape, wide, relu, use_res = spec
    case = ec.sp_case(spec)
    assert float(case.x.abs().max()) > 2048 and float(case.x.abs().max()) <= 4096
    wh, wl = ec.split_hi_lo(case.w)
    assert bool((wl != 0).any()) == wide and (wide or float(case.w.abs().max()) <= 4)
    y, ratio = ec.reference_sp(case, "f32")
    yp, _ = ec.reference_sp(case, "planes")
    print("conv2d_sp %s: bound / g = %.4g" % (shape, ratio))
    C = y.shape[-1]
    assert yp.dtype == torch.bfloat16 and yp.shape[-1] == 2 * C and bool((yp[..., C:] != 0).any())
    assert torch.equal(yp[..., :C], y.to(torch.bfloat16))
    # the three-term contraction is not the full product once both lo parts are non-zero
    full = ec.conv_f64(case.x, case.w, *shape[6:])
    xh, xl = ec.split_hi_lo(case.x)
    three = sum(ec.conv_f64(a, b, *shape[6:]) for a, b in ((xh, wh), (xl, wh), (xh, wl)))
    assert torch.equal(three, full) != wide


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", ec.DECONV_SHAPES)
def test_deconv_reference(shape, dtype):
    N, H, W, Cin, C, Cs = shape
    case = ec.deconv_case(shape, dtype)
    full, bound = ec.reference_deconv(case, 2, 2 * H + 2, 2 * W + 2)
    crop, _ = ec.reference_deconv(case, 2, 2 * H + 1, 2 * W)
    assert bound < ec.LIMIT and torch.equal(crop, full[:, 1:2 * H + 2, 1:2 * W + 1])
    f32 = F.conv_transpose2d(case.x.float().permute(0, 3, 1, 2), case.wt, case.bias, stride=2).permute(0, 2, 3, 1)
    want = torch.where(f32 > 0, f32, f32 * torch.tensor(0.1)).to(dtype)
    assert torch.equal(want, full)
