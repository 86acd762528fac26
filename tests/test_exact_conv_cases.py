"""The integer-valued conv cases of tests/exact_conv_cases.py, checked on the CPU before the GPU file trusts them:
(1) every case meets the exactness condition and torch's f32 convolution equals the float64 one bit for bit (the accumulation
order cannot matter); (2) the output conversion really rounds, ties included; (3) assert_bits_equal catches four planted faults
in every case; (4) the split-precision table (ec.SP_TABLE, tests/test_exact_sp_gpu.py): it covers every launch class, operand
form and output mode, each case is exact and needs its lo planes / second rounding / ties on >= 1 % of its elements, ten
planted faults are rejected, and the Bottleneck.run_sp reference is exact per layer.  Each test prints its figures (run with -s
to see them)."""
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


# ------------------------------------------------------------------------------------------------ the split-precision table
SP_IDS = [r[0] for r in ec.SP_TABLE]
MIN_SHARE = 0.01          # a condition on the cases, not a measurement: each fault class is exercised by >= 1 % of the elements


def _sp_raw_plan(*args):
    from mega.pytorch_amd import _lib
    return _lib.load().mega_conv2d_nhwc_sp_plan(*args)


def _sp_plan(M, Cout, K, taps, out_mode, has_ws=0):
    t = _sp_raw_plan(M, Cout, K, taps, {"plain": 0, "planes": 1, "f32": 2}[out_mode], has_ws)
    assert t > 0
    return t // 1000000, t % 1000000 // 1000, t % 1000


def _igemm8_rows(M, Cout, z=1):
    """igemm.hip's igemm8_rows, restated: 256 rows only where that saves a round of the 256 CUs"""
    cdiv = lambda a, b: -(-a // b)
    t256, t192 = cdiv(M, 256) * cdiv(Cout, 256) * z, cdiv(M, 192) * cdiv(Cout, 256) * z
    return 192 if cdiv(t192, 256) * 192 * 9 < cdiv(t256, 256) * 256 * 8 else 256


def test_sp_table_covers_every_launch_class_form_and_mode():
    """the table as data: every value of every dimension the SP kernels branch on, and the named pairs; the class and row count
    each row states are what the library's own rule (mega_conv2d_nhwc_sp_plan, no GPU needed) gives that shape"""
    rows = ec.SP_TABLE
    assert len(set(SP_IDS)) == len(rows) and 14 <= len(rows) <= 18
    for name, shape, form, wide_w, relu, use_res, out_mode, pad_cols, kind, nrows, knobs in rows:
        M, Cout, K, taps = ec.sp_gemm_shape(shape, form)
        assert _sp_plan(M, Cout, K, taps, out_mode) == (kind, nrows, 256), name
        assert nrows == _igemm8_rows(M, Cout) and (kind == 7) == (taps == 1 and K <= 512), name
        assert not (pad_cols and out_mode == "planes")
    col = lambda i: {r[i] for r in rows}
    assert col(2) == {"x3", "h2", "hi", "hi-plain"} and col(4) == {0, 1, 2} and col(6) == set(ec.SP_OUT_MODES)
    assert {(r[8], r[9]) for r in rows} == {(7, 192), (7, 256), (8, 192), (8, 256)}
    assert {(r[6], r[5]) for r in rows} == {(m, b) for m in ec.SP_OUT_MODES for b in (False, True)}
    assert {(r[2].split("-")[0], r[5]) for r in rows} == {(f, b) for f in ec.SP_FORMS for b in (False, True)}
    big = [r for r in rows if r[9] == 256]
    assert all(r[1][4] == 2048 and r[1][0] * r[1][1] * r[1][2] == 6200 and r[1][5] == 1 for r in big)
    assert any(r[5] and r[6] == "planes" for r in big) and any(r[2] == "h2" for r in big)
    assert {r[1][3] for r in big if r[2] == "x3"} == {64, 192}                      # streaming K = 192, matrix K = 576
    assert {r[6] for r in rows if r[7]} == {"f32", "plain"}                         # the caller's out= buffer, ldo > Cout
    couts = {(r[1][4], r[5]) for r in rows}
    assert (64, True) in couts and (128, True) in couts and {c for c, _ in couts} >= {8, 264, 520}
    geo = {r[1][5:] for r in rows}
    assert (3, 1, 1, 1) in geo and (3, 1, 2, 2) in geo and (1, 2, 0, 1) in geo
    assert any(r[1][5:] == (3, 1, 1, 1) and r[1][3] == 64 for r in rows) and any(r[1][5:] == (3, 1, 1, 1) and r[1][3] >= 128 for r in rows)
    assert any(r[1][5:] == (1, 2, 0, 1) and r[1][1] % 2 == 1 and r[1][2] % 2 == 1 for r in rows)
    # split-K and the wrappers: what the GPU file asserts before it compares
    for form, (M, K, Nout) in ec.SP_SPLITK.items():
        assert ec.SP_FORMS[form][1] * K >= 32768 and _sp_plan(M, Nout, ec.SP_FORMS[form][1] * K, 1, "f32", 1) == (8, 192, 256)
        assert _sp_raw_plan(M, Nout, ec.SP_FORMS[form][1] * K, 1, 1, 1) == -1      # split-K serves the f32 output only
    M, K, Nout, ld = ec.SP_LINEAR_T
    assert M % 8 != 0 and ld > (M + 7) // 8 * 8 and _sp_plan(Nout, (M + 7) // 8 * 8, 3 * K, 1, "f32") == (8, 192, 256)
    # the production launches the 256-row rows stand for
    assert _sp_plan(95760, 1024, 3 * 256, 1, "planes")[1] == 256 and _sp_plan(4788, 1024, 3 * 256, 1, "planes")[1] == 192


@pytest.mark.parametrize("row", ec.SP_TABLE, ids=SP_IDS)
def test_sp_case_is_exact_and_exercises_every_fault_class(row):
    """reference_sp asserts bound / g < 2^24 (and |y| < 65504 for f16 planes and plain outputs); here also: torch's f32 convolution
    of the operands as the kernel contracts them equals the float64 one bit for bit, and the shares of elements that need the
    lo planes / the second rounding / the plain conversion (ties included) are at least 1 % each"""
    name, shape, form, wide_w, relu, use_res, out_mode, pad_cols, kind, nrows, knobs = row
    case = ec.sp_table_case(row)
    y, ratio = ec.reference_sp(case, out_mode)
    s = ec._sp_setup(case)
    assert ratio < ec.LIMIT and s.T == ec.SP_FORMS[case.form][0]
    for t in (case.x, case.w, case.bias) + ((case.res,) if use_res else ()):
        assert torch.equal(t, t.round())
    assert torch.equal(case.scale.log2(), case.scale.log2().round()) and case.scale.unique().numel() > 1
    assert case.bias.unique().numel() > 2
    st, pad, dil = shape[6:]
    acc32 = F.conv2d(s.A.float().permute(0, 3, 1, 2), s.Wk.float().permute(0, 3, 1, 2), stride=st, padding=pad,
                     dilation=dil).permute(0, 2, 3, 1)
    assert torch.equal(acc32.double(), s.acc), "f32 accumulation is not exact on this case"
    if wide_w:
        assert not torch.equal(case.w.to(s.T).float(), case.w), "no weight that %s does not hold" % s.T
    shares = ec.sp_shares(case, out_mode)
    msg = "%s: bound / g = %.4g, shares %s" % (name, ratio, {k: "%.2f %%" % (100 * v) for k, v in shares.items()})
    print(msg)
    if form == "hi-plain":
        assert shares.pop("in_lo") == 0 and torch.equal(case.x.to(s.T).float(), case.x), msg
    want = {"in_lo"} - ({"in_lo"} if form == "hi-plain" else set()) | ({"res_lo"} if use_res else set()) \
        | {"planes": {"out_lo", "out_inexact2"}, "plain": {"rounded", "ties"}, "f32": set()}[out_mode]
    assert set(shares) == want, msg
    for k, v in shares.items():
        assert v >= MIN_SHARE, "%s below 1 %%: %s" % (k, msg)
    if out_mode == "planes":
        C = shape[4]
        assert y.dtype == s.T and y.shape[-1] == 2 * C and torch.equal(y[..., :C], ec.reference_sp(case, "plain")[0])


@pytest.mark.parametrize("row", ec.SP_TABLE, ids=SP_IDS)
def test_sp_planted_faults_are_rejected(row):
    """each fault of ec.SP_FAULTS this case can show, planted in the reference's own arithmetic, is rejected by assert_bits_equal"""
    name, shape, form, wide_w, relu, use_res, out_mode, pad_cols, kind, nrows, knobs = row
    case = ec.sp_table_case(row)
    want, _ = ec.reference_sp(case, out_mode)
    ec.assert_bits_equal(want.clone(), want, "self", relu=relu)
    caught = []
    for fault in ec.SP_FAULTS:
        if not ec.sp_fault_applies(case, out_mode, fault):
            continue
        bad, _ = ec.reference_sp(case, out_mode, fault=fault)
        with pytest.raises(AssertionError, match="elements differ"):
            ec.assert_bits_equal(bad, want, fault, relu=relu)
        caught.append(fault)
    print("%s: caught %s" % (name, ", ".join(caught)))
    assert caught


def test_every_sp_fault_is_planted_somewhere():
    """every planted fault applies to at least one row of the table, one of them a 256-row row; the split-K and wrapper cases
    are exact, need their lo planes, and reject a dropped term"""
    for fault in ec.SP_FAULTS:
        rows = [r for r in ec.SP_TABLE if ec.sp_fault_applies(ec.sp_table_case(r), r[6], fault)]
        assert rows and (any(r[9] == 256 for r in rows) or fault in ("hi_reads_lo", "trunc_plain")), fault
    for form in ec.SP_SPLITK:
        case = ec.sp_splitk_case(form)
        want, ratio = ec.reference_sp(case, "f32")
        assert ratio < ec.LIMIT and ec.sp_shares(case, "f32")["in_lo"] >= MIN_SHARE
        for fault in ("drop_xlo_wh", "w_unrounded" if form == "h2" else "drop_xhi_wl"):
            with pytest.raises(AssertionError, match="elements differ"):
                ec.assert_bits_equal(ec.reference_sp(case, "f32", fault=fault)[0], want, fault, relu=1)
    for with_bias in (False, True):
        case = ec.sp_linear_case(with_bias)
        assert ec.reference_sp(case, "f32")[1] < ec.LIMIT and ec.sp_shares(case, "f32")["in_lo"] >= MIN_SHARE


def test_sp_split_helpers():
    v = torch.tensor([257.0, 259.0, 4097.0, 65536.0 + 131.0, -65536.0 - 131.0, 1.0])
    hi, lo = ec.split_hi_lo(v)
    assert hi.tolist() == [256.0, 260.0, 4096.0, 65536.0, -65536.0, 1.0] and lo.tolist() == [1.0, -1.0, 1.0, 131.0, -131.0, 0.0]
    assert torch.equal(ec.split_hi_lo(v, trunc_lo=True)[1], lo)                      # exact remainders: nothing to truncate
    v = torch.tensor([2.0 ** 20 + 1029.0, -2.0 ** 20 - 1029.0])                      # remainder 1029: nearest 1032, truncated 1024
    assert ec.split_hi_lo(v)[0].tolist() == [2.0 ** 20, -2.0 ** 20]
    assert ec.split_hi_lo(v)[1].tolist() == [1032.0, -1032.0] and ec.split_hi_lo(v, trunc_lo=True)[1].tolist() == [1024.0, -1024.0]
    h, l = ec.split_hi_lo(torch.tensor([4097.0, 2049.0, 16384.0 + 4.0 + 2.0 ** -9]), torch.float16)
    assert h.tolist() == [4096.0, 2048.0, 16384.0] and l.tolist() == [1.0, 1.0, 4.0]     # 4 + 2^-9 needs 12 bits: a tie, to even
    y = ec.sp_output(torch.arange(32, dtype=torch.float64).view(1, 1, 2, 16) + 65536.0, torch.bfloat16, "planes", "shift_lo")
    assert y.shape == (1, 1, 2, 32) and y[0, 0, 0, 16:].tolist() == [8.0, 9, 10, 11, 12, 13, 14, 15, 0, 1, 2, 3, 4, 5, 6, 7]


BLOCK_RUNS = [(spec, mode) for spec in ec.SP_BLOCKS for mode in ("x3", "h2", "wide") if mode == "wide" or not spec[2]]


@pytest.mark.parametrize("spec,mode", BLOCK_RUNS, ids=["%s%s-%s" % (s[0], "-plain-x" if s[2] else "", m) for s, m in BLOCK_RUNS])
def test_sp_block_reference_is_exact_per_layer_and_bites(spec, mode):
    """reference_sp_block asserts bound / g < 2^24 for every layer; here also: every hand-off has a non-zero lo plane on >= 1 %
    of its elements (the block's input -- the identity of an identity block -- included), the two output forms agree, the
    mode's hand-off matters (a planes mode and the plain-inside mode differ), and the comparison rejects an identity taken from
    its hi plane alone and a downsample subsampled from the wrong pixels"""
    kind, hw, plain_x = spec
    case = ec.sp_block_case(spec)
    form, T, plain = ec.SP_BLOCK_MODES[mode]
    Cin, mid, Cout, stride, dil, ds = ec.SP_BLOCK_KINDS[kind]
    y, ratios, lo_shares = ec.reference_sp_block(case, mode, False)
    yp, _, _ = ec.reference_sp_block(case, mode, True)
    print("run_sp %s %s %s: bound / g per layer %s, lo shares %s" % (kind, hw, mode, ["%.4g" % r for r in ratios],
                                                                    ["%.1f %%" % (100 * v) for v in lo_shares]))
    assert len(ratios) == (4 if ds else 3) and max(ratios) < ec.LIMIT
    assert len(lo_shares) == (0 if plain_x else 1) + (1 if ds else 0) + (2 if plain is None else 0)
    assert min(lo_shares) >= MIN_SHARE, lo_shares
    N, H, W = hw
    s = 1 if dil > 1 else stride
    assert y.shape == (N, (H - 1) // s + 1, (W - 1) // s + 1, 2 * Cout) and y.dtype == T
    out_lo = (y[..., Cout:] != 0).double().mean().item()
    assert out_lo >= MIN_SHARE, out_lo
    if plain is None:
        assert yp.dtype == torch.float32 and torch.equal(yp.to(T), y[..., :Cout])
    else:
        assert yp.dtype == plain and torch.equal(yp, y[..., :Cout])
    if not plain_x:
        other, _, _ = ec.reference_sp_block(case, "wide" if mode != "wide" else "x3", False)
        assert other.dtype != y.dtype or not torch.equal(other, y)
    for fault in ("identity_hi",) + (("ds_dense",) if ds else ()):
        bad, _, _ = ec.reference_sp_block(case, mode, False, fault=fault)
        with pytest.raises(AssertionError, match="elements differ"):
            ec.assert_bits_equal(bad, y, fault, relu=1)


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
