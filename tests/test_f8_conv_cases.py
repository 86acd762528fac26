"""The FP8 conv cases check what they claim (CPU): exactness holds per case, the fp8-output cases reach every rounding class,
every planted fault changes the reference's bytes, and f8.quantize / ops.pack_conv_weight_f8 are the definition's."""
import pytest
import torch

import f8_conv_cases as fc
from mega.pytorch_amd import f8, ops

KEYS = fc.case_keys()
IDS = [fc.case_id(k) for k in KEYS]


def test_the_case_table_is_the_issues():
    assert len(fc.SHAPES) == 5 and len(KEYS) == 4 + 1 + 4 + 1 + 1
    for i in fc.ALL_COMBOS:
        assert {(k[1], k[2]) for k in KEYS if k[0] == fc.SHAPES[i]} == {(a, b) for a in ("bf16", "f8") for b in ("bf16", "f8")}
    for shape in fc.SHAPES:
        N, H, W, Cin, Cout, R = shape
        assert ops.f8_conv_admitted(N, H, W, Cin, Cout, R, R, 1, R // 2, 1)


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_every_case_is_exact(key):
    case = fc.conv_case(key)
    assert fc.check_exact(case) < fc.LIMIT
    assert len(set(case.scale.tolist())) >= 8, "the scales must differ per channel"
    assert float(case.w.abs().max()) <= 16 and torch.equal(case.w, case.w.round())
    assert torch.equal(case.bias, case.bias.round())


@pytest.mark.parametrize("key", [k for k in KEYS if k[2] == "f8"], ids=[i for k, i in zip(KEYS, IDS) if k[2] == "f8"])
def test_fp8_output_cases_reach_every_rounding_class(key):
    case = fc.conv_case(key)
    shares = fc.rounding_shares(case)
    print(fc.case_id(key), {k: round(v, 4) for k, v in shares.items()})
    for name in fc.CLASSES:
        assert shares[name] >= 0.01, "%s: class %s holds %.4f of the elements" % (fc.case_id(key), name, shares[name])


@pytest.mark.parametrize("fault", fc.FAULTS)
def test_every_planted_fault_changes_the_bytes(fault):
    hit = []
    for key in KEYS:
        case = fc.conv_case(key)
        if not fc.fault_applies(case, fault):
            continue
        good, bad = fc.reference(case), fc.reference(case, fault)
        try:
            fc.assert_codes_equal(bad, good, fault)
        except AssertionError:
            hit.append(fc.case_id(key))
    assert hit, "fault %s changes no case's bytes" % fault
    print(fault, "shows in", len(hit), "cases")


def test_the_zero_codes_compare_equal_and_nothing_else_does():
    a = torch.tensor([0x00, 0x80, 0x38], dtype=torch.uint8).view(fc.FP8)
    b = torch.tensor([0x80, 0x00, 0x38], dtype=torch.uint8).view(fc.FP8)
    fc.assert_codes_equal(a, b, "zeros")
    with pytest.raises(AssertionError):
        fc.assert_codes_equal(a, torch.tensor([0x00, 0x80, 0x39], dtype=torch.uint8).view(fc.FP8), "one code off")


def test_quantize_is_the_definition():
    q = lambda v, inv=1.0: f8.quantize(torch.tensor(v, dtype=torch.float32), inv).float().tolist()
    assert q([17.0, 19.0, 1.0625, 1.1875]) == [16.0, 20.0, 1.0, 1.25]              # ties go to even
    assert q([2.0 ** -10, 2.0 ** -9, 3 * 2.0 ** -10]) == [0.0, 2.0 ** -9, 2.0 ** -8]   # smallest subnormal 2^-9; ties to even
    assert q([449.0, 464.0, 465.0, 1e9, -1e9]) == [448.0, 448.0, 448.0, 448.0, -448.0]   # the clamp: no NaN above 464
    assert torch.isnan(torch.tensor(465.0).to(f8.FP8).float())                     # (what the clamp is for)
    assert q([896.0, 34.0], 0.5) == [448.0, 16.0]                                   # one f32 multiply first
    assert f8.quantize(torch.tensor([0.0, -0.0]), 1.0).view(torch.uint8).tolist() == [0x00, 0x80]
    assert f8.quantize(torch.tensor([448.0]), 1.0).view(torch.uint8).tolist() == [0x7e]     # e4m3fn, bias 7 (fnuz: 0x7f at 240)
    assert f8.quantize(torch.tensor([1.0]), 1.0).view(torch.uint8).tolist() == [0x38]
    assert f8.inv_scale(4.0) == 0.25 and f8.scale_of(0.0) == 1.0 and f8.scale_of(896.0) == 2.0


def test_pack_conv_weight_f8_round_trips():
    g = torch.Generator().manual_seed(5)
    w = torch.randn((64, 3, 3, 128), generator=g) * torch.logspace(-3, 1, 64).view(-1, 1, 1, 1)
    w[7] = 0
    codes, sw = ops.pack_conv_weight_f8(w)
    assert codes.dtype == f8.FP8 and codes.shape == w.shape and sw.dtype == torch.float32 and sw.shape == (64,)
    assert float(sw[7]) == 1.0 and not codes[7].float().any()
    back = codes.float() * sw.view(-1, 1, 1, 1)
    # half a step of e4m3 at |code| in [2^e, 2^(e+1)) is 2^(e-4); subnormal codes (below 2^-6) step 2^-9
    c = (w / sw.view(-1, 1, 1, 1)).abs().clamp(min=2.0 ** -6)
    half = torch.pow(2.0, torch.floor(torch.log2(c)) - 4) * sw.view(-1, 1, 1, 1)
    assert bool(((back - w).abs() <= half * (1 + 1e-6)).all())
    amax = codes.float().abs().flatten(1).max(dim=1).values
    assert bool((amax[torch.arange(64) != 7] == 448.0).all())
