"""ops.conv2d_nhwc_f8 (csrc/igemm_f8.hip) against the float64 reference of tests/f8_conv_cases.py, byte for byte (-m gpu).

The cases are exact by construction (check_exact), so there is no tolerance: a wrong A / B lane map of the block-scaled MFMA
(the reference's k_permuted fault), a border tap that reads the neighbouring row (pad_wraps_row), a lost K step, truncation,
a missing clamp or another exponent bias each change bytes (tests/test_f8_conv_cases.py proves it on the CPU)."""
import ctypes

import pytest
import torch

import f8_conv_cases as fc
import poison
from mega.pytorch_amd import _lib, f8, ops

pytestmark = pytest.mark.gpu

KEYS = fc.case_keys()
IDS = [fc.case_id(k) for k in KEYS]
_CODE = {"bf16": ops.BF16, "f8": ops.F8}


def _run(case, dev, out=None):
    return ops.conv2d_nhwc_f8(case.x.to(dev), case.wq.to(dev), case.scale.to(dev), case.bias.to(dev),
                              in_scale=case.in_scale if case.in_kind == "bf16" else None, out_scale=case.out_scale,
                              pad=case.pad, relu=bool(case.relu), out=out)


def _plan(case):
    N, H, W, Cin, Cout, R = case.shape
    return _lib.load().mega_conv2d_nhwc_f8_plan(N, H, W, Cin, Cout, R, R, 1, case.pad, 1, _CODE[case.in_kind], _CODE[case.out_kind])


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_conv_equals_the_float64_reference_byte_for_byte(dev, key):
    case = fc.conv_case(key)
    fc.check_exact(case)
    assert _plan(case) == (256 if case.shape[4] % 256 == 0 else 64)
    got = _run(case, dev)
    torch.cuda.synchronize()
    fc.assert_codes_equal(got, fc.reference(case), fc.case_id(key))


# (N, H, W, Cin, Cout, R, S, stride, pad, dil, in code, out code)
UNADMITTED = [
    (1, 5, 7, 96, 64, 1, 1, 1, 0, 1, ops.BF16, ops.F8),           # Cin not a multiple of 128
    (1, 5, 7, 64, 64, 1, 1, 1, 0, 1, ops.F8, ops.BF16),
    (1, 5, 7, 128, 96, 1, 1, 1, 0, 1, ops.BF16, ops.F8),          # Cout not a multiple of 64
    (1, 5, 7, 128, 64, 3, 3, 2, 1, 1, ops.F8, ops.BF16),          # 3x3 with stride 2
    (1, 5, 7, 128, 64, 1, 1, 2, 0, 1, ops.BF16, ops.F8),          # 1x1 with stride 2
    (1, 5, 7, 128, 64, 3, 3, 1, 2, 2, ops.F8, ops.BF16),          # dilation
    (1, 5, 7, 128, 64, 3, 3, 1, 0, 1, ops.F8, ops.BF16),          # 3x3 without padding
    (1, 5, 7, 128, 64, 1, 1, 1, 1, 1, ops.F8, ops.BF16),          # 1x1 with padding
    (1, 5, 7, 128, 64, 3, 1, 1, 1, 1, ops.F8, ops.BF16),          # 3x1
    (1, 5, 7, 128, 64, 5, 5, 1, 2, 1, ops.F8, ops.BF16),          # 5x5
    (0, 5, 7, 128, 64, 1, 1, 1, 0, 1, ops.F8, ops.BF16),          # no rows
    (1, 5, 7, 128, 64, 1, 1, 1, 0, 1, ops.F32, ops.BF16),         # f32 input
    (1, 5, 7, 128, 64, 1, 1, 1, 0, 1, ops.F16, ops.BF16),         # f16 input
    (1, 5, 7, 128, 64, 1, 1, 1, 0, 1, ops.F8, ops.F32),           # f32 output
]


@pytest.mark.parametrize("spec", UNADMITTED, ids=["-".join(str(v) for v in s) for s in UNADMITTED])
def test_an_unadmitted_layer_is_refused_and_nothing_is_written(dev, spec):
    N, H, W, Cin, Cout, R, S, stride, pad, dil, idt, odt = spec
    lib = _lib.load()
    assert lib.mega_conv2d_nhwc_f8_plan(N, H, W, Cin, Cout, R, S, stride, pad, dil, idt, odt) < 0
    if idt in (ops.BF16, ops.F8) and odt in (ops.BF16, ops.F8):
        assert not ops.f8_conv_admitted(N, H, W, Cin, Cout, R, S, stride, pad, dil)      # the wrapper's rule is the library's
    x = torch.zeros(max(N, 1) * H * W * Cin * 4, dtype=torch.uint8, device=dev)
    w = torch.zeros(Cout * R * S * Cin, dtype=torch.uint8, device=dev)
    out = torch.full((max(N, 1) * H * W * Cout * 4,), 0xA5, dtype=torch.uint8, device=dev)
    rc = lib.mega_conv2d_nhwc_f8(x.data_ptr(), idt, 1.0, w.data_ptr(), None, None, out.data_ptr(), odt, 1.0, N, H, W, Cin, Cout,
                                 R, S, stride, pad, dil, 1, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 1      # MEGA_ERR_ARG
    assert bool((out == 0xA5).all()), "a refused launch wrote to its output"


def test_the_wrappers_rule_is_the_librarys_on_the_admitted_side():
    lib = _lib.load()
    for N, H, W, Cin, Cout, R in fc.SHAPES + [(40, 38, 63, 1024, 256, 1), (40, 38, 63, 256, 256, 3), (1, 1, 1, 128, 64, 3)]:
        assert ops.f8_conv_admitted(N, H, W, Cin, Cout, R, R, 1, R // 2, 1)
        assert lib.mega_conv2d_nhwc_f8_plan(N, H, W, Cin, Cout, R, R, 1, R // 2, 1, ops.F8, ops.BF16) in (64, 256)


STALE = [k for k in KEYS if k[0] in (fc.SHAPES[0], fc.SHAPES[2]) and (k[1], k[2]) == (("bf16", "f8") if k[0][5] == 1 else ("f8", "bf16"))]


@pytest.mark.parametrize("mode", ["zeros", "ones"])
@pytest.mark.parametrize("key", STALE, ids=[fc.case_id(k) for k in STALE])
def test_the_result_does_not_depend_on_stale_output_bytes(dev, key, mode):
    case = fc.conv_case(key)
    with poison.poisoned(mode, (ops,)) as p:
        got = _run(case, dev)
        torch.cuda.synchronize()
    assert p.count >= 1, "the output did not come from the poisoned allocator"
    fc.assert_codes_equal(got, fc.reference(case), "%s under %s" % (fc.case_id(key), mode))


def test_a_captured_graph_replays_the_eager_bytes(dev):
    key = [k for k in KEYS if k[0] == fc.SHAPES[3]][0]
    case = fc.conv_case(key)
    eager = _run(case, dev)
    torch.cuda.synchronize()
    x, w, sc, bi = case.x.to(dev), case.wq.to(dev), case.scale.to(dev), case.bias.to(dev)
    out = torch.empty_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # warm-up outside the capture
        ops.conv2d_nhwc_f8(x, w, sc, bi, out_scale=case.out_scale, pad=case.pad, relu=bool(case.relu), out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.conv2d_nhwc_f8(x, w, sc, bi, out_scale=case.out_scale, pad=case.pad, relu=bool(case.relu), out=out)
    for i in range(2):
        out.view(torch.uint8).fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        fc.assert_codes_equal(out, eager, "replay %d" % i)
    fc.assert_codes_equal(eager, fc.reference(case), fc.case_id(key))
