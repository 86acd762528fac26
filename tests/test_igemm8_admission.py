"""CPU: the admission rules of igemm8's launcher (mega_igemm8_launch, igemm8.hip), pinned through the C ABI without a device.

Each igemm8 epilogue mode serves only part of what the C ABI can describe, and a launch admitted by mistake would reach an
epilogue that writes nothing.  Without a GPU the library still loads: a launch that is REFUSED returns MEGA_ERR_ARG (1) before
anything is launched; a launch that is ADMITTED goes on to hipFuncSetAttribute, which fails, and returns MEGA_ERR_LAUNCH (2).
Every table row is one call; a row that violates one admission clause (expect 1) stands next to its nearest admitted
neighbour (expect 2).  The pointers are the address of a small host buffer: nothing on these paths dereferences them.

The expected codes are those of the launcher as it was before its ladders were folded into one table (the table was run
against that library unchanged).  Clauses the C ABI cannot violate on their own are not rows: a split output together with an
f32 output (one out_mode argument chooses between them), split-K with a residual or a split output (mega_conv2d_nhwc_sp_dt
refuses those itself, which the rows below pin), and the sub-pixel C alignment (Cout % 64 == 0 implies it).

NOT marked gpu, and skipped when a device is visible: an admitted row would then really launch on the placeholder pointers.
"""
import ctypes

import pytest

from mega.pytorch_amd import _lib

F32, BF16, F16 = 0, 1, 2
ARG, LAUNCH = 1, 2


@pytest.fixture(autouse=True)
def _no_device_no_forced_tile(monkeypatch):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is visible: admitted rows would launch on placeholder pointers")
    monkeypatch.delenv("MEGA_IGEMM_TILE", raising=False)      # (a forced tile would change which launcher a row reaches)


_buf = ctypes.create_string_buffer(4096)
PTR = ctypes.addressof(_buf)


def _run(table, call):
    wrong = []
    for want, what, kw in table:
        got = call(**kw)
        print("%-58s want %d got %d" % (what, want, got))
        if got != want:
            wrong.append((what, want, got))
    assert not wrong, wrong


def _sp(dtype, ldi=128, kwrap=128, Cin=192, Cout=64, res=False, ldr=0, ldo=0, out_mode=0, H=4, W=4, R=1, ws=False):
    """mega_conv2d_nhwc_sp_dt; the defaults are the split-precision form of a 64 -> 64 1x1 conv on 4 x 4 pixels."""
    lib = _lib.load()
    return lib.mega_conv2d_nhwc_sp_dt(PTR, ldi, kwrap, PTR, PTR, PTR, PTR if res else None, ldr, PTR, ldo, out_mode, 1, H, W,
                                      Cin, Cout, R, R, 1, R // 2, 1, 1, dtype, PTR if ws else None, 1 << 40 if ws else 0, None)


SP_ROWS = [
    (LAUNCH, "base: [hi | lo | hi] x [Wh | Wh | Wl]", {}),
    (LAUNCH, "base, 3x3", dict(R=3)),
    (LAUNCH, "base, f32 output", dict(out_mode=2)),
    (LAUNCH, "base, split output", dict(out_mode=1)),
    (LAUNCH, "base, split residual", dict(res=True)),
    # ldi >= the planes the contraction reads, and whole K-tiles per pixel
    (ARG, "ldi 64 < kwrap 128", dict(ldi=64)),
    (ARG, "ldi 64 < Cin 128, no wrap", dict(ldi=64, kwrap=0, Cin=128)),
    (LAUNCH, "ldi 128 = Cin 128, no wrap", dict(ldi=128, kwrap=0, Cin=128)),
    (ARG, "ldi 160: not a multiple of 64", dict(ldi=160)),
    (ARG, "ldi 100: neither", dict(ldi=100)),
    (LAUNCH, "ldi 192", dict(ldi=192)),
    # kwrap: whole K-tiles, inside the contraction, and the wrapped part no longer than the first
    (ARG, "kwrap 96: not a multiple of 64", dict(kwrap=96)),
    (ARG, "kwrap 192 = Cin", dict(kwrap=192, ldi=192)),
    (LAUNCH, "kwrap 128 < Cin 192, ldi 192", dict(kwrap=128, ldi=192)),
    (ARG, "kwrap 64: Cin - kwrap = 128 > kwrap", dict(kwrap=64, ldi=64)),
    (LAUNCH, "kwrap 64: Cin - kwrap = 64", dict(kwrap=64, ldi=64, Cin=128)),
    # Cout: whole 16-byte vectors of bf16
    (ARG, "Cout 60", dict(Cout=60, ldo=64)),
    (LAUNCH, "Cout 56", dict(Cout=56, ldo=64)),
    # ldo: 16-byte rows (8 elements of 16 bits, 4 of f32) and wide enough for the output planes
    (ARG, "ldo 68, 16-bit output", dict(ldo=68)),
    (LAUNCH, "ldo 72, 16-bit output", dict(ldo=72)),
    (LAUNCH, "ldo 68, f32 output", dict(ldo=68, out_mode=2)),
    (ARG, "ldo 66, f32 output", dict(ldo=66, out_mode=2)),
    (ARG, "ldo 56 < Cout", dict(ldo=56)),
    (ARG, "ldo 120 < 2 Cout, split output", dict(ldo=120, out_mode=1)),
    (LAUNCH, "ldo 128 = 2 Cout, split output", dict(ldo=128, out_mode=1)),
    # ldr: 16-byte rows of split planes
    (ARG, "ldr 132", dict(res=True, ldr=132)),
    (LAUNCH, "ldr 136", dict(res=True, ldr=136)),
    (ARG, "ldr 120 < 2 Cout", dict(res=True, ldr=120)),
    (LAUNCH, "ldr 128 = 2 Cout", dict(res=True, ldr=128)),
    # the output below 2 GiB (f32: (M - 1) ldo + Cout elements of 4 bytes)
    (LAUNCH, "output 1.07 GB", dict(ldi=64, kwrap=0, Cin=64, out_mode=2, H=2000, W=2100)),
    (ARG, "output 2.2 GB", dict(ldi=64, kwrap=0, Cin=64, out_mode=2, H=4096, W=2100)),
    # split-K (a workspace and K >= 32768): f32 output without a residual only
    (LAUNCH, "split-K, f32 output", dict(ldi=32768, kwrap=0, Cin=32768, out_mode=2, ws=True)),
    (ARG, "split-K, residual", dict(ldi=32768, kwrap=0, Cin=32768, out_mode=2, ws=True, res=True)),
    (ARG, "split-K, split output", dict(ldi=32768, kwrap=0, Cin=32768, out_mode=1, ws=True)),
    (ARG, "split-K, 16-bit output", dict(ldi=32768, kwrap=0, Cin=32768, out_mode=0, ws=True)),
]


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_split_precision_admission(dtype):
    _run(SP_ROWS, lambda **kw: _sp(dtype, **kw))


def test_split_precision_takes_16_bit_types_only():
    assert _sp(F32) == ARG


def _rs(dtype=BF16, H=3, W=3, Cin=64, Cout=256, ldo=0, ldr=0, res_H=5, res_W=5, res_stride=2, res=True):
    """mega_conv2d_nhwc_rs; the defaults: 3 x 3 output pixels that add pixels (2 y, 2 x) of a 5 x 5 residual map."""
    lib = _lib.load()
    return lib.mega_conv2d_nhwc_rs(PTR, PTR, PTR, PTR, PTR if res else None, PTR, 1, H, W, Cin, Cout, 1, ldo, ldr, res_H, res_W,
                                   res_stride, dtype, None)


RS_ROWS = [
    (LAUNCH, "base, bf16", {}),
    (LAUNCH, "base, f16", dict(dtype=F16)),
    (ARG, "f32 operands", dict(dtype=F32)),
    (ARG, "no residual", dict(res=False)),
    # the streaming class: 1x1 with K <= 512
    (LAUNCH, "K 512", dict(Cin=512)),
    (ARG, "K 576: not the streaming class", dict(Cin=576)),
    # whole 256-wide tiles of columns
    (ARG, "Cout 128", dict(Cout=128)),
    (ARG, "Cout 384", dict(Cout=384)),
    (LAUNCH, "Cout 512", dict(Cout=512)),
    # 16-byte rows
    (ARG, "ldo 260", dict(ldo=260)),
    (LAUNCH, "ldo 264", dict(ldo=264)),
    (ARG, "ldr 260", dict(ldr=260)),
    (LAUNCH, "ldr 264", dict(ldr=264)),
    (ARG, "ldr 248 < Cout", dict(ldr=248)),
    # the residual map holds pixel ((Ho - 1) s, (Wo - 1) s)
    (ARG, "res_H 4: row (Ho - 1) s = 4 is outside", dict(res_H=4)),
    (ARG, "res_W 4: column (Wo - 1) s = 4 is outside", dict(res_W=4)),
    (LAUNCH, "res_H 5, res_W 9", dict(res_W=9)),
    (ARG, "stride 3: row 6 is outside 5 x 5", dict(res_stride=3)),
    (LAUNCH, "stride 3 in 7 x 7", dict(res_stride=3, res_H=7, res_W=7)),
    (ARG, "res_H 0", dict(res_H=0)),
    (ARG, "res_stride 0", dict(res_stride=0)),
]


def test_strided_residual_admission():
    _run(RS_ROWS, _rs)


def _ps(dtype=BF16, H=3, W=3, Cin=64, C=64, out_H=8, out_W=8, crop=0, ldo=128, coff=0, ksplit=1):
    """mega_conv2d_nhwc_subpixel; the defaults run on the register-staged tiles, H = W = 160 (25921 GEMM rows: more than half
    a round of 192-row tiles) with C % 64 == 0 on igemm8's sub-pixel read-out."""
    lib = _lib.load()
    return lib.mega_conv2d_nhwc_subpixel(PTR, PTR, PTR, PTR, 1, H, W, Cin, C, 1, out_H, out_W, crop, ldo, coff, dtype, ksplit,
                                         None, 0, None)


_PS_CLAUSES = [
    (LAUNCH, "base", {}),
    (LAUNCH, "base, f16", dict(dtype=F16)),
    (LAUNCH, "C 128, ldo 256", dict(C=128, ldo=256)),
    # 4 C columns in whole 64-wide tiles (which implies C's own 16-byte alignment)
    (ARG, "C 72: 4 C % 64 = 32", dict(C=72)),
    (ARG, "C 68", dict(C=68)),
    # ldo, coff: 16-byte vectors; the slice inside the pixel
    (ARG, "ldo 132", dict(ldo=132)),
    (LAUNCH, "ldo 136", dict(ldo=136)),
    (ARG, "coff 4", dict(ldo=136, coff=4)),
    (LAUNCH, "coff 8", dict(ldo=136, coff=8)),
    (ARG, "coff 72 + C 64 > ldo 128", dict(coff=72)),
    (LAUNCH, "coff 64 + C 64 = ldo 128", dict(coff=64)),
    # the output tensor below 2 GiB
    (LAUNCH, "output 1.07 GB", dict(out_H=2048, out_W=2048)),
    (ARG, "output 4.3 GB", dict(out_H=4096, out_W=4096)),
    (ARG, "crop -1", dict(crop=-1)),
]
PS_ROWS = _PS_CLAUSES + [(want, what + " [igemm8]", dict(kw, H=160, W=160)) for want, what, kw in _PS_CLAUSES] + [
    (LAUNCH, "C 80: register-staged tiles only", dict(C=80)),
    (LAUNCH, "C 80 at igemm8's size: register-staged tiles", dict(C=80, H=160, W=160)),
    # f32 operands: vectors of 4 elements, Cin in K-tiles of 32
    (LAUNCH, "f32, ldo 132, Cin 32", dict(dtype=F32, ldo=132, Cin=32)),
    (ARG, "f32, ldo 130", dict(dtype=F32, ldo=130)),
    (ARG, "bf16, Cin 32", dict(Cin=32)),
    (ARG, "dtype 3", dict(dtype=3)),
]


def test_subpixel_admission():
    _run(PS_ROWS, _ps)
