"""ops.stem_pool (spatial.hip stem_pool_kernel: conv 7x7/2 + FrozenBN + ReLU + max_pool2d(3, 2, 1), resnet.py:355-366, in one
persistent kernel) at the edges of its own tiling: bit for bit against ops.maxpool3x3s2(ops.stem_u8(...)) (uint8 frames) or
ops.maxpool3x3s2(ops.stem(...)) (preprocessed f32 image), with the seeded inputs of test_kernels_gpu.py::
test_stem_pool_bit_equal.

The tile loop itself (more tiles than resident blocks, an image boundary crossed inside one block's loop) is what
test_stem_pool_bit_equal's (2, 600, 1000) case already runs: 2 x 22 x 21 = 924 tiles on at most 512 blocks.  It is not
repeated here."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MEAN = (102.9801, 115.9465, 122.7717)


def _ops():
    from mega.pytorch_amd import ops
    return ops


def _draw(ops, dev, g, dtype):
    w = torch.randn((64, 3, 7, 7), generator=g) * 0.05
    sc = (torch.rand((64,), generator=g) + 0.5).to(dev)
    bi = (torch.randn((64,), generator=g) * 0.1).to(dev)
    return w, ops.pack_stem_weight_bf16(w, dtype).to(dev), sc, bi


def _inputs(ops, dev, N, H, W, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(H * 3 + W)
    u8 = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    w, w160, sc, bi = _draw(ops, dev, g, dtype)
    return u8, w, w160, sc, bi


def _same_bits(got, ref, what=""):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    nd = (got.view(torch.int16) != ref.view(torch.int16)).sum().item()
    assert nd == 0, "%s: %d of %d elements differ" % (what, nd, got.numel())


def _edge_cases():
    """Pooled sizes 1, T - 1, T, T + 1, 2 T + 1 of the kernel's own tile T, each reached through every residue of the frame
    size mod 4 (pooled = (size - 1) // 4 + 1, so size = 4 (pooled - 1) + 1 + r, r = 0 .. 3: the four (Ho, Hp) rounding cases,
    and for W the four byte alignments of the uint8 row pitch 3 W).  20 heights and 20 widths, paired so that sizes and
    residues mix."""
    th, tw = _ops().stem_pool_tile()
    hs = [(hp, 4 * (hp - 1) + 1 + r) for hp in (1, th - 1, th, th + 1, 2 * th + 1) for r in range(4)]
    ws = [(wp, 4 * (wp - 1) + 1 + r) for r in range(4) for wp in (1, tw - 1, tw, tw + 1, 2 * tw + 1)]
    assert sorted(set(h % 4 for _, h in hs)) == [0, 1, 2, 3] and sorted(set(w % 4 for _, w in ws)) == [0, 1, 2, 3]
    return [(hp, h, wp, w) for (hp, h), (wp, w) in zip(hs, ws)]


def test_tile_edges(dev):
    ops = _ops()
    th, tw = ops.stem_pool_tile()
    assert th >= 2 and tw >= 2
    cases = _edge_cases()
    assert len(cases) == 20
    for hp, H, wp, W in cases:
        u8, w, w160, sc, bi = _inputs(ops, dev, 2, H, W)
        ref = ops.maxpool3x3s2(ops.stem_u8(u8, w160, sc, bi, MEAN, True))
        got = ops.stem_pool(u8, w160, sc, bi, MEAN, True)
        assert tuple(got.shape) == (2, hp, wp, 64)
        _same_bits(got, ref, "H %d W %d (pooled %d x %d, tile %d x %d)" % (H, W, hp, wp, th, tw))
        assert float(got.float().abs().max()) > 0


@pytest.mark.parametrize("shape", [(2, 9, 3), (2, 33, 47), (3, 13, 5), (1, 61, 101), (2, 30, 50)])
def test_no_byte_outside_the_frames_enters_a_result(dev, shape):
    """The frames are the middle slice of a larger uint8 tensor whose other bytes are 255 (and start at an odd byte offset for
    odd H W): the result must have the bits the same frames give from an allocation of their own.  Only allocated memory is
    ever touched."""
    ops = _ops()
    N, H, W = shape
    u8, w, w160, sc, bi = _inputs(ops, dev, N, H, W)
    big = torch.full((N + 2, H, W, 3), 255, dtype=torch.uint8, device=dev)
    big[1:N + 1] = u8
    inner = big[1:N + 1]
    assert inner.is_contiguous() and inner.data_ptr() == big.data_ptr() + H * W * 3
    for to_bgr in (True, False):
        own = ops.stem_pool(u8.clone(), w160, sc, bi, MEAN, to_bgr)
        _same_bits(ops.stem_pool(inner, w160, sc, bi, MEAN, to_bgr), own, "slice of a larger tensor, to_bgr %s" % to_bgr)
        _same_bits(own, ops.maxpool3x3s2(ops.stem_u8(u8, w160, sc, bi, MEAN, to_bgr)), "to_bgr %s" % to_bgr)


@pytest.mark.parametrize("fill", [0, 255])
def test_constant_frames(dev, fill):
    ops = _ops()
    N, H, W = 2, 59, 102
    _, w, w160, sc, bi = _inputs(ops, dev, N, H, W)
    u8 = torch.full((N, H, W, 3), fill, dtype=torch.uint8, device=dev)
    _same_bits(ops.stem_pool(u8, w160, sc, bi, MEAN, True), ops.maxpool3x3s2(ops.stem_u8(u8, w160, sc, bi, MEAN, True)),
               "frames of %d" % fill)


def test_all_negative_before_the_relu_gives_plus_zero(dev):
    """|conv| <= 147 taps x 255 x max|w| (< 0.3 at 0.05 sigma) x scale 1.5 < 2e4, so bias -1e6 makes every value negative
    before the ReLU: every pooled element is the bit pattern of +0 (never -0: the pool orders bit patterns)."""
    ops = _ops()
    N, H, W = 2, 59, 102
    u8, w, w160, sc, bi = _inputs(ops, dev, N, H, W)
    assert float(w.abs().max()) < 0.3
    bi = torch.full_like(bi, -1e6)
    got = ops.stem_pool(u8, w160, sc, bi, MEAN, True)
    _same_bits(got, ops.maxpool3x3s2(ops.stem_u8(u8, w160, sc, bi, MEAN, True)), "bias -1e6")
    assert int((got.view(torch.int16) != 0).sum().item()) == 0


def test_forms_bf16(dev):
    """both channel orders of the uint8 frames and the preprocessed f32 NCHW image, on a map of several tiles with partial
    ones at the right and bottom"""
    ops = _ops()
    th, tw = ops.stem_pool_tile()
    N, H, W = 2, 4 * (2 * th + 2) + 2, 4 * (2 * tw + 3) + 3
    u8, w, w160, sc, bi = _inputs(ops, dev, N, H, W)
    wt = w.permute(1, 2, 3, 0).reshape(147, 64).contiguous().to(dev)
    for to_bgr in (True, False):
        _same_bits(ops.stem_pool(u8, w160, sc, bi, MEAN, to_bgr), ops.maxpool3x3s2(ops.stem_u8(u8, w160, sc, bi, MEAN, to_bgr)),
                   "uint8 frames, to_bgr %s" % to_bgr)
    img = ops.preprocess_frames(u8, MEAN, True)
    _same_bits(ops.stem_pool(img, w160, sc, bi), ops.maxpool3x3s2(ops.stem(img, wt, sc, bi, torch.bfloat16, w_n160=w160)),
               "f32 NCHW image")


def test_forms_f16(dev):
    """IEEE-half operands.  There is no unfused fp16 stem to compare bits with, so: the uint8 and the f32-image form of the
    kernel agree bit for bit (they differ only in the patch load), and both are within 2 ulp of fp16, relative to the map's
    scale, of f32 arithmetic on the fp16-rounded pixels and weights (the bound of test_f16_gpu.py::test_f16_stem_pool: the
    summation order differs, so single-ulp flips of the staged fp16 map are allowed)."""
    ops = _ops()
    th, tw = ops.stem_pool_tile()
    N, H, W = 2, 4 * (2 * th + 2) + 2, 4 * (2 * tw + 3) + 3
    u8, w, w160, sc, bi = _inputs(ops, dev, N, H, W, torch.float16)
    img = ops.preprocess_frames(u8, MEAN, True)
    a, b = ops.stem_pool(u8, w160, sc, bi, MEAN, True), ops.stem_pool(img, w160, sc, bi)
    assert a.dtype == torch.float16
    _same_bits(a, b, "uint8 frames against the f32 image")
    conv = F.conv2d(img.cpu().half().float(), w.half().float(), stride=2, padding=3)
    stem = F.relu(conv * sc.cpu().view(1, -1, 1, 1) + bi.cpu().view(1, -1, 1, 1)).half().float()
    ref = F.max_pool2d(stem, 3, 2, 1).permute(0, 2, 3, 1)
    assert a.shape == ref.shape
    err = (a.float().cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert err < 2e-3, "fp16 stem + pool: %.3g of scale" % err
    assert (a.view(torch.int16) < 0).sum().item() == 0
