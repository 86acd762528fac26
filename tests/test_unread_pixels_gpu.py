"""-m gpu: the even-pixel forms of the blocks whose output only a stride-2 1x1 conv reads (layer1 / layer2's last block, STRIDE_IN_1X1;
modeling.ResNet.skip_unread_pixels).  A stride-2 1x1 conv without padding loads pixels (2i, 2j) and nothing else, so those
blocks write y[:, ::2, ::2, :] alone: ops.bottleneck64(subsample=True), conv2 as a stride-2 conv, conv3 with its identity read at
a pixel stride of 2.  Every pixel that is still computed goes through the same instructions in the same K order: all
comparisons here are on the 16-bit patterns, in bf16 and in f16.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


def _ops():
    from mega.pytorch_amd import ops
    return ops


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _bneck_weights(g, dtype, dev, kind):
    if kind == "ints":        # small integers and power-of-two scales: every product and partial sum is exact
        w = [torch.randint(-1, 2, s, generator=g).float() for s in ((64, 1, 1, 256), (64, 3, 3, 64), (256, 1, 1, 64))]
        sb = [(torch.full((n,), sc), torch.randint(-2, 3, (n,), generator=g).float()) for n, sc in ((64, 1 / 16.), (64, 1 / 16.), (256, 1 / 8.))]
    else:
        w = [torch.randn(s, generator=g) * k for s, k in (((64, 1, 1, 256), 0.06), ((64, 3, 3, 64), 0.05), ((256, 1, 1, 64), 0.1))]
        sb = [(torch.rand((n,), generator=g) + 0.5, torch.randn((n,), generator=g) * 0.2) for n in (64, 64, 256)]
        if kind == "negative":    # bn3's bias far below anything conv3 + x can reach: every pre-ReLU value is negative
            sb[2] = (sb[2][0], torch.full((256,), -1.0e4))
    return [t.to(dtype).to(dev) for t in w], [(s.to(dev), b.to(dev)) for s, b in sb]


def _bneck_input(g, shape, dtype, dev, kind):
    N, H, W = shape
    if kind == "ints":
        x = torch.randint(0, 3, (N, H, W, 256), generator=g).float()
    else:
        x = torch.randn((N, H, W, 256), generator=g).relu()
    if kind == "large_odd":       # the pixels the compact output drops are ~100x the others (and finite in f16 all the way through
        odd = torch.ones((H, W), dtype=torch.bool)      # the block): a wrong pixel mapping cannot pass
        odd[::2, ::2] = False
        x[:, odd] = 100.0
    return x.to(dtype).to(dev)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 8, 16), (2, 9, 17), (3, 23, 37), (2, 16, 33), "slice"])
def test_bottleneck64_even_pixels_equal_dense(dev, shape, dtype):
    """ops.bottleneck64(subsample=True) == ops.bottleneck64(x)[:, ::2, ::2, :] bit for bit: one full 8 x 16 tile, odd sizes with
    one-pixel edge tiles, partial tiles on both edges with several tiles per frame, a batch slice of a larger tensor; random
    values, exact small integers, an all-negative pre-ReLU case (all +0) and odd pixels ~100x larger than the even ones."""
    ops = _ops()
    for kind in ("random", "ints", "negative", "large_odd"):
        g = torch.Generator().manual_seed(11 + len(kind))
        w, sb = _bneck_weights(g, dtype, dev, kind)
        if shape == "slice":
            big = _bneck_input(g, (4, 9, 17), dtype, dev, kind)
            x = big[1:3]
            assert x.is_contiguous() and x.data_ptr() != big.data_ptr()
        else:
            x = _bneck_input(g, shape, dtype, dev, kind)
        args = (w[0], sb[0][0], sb[0][1], w[1], sb[1][0], sb[1][1], w[2], sb[2][0], sb[2][1])
        dense = ops.bottleneck64(x, *args)
        got = ops.bottleneck64(x, *args, subsample=True)
        N, H, W = x.shape[:3]
        assert tuple(got.shape) == (N, (H + 1) // 2, (W + 1) // 2, 256) and got.is_contiguous()
        want = dense[:, ::2, ::2, :]
        nd = (got.view(torch.int16) != want.contiguous().view(torch.int16)).sum().item()
        assert nd == 0, "%s: %d of %d elements differ" % (kind, nd, got.numel())
        if kind == "negative":
            assert int(got.view(torch.int16).abs().max()) == 0
        else:
            assert float(got.float().abs().max()) > 0


def _conv3_case(g, N, H, W, Cout, dtype, dev):
    ho, wo = (H + 1) // 2, (W + 1) // 2
    t2 = torch.randn((N, ho, wo, 128), generator=g).relu().to(dtype).to(dev)
    x = torch.randn((N, H, W, Cout), generator=g).to(dtype)
    odd = torch.ones((H, W), dtype=torch.bool)
    odd[::2, ::2] = False
    x[:, odd] = 1000.0            # (what the strided read must skip)
    w3 = (torch.randn((Cout, 1, 1, 128), generator=g) * 0.1).to(dtype).to(dev)
    s = (torch.rand((Cout,), generator=g) + 0.5).to(dev)
    b = (torch.randn((Cout,), generator=g) * 0.2).to(dev)
    return t2, x.to(dev), w3, s, b


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 21, 17), (2, 75, 125), (1, 2, 2), (1, 20, 16)])
def test_conv3_residual_at_pixel_stride(dev, shape, dtype):
    """conv3 1x1 128 -> 512 + residual + ReLU on t2 [N,ho,wo,128] with the residual read at stride 2 from [N,H,W,512] == the same
    conv with the residual x[:, ::2, ::2].contiguous(): an M tail inside a tile, layer2's own map size, a single row, even sizes."""
    ops = _ops()
    g = torch.Generator().manual_seed(shape[1] * 5 + shape[2])
    t2, x, w3, s, b = _conv3_case(g, *shape, 512, dtype, dev)
    want = ops.conv2d_nhwc(t2, w3, s, b, residual=x[:, ::2, ::2].contiguous(), relu=True)
    got = ops.conv2d_nhwc(t2, w3, s, b, residual=x, relu=True, residual_stride=2)
    assert _bits_equal(got, want) and float(got.float().abs().max()) > 0
    assert float(got.float().abs().max()) < 500.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile", ["8:192", "8:256"])
def test_conv3_residual_at_pixel_stride_both_tiles(dev, tile, dtype, monkeypatch):
    """the same at Cout = 256 on igemm8's 192-row and on its 256-row tile (MEGA_IGEMM_TILE pins the tile of both launches), with
    rows past M in the last tile; and the unpinned launch gives the same bits."""
    ops = _ops()
    g = torch.Generator().manual_seed(77)
    t2, x, w3, s, b = _conv3_case(g, 2, 41, 29, 256, dtype, dev)        # M = 2 * 21 * 15 = 630: a tail on both tiles
    free = ops.conv2d_nhwc(t2, w3, s, b, residual=x, relu=True, residual_stride=2)
    monkeypatch.setenv("MEGA_IGEMM_TILE", tile)
    want = ops.conv2d_nhwc(t2, w3, s, b, residual=x[:, ::2, ::2].contiguous(), relu=True)
    got = ops.conv2d_nhwc(t2, w3, s, b, residual=x, relu=True, residual_stride=2)
    monkeypatch.delenv("MEGA_IGEMM_TILE")
    assert _bits_equal(got, want) and _bits_equal(free, want) and float(got.float().abs().max()) > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 21, 17), (2, 75, 125)])
def test_stride2_conv2_equals_dense_at_even_pixels(dev, shape, dtype):
    """conv2d_nhwc(t1, w2, stride=2, pad=1) == conv2d_nhwc(t1, w2, pad=1)[:, ::2, ::2] for the 3x3 128 -> 128 conv: output pixel
    (i, j) of the stride-2 conv is centred on input pixel (2i, 2j) -- the fact the even-pixel blocks rest on."""
    ops = _ops()
    N, H, W = shape
    g = torch.Generator().manual_seed(H + W)
    t1 = torch.randn((N, H, W, 128), generator=g).relu().to(dtype).to(dev)
    w2 = (torch.randn((128, 3, 3, 128), generator=g) * 0.04).to(dtype).to(dev)
    s = (torch.rand((128,), generator=g) + 0.5).to(dev)
    b = (torch.randn((128,), generator=g) * 0.2).to(dev)
    dense = ops.conv2d_nhwc(t1, w2, s, b, pad=1, relu=True)
    got = ops.conv2d_nhwc(t1, w2, s, b, stride=2, pad=1, relu=True)
    assert tuple(got.shape) == (N, (H + 1) // 2, (W + 1) // 2, 128)
    assert _bits_equal(got, dense[:, ::2, ::2, :]) and float(got.float().abs().max()) > 0


def _resnet50(dev, dtype):
    from mega.pytorch_amd import config, modeling
    cfg = config.get_cfg("R-50")
    cfg.DTYPE = {torch.bfloat16: "bfloat16", torch.float16: "float16"}[dtype]
    torch.manual_seed(5)
    body = modeling.ResNet(cfg)
    g = torch.Generator().manual_seed(6)
    for m in body.modules():
        if isinstance(m, modeling.FrozenBatchNorm2d):
            m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
            m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return body.to(dev)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frames", [(8, 128, 256), (2, 75, 131)])
def test_backbone_c4_unchanged_by_skipping_unread_pixels(dev, frames, dtype):
    """ResNet.run_nhwc (R-50-C4, seeded weights) with skip_unread_pixels on and off: C4 bit-equal.  8 frames of 128 x 256 give
    layer1 exactly the 128 tiles at which its blocks run as bneck64 (the even-pixel kernel); 2 odd-sized frames stay on the
    three-launch path (stride-2 conv2, conv3 with the strided residual).  layer1's and layer2's stored maps are compact."""
    from mega.pytorch_amd import modeling
    body = _resnet50(dev, dtype)
    N, H, W = frames
    img = torch.rand((N, 3, H, W), generator=torch.Generator().manual_seed(9)) * 255.0
    img = img.to(dev)
    h4, w4 = ((H + 1) // 2 + 1) // 2, ((W + 1) // 2 + 1) // 2      # stem (7x7 / 2, pad 3), max-pool (3x3 / 2, pad 1)
    fused = N * (-(-h4 // 8)) * (-(-w4 // 16)) >= 128
    assert fused == (frames == (8, 128, 256))
    shapes = {}
    for name in ("layer1", "layer2"):
        blk = list(getattr(body, name))[-1]
        def run(x, *a, _blk=blk, _name=name, **k):
            y = modeling.Bottleneck.run(_blk, x, *a, **k)
            shapes[_name] = (tuple(x.shape), tuple(y.shape), k.get("subsample", False))
            return y
        blk.run = run
    try:
        assert modeling.ResNet.skip_unread_pixels is True
        with torch.no_grad():
            got = body.run_nhwc(img)
            on = dict(shapes)
            body.skip_unread_pixels = False
            want = body.run_nhwc(img)
            off = dict(shapes)
    finally:
        body.skip_unread_pixels = True
    for name in ("layer1", "layer2"):
        (n, h, w, c), yshape, sub = on[name]
        assert sub and yshape == (n, (h + 1) // 2, (w + 1) // 2, c), (name, on[name])
        assert not off[name][2] and off[name][1] == off[name][0]
    assert on["layer1"][0][1:3] == (h4, w4)
    assert _bits_equal(got, want) and float(got.float().abs().max()) > 0
