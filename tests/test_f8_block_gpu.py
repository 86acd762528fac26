"""An FP8 bottleneck (cfg.FP8_CONV) on real-valued data, stage by stage against a float64 fake-quant twin (-m gpu).

One Bottleneck(1024, 256, 1024) identity block, f8=True, on a (2, 9, 11) map: N(0,1) / sqrt(K) weights, a ReLU'd N(0,1) trunk in
bf16, scales from f8.calibrate on that input.  Each stage is fed the GPU's own previous output, so one flipped code cannot
propagate into the next comparison.

The derived bound.  The kernel's accumulator is an f32 sum of K exact code products; whatever the order, it differs from the
exact sum by at most K 2^-23 sum|a b| (a loose form of the (K - 1) u sum|a b| bound of recursive summation, u = 2^-24, that
also covers the epilogue's two f32 roundings), i.e. by  K 2^-23 sum|a b| |scale[o]|  after the epilogue's scale.
  conv1 (fp8 out): the codes equal the twin's except at boundary elements -- the twin's pre-rounding value lies within that
    bound of a rounding boundary -- where the adjacent code is allowed; at most 0.1 % of the elements may use the allowance
    (an f32-accumulated conv1 of this kind flips 0 of 71,680 codes against float64 on the CPU).
  conv2 (bf16 out): one bf16 ulp of the twin's value plus the same bound, per element.
  whole block: conv3 + residual of the existing bf16 path applied to that conv2 output, bit for bit.
"""
import pytest
import torch

from exact_conv_cases import assert_bits_equal, conv_f64
from test_oracle_golden import _npz, e2e_inputs
from mega.pytorch_amd import config, f8, modeling, ops

pytestmark = pytest.mark.gpu

N, H, W = 2, 9, 11
_STATE = {}


def _block(dev):
    """the block, its trunk, the calibrated scales and the GPU's stage outputs, computed once"""
    if "blk" in _STATE:
        return _STATE
    g = torch.Generator().manual_seed(1234)
    blk = modeling.Bottleneck(1024, 256, 1024, 1, mode=modeling.CONV_MODES["bf16"], f8=True)
    with torch.no_grad():
        for conv in (blk.conv1, blk.conv2, blk.conv3):
            K = conv.weight[0].numel()
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / K ** 0.5)
        for bn in (blk.bn1, blk.bn2, blk.bn3):
            bn.weight.copy_(0.5 + torch.rand(bn.weight.shape, generator=g))
            bn.bias.copy_(0.1 * torch.randn(bn.bias.shape, generator=g))
    blk.to(dev)
    x = torch.randn((N, H, W, 1024), generator=g).clamp(min=0).to(torch.bfloat16).to(dev)
    sc = f8.calibrate(blk, x)
    assert sc == {"": {"in": blk.f8_in_scale, "mid": blk.f8_mid_scale}}
    assert blk.f8_in_scale == float(x.float().abs().max()) / 448.0 and blk.f8_mid_scale > 0
    pk = blk._packed(x.dtype, x.device)
    sc1, sc2 = blk._f8_fold(pk)
    t1 = ops.conv2d_nhwc_f8(x, pk["q1"], sc1, pk["b1"], in_scale=blk.f8_in_scale, out_scale=blk.f8_mid_scale, relu=True)
    t2 = ops.conv2d_nhwc_f8(t1, pk["q2"], sc2, pk["b2"], pad=1, relu=True)
    torch.cuda.synchronize()
    _STATE.update(blk=blk, x=x, pk=pk, sc1=sc1, sc2=sc2, t1=t1, t2=t2)
    return _STATE


def _twin(a, wq, scale, bias, pad):
    """(y, bound): float64 conv of the codes, y = relu(acc * scale + bias), bound = K 2^-23 sum|a b| |scale| per element"""
    a, wq = a.double().cpu(), wq.double().cpu()
    K = wq[0].numel()
    acc = conv_f64(a, wq, 1, pad, 1)
    absacc = conv_f64(a.abs(), wq.abs(), 1, pad, 1)
    sc, bi = scale.double().cpu(), bias.double().cpu()
    return (acc * sc + bi).clamp(min=0), K * 2.0 ** -23 * absacc * sc.abs()


def _order(codes):
    """e4m3 codes -> integers in value order (+-0 both 0): adjacent codes differ by 1"""
    b = codes.view(torch.uint8).to(torch.int32)
    return torch.where(b >= 128, -(b - 128), b)


def test_conv1_codes_equal_the_twin_except_at_rounding_boundaries(dev):
    s = _block(dev)
    blk = s["blk"]
    a = f8.quantize(s["x"].cpu(), f8.inv_scale(blk.f8_in_scale))           # the load path's codes: one f32 multiply, clamp, RNE
    y, bound = _twin(a, s["pk"]["q1"], s["sc1"], s["pk"]["b1"], 0)
    inv = f8.inv_scale(blk.f8_mid_scale)
    q = (y * inv).clamp(max=448.0)
    bound = bound * inv
    # float64 -> e4m3 in ONE rounding: the step of q's binade (subnormals share 2^-9), round half to even
    step = torch.pow(2.0, torch.floor(torch.log2(q.clamp(min=2.0 ** -6))) - 3)
    want = (torch.round(q / step) * step).float().to(f8.FP8)
    assert torch.equal(want.double(), torch.round(q / step) * step)
    frac = q / step - torch.floor(q / step)
    dist = torch.where(q >= 448.0, q - 432.0 + 1e9, (frac - 0.5).abs() * step)      # to the nearest midpoint between two codes
    boundary = dist <= bound
    got = s["t1"].cpu()
    diff = _order(got) - _order(want)
    used = diff != 0
    n = used.numel()
    print("conv1: %d of %d codes differ from the twin (%d boundary elements, largest bound %.3g of a step); codes in use: max %g, "
          "zero share %.3f" % (int(used.sum()), n, int(boundary.sum()), float((bound / step).max()), float(got.float().max()),
                               float((got.float() == 0).double().mean())))
    assert float(got.float().max()) == 448.0 or float(got.float().max()) >= 416.0      # the calibrated scale fills the range
    assert not bool((used & ~boundary).any()), "a code differs from the twin away from every rounding boundary"
    assert int(diff.abs().max()) <= 1, "a boundary element is more than one code away"
    assert int(used.sum()) <= 0.001 * n, "%d of %d elements use the boundary allowance (cap 0.1 %%)" % (int(used.sum()), n)


def test_conv2_equals_the_twin_to_one_bf16_ulp_plus_the_bound(dev):
    s = _block(dev)
    y, bound = _twin(s["t1"].float(), s["pk"]["q2"], s["sc2"], s["pk"]["b2"], 1)
    ulp = torch.pow(2.0, torch.floor(torch.log2(y.abs().clamp(min=2.0 ** -126))) - 7)
    err = (s["t2"].double().cpu() - y).abs()
    worst = float((err / (ulp + bound)).max())
    print("conv2: largest error %.3g of the allowance; %.4f of the elements differ from the twin's own bf16 rounding" % (
        worst, float((s["t2"].cpu() != y.to(torch.bfloat16)).double().mean())))
    assert bool((err <= ulp + bound).all()), "conv2 differs from the twin by %.3g of the allowance" % worst
    assert float(s["t2"].float().abs().max()) > 0


def test_the_whole_block_is_conv3_of_the_bf16_path_on_that_output(dev):
    s = _block(dev)
    pk = s["pk"]
    want = ops.conv2d_nhwc(s["t2"], pk["w3"], pk["s3"], pk["b3"], residual=s["x"], relu=True)
    got = s["blk"].run(s["x"])
    out = torch.empty_like(want)
    got2 = s["blk"].run(s["x"], out=out)
    torch.cuda.synchronize()
    assert got2 is out or got2.data_ptr() == out.data_ptr()
    assert_bits_equal(got, want, "FP8 block", relu=1)
    assert_bits_equal(out, want, "FP8 block, out=", relu=1)
    # and it is not the bf16 block's result: the FP8 path really ran (the difference is printed, not bounded here)
    with f8._bypass(lambda *a: None):
        ref = s["blk"].run(s["x"])
    assert not torch.equal(ref, got)
    print("FP8 block against the bf16 block: largest difference %.3g of the largest output" % float(
        (got.float() - ref.float()).abs().max() / ref.float().abs().max()))


def test_fp8_conv_off_gives_the_default_models_c4_bits(dev):
    bodies = []
    for settings in ({}, {"FP8_CONV": "off"}):
        cfg = config.get_cfg("R-50")
        cfg.DTYPE = "bfloat16"
        cfg.MODEL.DEVICE = str(dev)
        for k, v in settings.items():
            setattr(cfg, k, v)
        torch.manual_seed(11)
        bodies.append(modeling.ResNet(cfg).to(dev))
    bodies[1].load_state_dict(bodies[0].state_dict())
    img = torch.randn((2, 3, 96, 160), generator=torch.Generator().manual_seed(3)).to(dev) * 50
    a, b = (m.run_nhwc(img) for m in bodies)
    torch.cuda.synchronize()
    assert a.shape[-1] == 1024 and bool(torch.isfinite(a.float()).all())
    assert_bits_equal(b, a, "C4 with FP8_CONV off")


def test_clip_engine_with_an_fp8_r50_equals_the_model_call(dev):
    """the clip of test_reference_call_convention_equals_engine: model(images) per key frame == ClipEngine batches, bit for bit,
    with layer3's identity blocks in FP8 (the scales are kernel arguments by value, fixed at capture)"""
    from mega.pytorch_amd import engine
    d = _npz("ref_e2e_r50.npz")
    sd, frames, gfor, T = e2e_inputs(d)
    fr = frames.to(dev)
    models = []
    for _ in range(2):
        cfg = config.get_cfg("R-50")
        cfg.DTYPE, cfg.FP8_CONV = "bfloat16", "layer3"
        cfg.MODEL.DEVICE = str(dev)
        cfg.NMS_STRICT_GT = True
        m = modeling.build_detection_model(cfg)
        m.load_state_dict(sd)
        m.to(dev)
        models.append(m)
    sc = f8.calibrate(models[0], fr[:4])
    assert len(sc) == 5 and all(v["in"] > 0 and v["mid"] > 0 for v in sc.values())
    f8.load_scales(models[1], sc)
    m1, m2 = models
    dets = engine.ClipEngine(m2, steps_per_batch=3).run(fr, T, gfor, first=0, last=5)
    for idx in range(5):
        images = {"cur": fr[idx], "ref_l": [fr[min(T - 1, idx + 12)]], "ref_g": [fr[g] for g in gfor(idx)],
                  "frame_category": 0 if idx == 0 else 1, "seg_len": T, "ref_l_init": [fr[i] for i in range(1, 13)]}
        det = m1(images)[0]
        assert torch.equal(det.bbox, dets[idx].bbox) and torch.equal(det.get_field("labels"), dets[idx].get_field("labels"))
        assert torch.equal(det.get_field("scores"), dets[idx].get_field("scores"))
