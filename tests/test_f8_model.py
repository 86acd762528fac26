"""CPU: how a model comes by its FP8 blocks (cfg.FP8_CONV), what it refuses, and the scales' round trip (f8.py)."""
import json

import pytest
import torch

from mega.pytorch_amd import config, f8, modeling, ops
import mega.pytorch_amd.fgfa  # noqa: F401  (registers the FGFA / DFF detectors)


def _cfg(settings, arch="R-50", method="mega"):
    cfg = config.get_cfg(arch, method)
    cfg.MODEL.DEVICE = "cpu"
    for k, v in settings.items():
        setattr(cfg, k, v)
    return cfg


def _blocks(model):
    return [(n, m) for n, m in model.named_modules() if isinstance(m, modeling.Bottleneck)]


@pytest.mark.parametrize("settings", [{}, {"FP8_CONV": "off"}, {"DTYPE": "bfloat16"}, {"DTYPE": "bfloat16", "FP8_CONV": "off"}],
                         ids=["default", "off", "bf16", "bf16-off"])
def test_off_builds_no_f8_block(settings):
    assert config.get_cfg("R-50").FP8_CONV == "off"
    model = modeling.build_detection_model(_cfg(settings))
    assert f8.f8_blocks(model) == [] and f8.scales(model) == {}
    assert all(m.f8 is False and m.f8_in_scale is None and m.f8_mid_scale is None for _, m in _blocks(model))


@pytest.mark.parametrize("arch,count", [("R-50", 5), ("R-101", 22)])
def test_layer3_marks_exactly_the_identity_blocks_of_layer3(arch, count):
    cfg = _cfg({"DTYPE": "bfloat16", "FP8_CONV": "layer3"}, arch)
    model = modeling.build_detection_model(cfg)
    marked = [n for n, m in _blocks(model) if m.f8]
    assert marked == ["backbone.body.layer3.%d" % i for i in range(1, count + 1)]
    assert [n for n, _ in f8.f8_blocks(model)] == marked
    for n, m in _blocks(model):
        if m.f8:
            assert m.downsample is None and m.stride == 1 and m.dilation == 1
        else:
            assert ".layer3." not in n or n.endswith(".layer3.0")
    assert not any(m.f8 for n, m in _blocks(model) if "layer1" in n or "layer2" in n or "roi_heads" in n)
    res5 = [m for m in model.roi_heads.box.feature_extractor.head.modules() if isinstance(m, modeling.Bottleneck)]
    assert len(res5) == 3 and not any(m.f8 for m in res5)
    # the conv mode of an FP8 model is still "bf16", and the table still has its six rows
    assert modeling.conv_mode(cfg) == "bf16" and model.backbone.body.mode is modeling.CONV_MODES["bf16"]
    assert len(modeling.CONV_MODES) == 6 and len(modeling.ConvMode._fields) == 7


@pytest.mark.parametrize("method", ["fgfa", "dff", "base"])
def test_the_other_detectors_take_the_key_too(method):
    model = modeling.build_detection_model(_cfg({"DTYPE": "bfloat16", "FP8_CONV": "layer3"}, method=method))
    assert len(f8.f8_blocks(model)) == 5


@pytest.mark.parametrize("settings", [{}, {"DTYPE": "float32"}, {"F32_CONV": "bf16x3"}, {"DTYPE": "float16"},
                                      {"DTYPE": "float16", "F16_CONV": "x2"}, {"DTYPE": "bfloat16", "RESIDUAL_STREAM": "planes"}],
                         ids=["default-f32", "f32", "x3", "f16", "h2", "wide"])
def test_every_other_mode_refuses_layer3(settings):
    with pytest.raises(ValueError, match="FP8_CONV"):
        modeling.build_detection_model(_cfg(dict(settings, FP8_CONV="layer3")))


def test_an_unknown_value_is_refused():
    with pytest.raises(ValueError, match="FP8_CONV"):
        modeling.build_detection_model(_cfg({"DTYPE": "bfloat16", "FP8_CONV": "layer4"}))


def test_only_an_identity_block_of_the_bf16_mode_can_be_f8():
    bf16 = modeling.CONV_MODES["bf16"]
    assert modeling.Bottleneck(1024, 256, 1024, 1, mode=bf16, f8=True).f8
    for args, mode in (((512, 256, 1024, 2), bf16), ((1024, 256, 1024, 2), bf16), ((1024, 256, 1024, 1), modeling.CONV_MODES["f16"]),
                       ((256, 64, 256, 1), bf16)):
        with pytest.raises(ValueError, match="FP8"):
            modeling.Bottleneck(*args, mode=mode, f8=True)


def test_an_f8_block_without_scales_raises():
    blk = modeling.Bottleneck(1024, 256, 1024, 1, mode=modeling.CONV_MODES["bf16"], f8=True)
    with pytest.raises(RuntimeError, match="scales"):
        blk.run(torch.zeros((1, 2, 2, 1024), dtype=torch.bfloat16))
    blk.set_f8_scales(0.5, 0.25)
    assert (blk.f8_in_scale, blk.f8_mid_scale) == (0.5, 0.25)
    with pytest.raises(ValueError):
        modeling.Bottleneck(1024, 256, 1024, 1, mode=modeling.CONV_MODES["bf16"]).set_f8_scales(1.0, 1.0)


def test_scales_round_trip_through_json(tmp_path):
    cfg = _cfg({"DTYPE": "bfloat16", "FP8_CONV": "layer3"})
    model = modeling.build_detection_model(cfg)
    names = [n for n, _ in f8.f8_blocks(model)]
    assert f8.scales(model) == {n: {"in": None, "mid": None} for n in names}
    want = {n: {"in": 0.01 * (i + 1) / 3.0, "mid": 1.0 / (7.0 + i)} for i, n in enumerate(names)}
    path = tmp_path / "scales.json"
    path.write_text(json.dumps(want))
    f8.load_scales(model, str(path))
    assert f8.scales(model) == want                                   # floats survive JSON exactly
    other = modeling.build_detection_model(cfg)
    f8.load_scales(other, json.loads(json.dumps(f8.scales(model))))
    assert f8.scales(other) == want
    for bad in ({k: v for k, v in list(want.items())[1:]}, dict(want, extra={"in": 1.0, "mid": 1.0}),
                dict(want, **{names[0]: {"in": 0.0, "mid": 1.0}}), dict(want, **{names[0]: {"in": float("inf"), "mid": 1.0}})):
        with pytest.raises(ValueError):
            f8.load_scales(other, bad)
    with pytest.raises(ValueError):
        f8.calibrate(modeling.build_detection_model(_cfg({"DTYPE": "bfloat16"})), torch.zeros(1, 3, 32, 32))


def test_state_dict_keys_are_unchanged():
    off = modeling.build_detection_model(_cfg({"DTYPE": "bfloat16"}))
    on = modeling.build_detection_model(_cfg({"DTYPE": "bfloat16", "FP8_CONV": "layer3"}))
    f8.load_scales(on, {n: {"in": 1.0, "mid": 1.0} for n, _ in f8.f8_blocks(on)})
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    on.load_state_dict(off.state_dict())
    assert not [n for n, _ in on.named_parameters() if "f8" in n] and not [n for n, _ in on.named_buffers() if "f8" in n]


def test_conv2d_nhwc_f8_refuses_before_any_device_or_library_check():
    w = lambda co, r, ci: torch.zeros((co, r, r, ci), dtype=f8.FP8)        # CPU tensors: any later check would object
    sc, bi = torch.ones(64), torch.zeros(64)
    with pytest.raises(ValueError, match="admit"):
        ops.conv2d_nhwc_f8(torch.zeros((1, 4, 4, 96), dtype=torch.bfloat16), w(64, 1, 96), sc, bi, in_scale=1.0)
    with pytest.raises(ValueError, match="admit"):
        ops.conv2d_nhwc_f8(torch.zeros((1, 4, 4, 128), dtype=f8.FP8), w(64, 3, 128), sc, bi, pad=1, stride=2)
    with pytest.raises(ValueError, match="dtype"):
        ops.conv2d_nhwc_f8(torch.zeros((1, 4, 4, 128), dtype=torch.float32), w(64, 1, 128), sc, bi, in_scale=1.0)
    with pytest.raises(ValueError, match="dtype"):
        ops.conv2d_nhwc_f8(torch.zeros((1, 4, 4, 128), dtype=f8.FP8), torch.zeros((64, 1, 1, 128), dtype=torch.bfloat16), sc, bi)
    with pytest.raises(ValueError, match="in_scale"):
        ops.conv2d_nhwc_f8(torch.zeros((1, 4, 4, 128), dtype=torch.bfloat16), w(64, 1, 128), sc, bi)
    with pytest.raises(RuntimeError):        # an admitted call on CPU tensors gets as far as the device check
        ops.conv2d_nhwc_f8(torch.zeros((1, 4, 4, 128), dtype=f8.FP8), w(64, 1, 128), sc, bi)
