"""CPU: the table of the frame stage's precision modes (modeling.CONV_MODES) and how modules come by their mode -- told at
construction, from the cfg, never set from outside afterwards."""
import pytest
import torch

from mega.pytorch_amd import config, modeling, ops
import mega.pytorch_amd.fgfa  # noqa: F401  (registers the FGFA / DFF detectors)
import mega.pytorch_amd.rdn  # noqa: F401

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
#          cfg settings                                          name    compute planes   operands plane_dtype plain   stem_dtype
CASES = [({},                                                    "f32",  F32,    None,    None,    None,       None,   F32),
         ({"F32_CONV": "bf16x3"},                                "x3",   F32,    "all",   "x3",    BF16,       "f32",  F32),
         ({"DTYPE": "bfloat16"},                                 "bf16", BF16,   None,    None,    None,       None,   BF16),
         ({"DTYPE": "bfloat16", "RESIDUAL_STREAM": "planes"},    "wide", BF16,   "trunk", "hi",    BF16,       "bf16", BF16),
         ({"DTYPE": "float16"},                                  "f16",  F16,    None,    None,    None,       None,   F16),
         ({"DTYPE": "float16", "F16_CONV": "x2"},                "h2",   F16,    "all",   "h2",    F16,        "f32",  F32)]


def _cfg(settings, method="mega"):
    cfg = config.get_cfg("R-50", method)
    cfg.MODEL.DEVICE = "cpu"
    for k, v in settings.items():
        setattr(cfg, k, v)
    return cfg


def test_the_table_has_the_six_modes():
    assert sorted(modeling.CONV_MODES) == sorted(c[1] for c in CASES)
    assert all(k == m.name for k, m in modeling.CONV_MODES.items())


@pytest.mark.parametrize("case", CASES, ids=[c[1] for c in CASES])
def test_cfg_to_mode_and_every_module_carries_it(case):
    cfg = _cfg(case[0])
    assert modeling.conv_mode(cfg) == case[1]
    mode = modeling.conv_mode_of(cfg)
    assert tuple(mode) == case[1:] and mode is modeling.CONV_MODES[case[1]]
    with pytest.raises(AttributeError):
        mode.planes = "all"
    model = modeling.build_detection_model(cfg)
    fe = model.roi_heads.box.feature_extractor
    body = [m for m in model.backbone.modules() if isinstance(m, modeling.Bottleneck)]
    res5 = [m for m in fe.head.modules() if isinstance(m, modeling.Bottleneck)]
    assert len(body) == 3 + 4 + 6 and len(res5) == 3
    for m in body + res5 + [model.backbone.body, fe.head, fe, model.rpn.head]:
        assert m.mode is mode, type(m).__name__
    assert fe.dtype == model.backbone.body.dtype == case[2] and fe.head_x3 == (case[1] == "x3")
    # the packed operand of a conv in this mode: OHWI, K x 3 / x 2 in the operand forms that split, in the planes' dtype
    w = mode.pack(torch.nn.Conv2d(64, 8, 3, bias=False))
    kmul = {"x3": 3, "h2": 2}.get(mode.operands, 1)
    assert w.shape == (8, 3, 3, kmul * 64) and w.dtype == (mode.plane_dtype or mode.compute)


@pytest.mark.parametrize("method,name", [("fgfa", "GeneralizedRCNNFGFA"), ("dff", "GeneralizedRCNNDFF"),
                                         ("rdn", "GeneralizedRCNNRDN")])
def test_the_other_detectors_are_built_in_a_plain_mode(method, name):
    model = modeling.build_detection_model(_cfg({}, method))
    assert type(model).__name__ == name
    blocks = [m for m in model.modules() if isinstance(m, modeling.Bottleneck)]
    heads = [m for m in model.modules() if isinstance(m, modeling.ResNetHead)]
    assert len(blocks) == 3 + 4 + 6 + 3 and len(heads) == 1
    for m in blocks + heads + [model.backbone.body, model.rpn.head]:
        assert m.mode.planes is None and m.mode.operands is None and m.mode.name == "f32", type(m).__name__


def test_an_unknown_operand_form_is_refused_before_the_device_and_library_checks():
    x = ops.Planes(torch.zeros((1, 2, 2, 128), dtype=torch.bfloat16), 64)        # CPU tensors: any later check would object
    with pytest.raises(ValueError, match="operands"):
        ops.conv2d_sp(x, torch.zeros((8, 1, 1, 192), dtype=torch.bfloat16), operands="nonsense")
    with pytest.raises(ValueError, match="operands"):
        ops.linear_sp(ops.Planes(torch.zeros((4, 128), dtype=torch.bfloat16), 64), torch.zeros((8, 192), dtype=torch.bfloat16),
                      operands=True)
