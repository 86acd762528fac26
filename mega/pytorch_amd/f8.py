"""The FP8 quantisation of the opt-in FP8 conv path (cfg.FP8_CONV = "layer3"): this docstring is its definition; the kernel
(csrc/igemm_f8.hip), ops.conv2d_nhwc_f8 and the tests' float64 twins implement it.

Format.  OCP `e4m3fn`, carried as torch.float8_e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; largest finite value 448
(code 0x7e), no infinities, smallest subnormal 2^-9.  It is NOT MI300's `fnuz` format (bias 8).  The zero codes 0x00 and 0x80
compare equal.  NaN inputs are out of scope, as everywhere else in this project.

quantize(v, inv) = (v.float() * inv).clamp(-448, 448).to(torch.float8_e4m3fn)
    one f32 multiply, a clamp, then ONE round-to-nearest-even conversion.  The clamp comes first: without it torch turns
    values above 464 into NaN; with it they become 448.  Ties go to even: 17 -> 16, 19 -> 20, 1.0625 -> 1.0, 1.1875 -> 1.25;
    2^-10 (half the smallest subnormal, a tie) -> 0.

Weights.  One scale per output channel: sw[o] = absmax(w[o]) / 448, or 1 for an all-zero channel; codes = quantize(w[o],
    1 / sw[o]), laid out OHWI (ops.pack_conv_weight_f8).
Activations.  One static scale per tensor, s = absmax / 448 over the calibration frames (calibrate below); the kernel gets
    1 / s, computed once on the host in f32 (inv_scale).
The conv.  Per output channel  y = acc * (s_in * sw[o] * bn_scale[o]) + bn_bias[o],  acc = the f32 sum of code products; the
    host folds the three factors, in f32 and in that order, into the one scale[Cout] vector every conv entry point takes
    (fold_scale).  A padding tap is the code 0x00.

A model built with FP8_CONV "layer3" runs the identity blocks of layer3 as  conv1 (bf16 trunk -> fp8, quantised on the kernel's
load path and again in its epilogue), conv2 (fp8 -> bf16), conv3 + residual on the bf16 kernel as before.  Each such block
holds two calibrated scales, plain Python floats: f8_in_scale for the trunk it reads, f8_mid_scale for conv1's output.
"""
import contextlib
import json

import torch

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


def quantize(v, inv):
    """values -> e4m3fn codes: (v.float() * inv).clamp(-448, 448), one round-to-nearest-even conversion"""
    return (v.float() * inv).clamp(-FP8_MAX, FP8_MAX).to(FP8)


def inv_scale(s):
    """1 / s as the kernel gets it: one f32 division of the f32 value of s, as a Python float"""
    return float((1.0 / torch.tensor(float(s), dtype=torch.float32)).item())


def scale_of(absmax):
    """the stored scale of a tensor whose largest magnitude is absmax: absmax / 448, or 1 for an all-zero tensor"""
    absmax = float(absmax)
    return absmax / FP8_MAX if absmax > 0.0 else 1.0


def weight_scales(w_ohwi):
    """sw [Cout] f32 of an OHWI weight: absmax(w[o]) / 448, 1 for an all-zero channel"""
    amax = w_ohwi.float().abs().flatten(1).max(dim=1).values
    return torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))


def fold_scale(s_in, sw, bn_scale=None):
    """scale[Cout] f32 of the conv's epilogue: (f32(s_in) * sw) * bn_scale, every product rounded to f32"""
    v = torch.tensor(float(s_in), dtype=torch.float32, device=sw.device) * sw.float()
    return (v if bn_scale is None else v * bn_scale.float()).contiguous()


# ------------------------------------------------------------------------------------------------ the model's scales
def f8_blocks(model):
    """[(module name, block)] of the model's FP8 bottlenecks, in module order"""
    return [(n, m) for n, m in model.named_modules() if getattr(m, "f8", False)]


def scales(model):
    """{module name: {"in": f8_in_scale, "mid": f8_mid_scale}} of every FP8 block (None where not calibrated)"""
    return {n: {"in": m.f8_in_scale, "mid": m.f8_mid_scale} for n, m in f8_blocks(model)}


def load_scales(model, d):
    """sets the scales of every FP8 block from scales()'s dict (or its JSON file's path); a block without an entry, an entry
    without a block, or a scale that is not a positive finite number raises."""
    if isinstance(d, str):
        with open(d) as f:
            d = json.load(f)
    blocks = dict(f8_blocks(model))
    if set(blocks) != set(d):
        raise ValueError("FP8 scales do not match the model's FP8 blocks: missing %s, unknown %s"
                         % (sorted(set(blocks) - set(d)), sorted(set(d) - set(blocks))))
    for n, m in blocks.items():
        vals = []
        for k in ("in", "mid"):
            v = float(d[n][k])
            if not (v > 0.0 and v < float("inf")):
                raise ValueError("FP8 scale %s[%r] = %r is not a positive finite number" % (n, k, d[n][k]))
            vals.append(v)
        m.set_f8_scales(*vals)
    return model


class _Recorder(object):
    """what a calibration pass sees: the absmax of each FP8 block's input and conv1 output, over every call"""

    def __init__(self):
        self.amax = {}

    def __call__(self, block, x, t):
        a = self.amax.setdefault(id(block), [0.0, 0.0])
        a[0] = max(a[0], float(x.float().abs().max()))
        a[1] = max(a[1], float(t.float().abs().max()))


@contextlib.contextmanager
def _bypass(rec):
    from . import modeling
    prev = modeling._F8_RECORDER
    modeling._F8_RECORDER = rec
    try:
        yield
    finally:
        modeling._F8_RECORDER = prev


def calibrate(model, frames):
    """Runs the model's backbone in bf16 over `frames` -- FP8_CONV is bypassed inside this call -- records the absmax of each
    FP8 block's input and of its conv1 output, and sets  scale = absmax / 448  on the block.
    model: a detector or backbone (its ResNet body is run), or a single FP8 Bottleneck.  frames: what that module takes -- for a
    body a preprocessed f32 image batch [N,3,H,W], or the uint8 RGB frames [N,H,W,3] (preprocessed as the engines' stem does,
    with the model's cfg.INPUT mean); for a block the NHWC trunk tensor -- or a list of them (the absmax is over all).
    -> scales(model)."""
    from . import modeling
    blocks = f8_blocks(model)
    if not blocks:
        raise ValueError("the model has no FP8 block (cfg.FP8_CONV is 'off')")
    bodies = [m for m in model.modules() if isinstance(m, modeling.ResNet)]
    rec = _Recorder()
    batches = frames if isinstance(frames, (list, tuple)) else [frames]
    with torch.no_grad(), _bypass(rec):
        for b in batches:
            if bodies and b.dtype == torch.uint8:
                inp = model.cfg.INPUT
                bodies[0].run_nhwc(b, u8_norm=(tuple(inp.PIXEL_MEAN), bool(inp.TO_BGR255)))
            elif bodies:
                bodies[0].run_nhwc(b)
            elif isinstance(model, modeling.Bottleneck):
                model.run(b)
            else:
                raise ValueError("calibrate needs a model with a ResNet body, or one FP8 Bottleneck")
    for n, m in blocks:
        if id(m) not in rec.amax:
            raise RuntimeError("FP8 block %s was not reached by the calibration pass" % n)
        a_in, a_mid = rec.amax[id(m)]
        m.set_f8_scales(scale_of(a_in), scale_of(a_mid))
    return scales(model)
