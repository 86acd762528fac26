"""cfg.FP8_CONV = "layer3" on the benchmarked configuration against the f32 oracle: the sibling of
test_e2e_gpu.py::test_r101_600x1000_bf16_vs_oracle (-m gpu)."""
import pytest
import torch

from test_e2e_gpu import _bf16_metrics, _fmt, _model, _r101_fixture

pytestmark = pytest.mark.gpu

CALIBRATION_FRAMES = 4


def f8_run(dev):
    """28 key frames of the R-101 600x1000 fixture clip, all bf16 with layer3's identity blocks in FP8, the scales calibrated on
    the clip's own first frames; -> {kept key frame: _bf16_metrics against the f32 oracle}"""
    from mega.pytorch_amd import engine, f8, modeling
    d, gen = _r101_fixture()
    sd, clip, gfor = gen.inputs()
    nkey, T = int(d["cfg_nkey"]), int(d["cfg_T"])
    cfg, base = _model(dev, "bfloat16", strict_gt=True, arch="R-101", sd=sd)
    del base
    cfg = cfg.clone()
    cfg.FP8_CONV = "layer3"
    model = modeling.build_detection_model(cfg)
    model.load_state_dict(sd)
    model.to(dev)
    clip = clip.to(dev)
    sc = f8.calibrate(model, clip[:CALIBRATION_FRAMES])
    assert len(sc) == 22 and all(v["in"] > 0 and v["mid"] > 0 for v in sc.values())
    eng = engine.ClipEngine(model, steps_per_batch=4, keep_logits=True)
    dets = eng.run(clip, T, gfor, first=0, last=nkey)
    out = {}
    for idx in [int(k) for k in d["keep"]]:
        out[idx] = _bf16_metrics(d, idx, eng.key_boxes_log[idx].cpu().numpy(), eng.logits_log[idx].cpu().numpy(), dets[idx])
    del eng, model
    torch.cuda.empty_cache()
    return out


def test_r101_600x1000_fp8_layer3_vs_oracle(dev):
    """All bf16 with conv1 / conv2 of layer3's 22 identity blocks on FP8 operands (per-tensor activation scales calibrated on the
    clip's first four frames, per-channel weight scales) against the f32 oracle on the kept key frames, incl. the memory-full
    regime.  MEASURED on MI355X, three runs on one box (bit-identical): proposals IoU-matched 75.0-77.0 %, matched-box median
    0.47-0.51 px, logit |err| median 4.92-5.31e-3 / p99 1.83-2.02e-2 on a scale of 1.13, detections matched 51.3-59.3 % -- the
    bf16 sibling in the same session: 90.0-94.0 %, 0.10-0.11 px, 1.53-1.78e-3 / 6.9-8.3e-3, 78.0-80.3 %.  On this seeded
    random-weight fixture every class score is a near-tie, so a detection flips easily (test_r101_bf16_attribution); no claim
    about trained weights follows.  Bounds by the sibling's convention: worst run minus two points for the matched shares; for
    the errors the sibling's own ratio of bound to its worst measurement (median 2.0e-3 / 1.78e-3, p99 9.5e-3 / 8.26e-3, box
    median 0.125 / 0.114).  The run takes about as long as the sibling's (2.4 s against 1.8 s after the fixture is built)."""
    B = f8_run(dev)
    for idx, m in sorted(B.items()):
        print(_fmt("fp8-layer3", idx, m))
    for idx, m in sorted(B.items()):
        sc = max(1.0, m["scale"])
        assert m["overlap"] >= BOUNDS["overlap"], "key frame %d: only %.1f%% of the proposals match an oracle proposal" % (idx, 100 * m["overlap"])
        assert m["dbox_med"] < BOUNDS["dbox_med"]
        assert m["l_med"] < BOUNDS["l_med"] * sc and m["l_p99"] < BOUNDS["l_p99"] * sc
        assert m["dmatch"] >= BOUNDS["dmatch"]


# worst of the three runs -> bound: 75.0 % - 2; 0.513 px * 0.125 / 0.114; 5.31e-3 * 2.0 / 1.78; 2.02e-2 * 9.5 / 8.26; 51.3 % - 2
BOUNDS = {"overlap": 0.73, "dbox_med": 0.562, "l_med": 5.96e-3, "l_p99": 2.32e-2, "dmatch": 0.49}
