"""Evidence for cfg.FP8_CONV (README "Arithmetic modes"): prints ONE JSON line with
  kernels     conv1 (1x1, 1024 -> 256) and conv2 (3x3, 256 -> 256) of one layer3 identity block at the headline shape, 40 frames
              of 38 x 63 (M = 95,760 rows): the FP8 launch (ops.conv2d_nhwc_f8: bf16 in -> fp8 out, fp8 in -> bf16 out) beside the
              existing bf16 launch (ops.conv2d_nhwc) of the same layer, in the same process.  HIP events around --inner
              back-to-back launches, --reps windows per leg, the legs alternating inside every repetition; median and min-max.
  e2e         bench.py's workload (MEGA R-101, 600 x 1000, bf16, its engine settings and pre-roll) with FP8_CONV off and on:
              two engines in one process, timed blocks of --steps key frames alternating between them; median key frames/s
              and min-max per leg.  The scales are calibrated on the clip's first four frames.
  parity      (--parity, needs tests/golden's R-101 fixture) both legs against the f32 oracle: proposals IoU-matched, logit
              error median / p99, detections matched, worst kept key frame.
No GPU, no number: this tool has no fallback.
usage: python tools/bench_f8.py [--reps 15] [--inner 20] [--steps 60] [--blocks 5] [--parity] [--no-e2e] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, FH, FW = 40, 38, 63


def _stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1]}


def kernel_times(dev, reps, inner):
    from mega.pytorch_amd import f8, ops
    g = torch.Generator().manual_seed(0)
    x = torch.randn((FRAMES, FH, FW, 1024), generator=g).clamp(min=0).to(torch.bfloat16).to(dev)
    w1 = torch.randn((256, 1, 1, 1024), generator=g) / 32.0
    w2 = torch.randn((256, 3, 3, 256), generator=g) / 48.0
    one, zero = torch.ones(256, device=dev), torch.zeros(256, device=dev)
    w1b, w2b = w1.to(torch.bfloat16).to(dev), w2.to(torch.bfloat16).to(dev)
    (q1, sw1), (q2, sw2) = ops.pack_conv_weight_f8(w1), ops.pack_conv_weight_f8(w2)
    q1, q2 = q1.to(dev), q2.to(dev)
    s_in = f8.scale_of(float(x.float().abs().max()))
    t_bf = ops.conv2d_nhwc(x, w1b, one, zero, relu=True)
    s_mid = f8.scale_of(float(t_bf.float().abs().max()))
    sc1, sc2 = f8.fold_scale(s_in, sw1.to(dev)), f8.fold_scale(s_mid, sw2.to(dev))
    t_f8 = ops.conv2d_nhwc_f8(x, q1, sc1, zero, in_scale=s_in, out_scale=s_mid, relu=True)
    o1b, o1f = torch.empty_like(t_bf), torch.empty_like(t_f8)
    o2b = torch.empty_like(t_bf)
    o2f = torch.empty_like(t_bf)
    legs = [("conv1_bf16", lambda: ops.conv2d_nhwc(x, w1b, one, zero, relu=True, out=o1b)),
            ("conv1_f8", lambda: ops.conv2d_nhwc_f8(x, q1, sc1, zero, in_scale=s_in, out_scale=s_mid, relu=True, out=o1f)),
            ("conv2_bf16", lambda: ops.conv2d_nhwc(t_bf, w2b, one, zero, pad=1, relu=True, out=o2b)),
            ("conv2_f8", lambda: ops.conv2d_nhwc_f8(t_f8, q2, sc2, zero, pad=1, relu=True, out=o2f))]
    for _, fn in legs:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in legs}
    for _ in range(reps):
        for name, fn in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / inner)
    out = {"shape": {"frames": FRAMES, "H": FH, "W": FW, "rows": FRAMES * FH * FW}, "reps": reps, "inner": inner,
           "ms": {k: _stats(v) for k, v in ms.items()}}
    M = FRAMES * FH * FW
    for name, K in (("conv1", 1024), ("conv2", 9 * 256)):
        fl = 2.0 * M * 256 * K
        out["ms"][name + "_f8"]["tflops"] = fl / out["ms"][name + "_f8"]["median"] * 1e-9
        out["ms"][name + "_bf16"]["tflops"] = fl / out["ms"][name + "_bf16"]["median"] * 1e-9
        out[name + "_speedup"] = out["ms"][name + "_bf16"]["median"] / out["ms"][name + "_f8"]["median"]
    # (the difference of the two conv2 outputs, as a share of the largest bf16 output: the FP8 legs computed the layer)
    out["conv2_max_rel_diff"] = float((o2f.float() - o2b.float()).abs().max() / o2b.float().abs().max())
    return out


def e2e(dev, steps, blocks):
    import bench
    from mega.pytorch_amd import engine as eng, f8, modeling
    cfg, off, sd = bench.build_model("R-101", "bfloat16", dev)
    cfg_on = cfg.clone()
    cfg_on.FP8_CONV = "layer3"
    on = modeling.build_detection_model(cfg_on)
    on.load_state_dict(sd)
    on.to(dev)
    KF = bench.key_frames_per_block(steps, 1)
    spb = bench.default_steps_per_batch(steps, 1)
    afi = cfg.MODEL.VID.MEGA.ALL_FRAME_INTERVAL
    pre = max(40, afi + 12 + 1, 3 * spb + 1)
    pre = 1 + -(-(pre - 1) // spb) * spb
    T = pre + KF * (3 + blocks) + 14
    clip = bench.make_clip(T, 600, 1000, dev)
    gfor = eng.global_schedule(T, cfg.MODEL.VID.MEGA.GLOBAL.SIZE, seed=0)
    f8.calibrate(on, clip[:4])
    runners = {}
    for name, model in (("off", off), ("on", on)):
        r = eng.ClipEngine(model, steps_per_batch=spb)
        r.run(clip, T, gfor, first=0, last=1)
        pos = 1
        while pos < pre + 2 * KF:
            r.run(clip, T, gfor, first=pos, last=pos + KF)
            torch.cuda.synchronize()
            pos += KF
        runners[name] = [r, pos]
    fps = {"off": [], "on": []}
    for _ in range(blocks):
        for name in ("off", "on"):
            r, pos = runners[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.run(clip, T, gfor, first=pos, last=pos + KF)
            torch.cuda.synchronize()
            fps[name].append(KF / (time.perf_counter() - t0))
            runners[name][1] = pos + KF
    out = {"steps": steps, "blocks": blocks, "steps_per_batch": spb, "key_frames_per_s": {k: _stats(v) for k, v in fps.items()}}
    out["on_over_off"] = out["key_frames_per_s"]["on"]["median"] / out["key_frames_per_s"]["off"]["median"]
    return out


def parity(dev):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_e2e_gpu as e
    import test_f8_e2e_gpu as t
    runs = {"off": e._r101_mixed_run(dev, "bfloat16", "bfloat16"), "on": t.f8_run(dev)}
    out = {}
    for name, r in runs.items():
        out[name] = {"proposals_matched_min": min(m["overlap"] for m in r.values()),
                     "logit_err_median_max": max(m["l_med"] for m in r.values()),
                     "logit_err_p99_max": max(m["l_p99"] for m in r.values()),
                     "detections_matched_min": min(m["dmatch"] for m in r.values()),
                     "logit_scale": max(m["scale"] for m in r.values()), "key_frames": sorted(r)}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_f8 needs an MI355X: no HIP device, no number")
    dev = torch.device("cuda:0")
    line = {"tool": "bench_f8", "device": torch.cuda.get_device_name(0), "kernels": kernel_times(dev, args.reps, args.inner)}
    if not args.no_e2e:
        line["e2e"] = e2e(dev, args.steps, args.blocks)
    if args.parity:
        line["parity"] = parity(dev)
    line["note"] = "seeded random weights and a synthetic clip: no claim about real VID weights (no dataset on the bench machines)"
    text = json.dumps(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
