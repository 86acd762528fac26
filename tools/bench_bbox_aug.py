"""Evidence for TEST.BBOX_AUG: prints ONE JSON line with
  merge_ms / merge_us_per_frame   mega_bbox_aug_merge on a VID-val-like synthetic chunk (16 frames x 4 views x 300 rows,
                                  31 classes, ~30 % of the candidates above the threshold), median of --reps events
  video_s                         wall time of one video (MEGA R-101 600x1000 bf16, synthetic frames through FrameSource)
                                  through inference.compute_on_dataset: plain, TEST.BBOX_AUG with the identity view alone
                                  (K = 1) and with 4 views (identity, flip, 500, its flip); each timed call includes its
                                  engine's graph captures
usage: python tools/bench_bbox_aug.py [--frames 120] [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def merge_time(dev, reps):
    from mega.pytorch_amd import ops
    g = torch.Generator(device=dev).manual_seed(0)
    K, F, C1, R = 4, 16, 30, 300
    sizes = [(1000, 600), (1000, 600), (833, 500), (833, 500)]
    flips = [False, True, False, True]
    ctr = torch.rand((K, F, C1, R, 2), generator=g, device=dev) * torch.tensor([800., 450.], device=dev)
    half = torch.rand((K, F, C1, R, 2), generator=g, device=dev) * 100 + 4
    cb = torch.cat([ctr - half, ctr + half], -1).clamp(min=0).contiguous()
    cs = torch.rand((K, F, C1, R), generator=g, device=dev)
    cs = torch.where(torch.rand(cs.shape, generator=g, device=dev) < 0.3, cs, torch.full_like(cs, -1.0)).contiguous()
    for _ in range(3):
        ops.bbox_aug_merge(cb, cs, sizes, flips, 0.001, 0.5, 300)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.bbox_aug_merge(cb, cs, sizes, flips, 0.001, 0.5, 300)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], F


def video_times(dev, T):
    import bench
    from mega.pytorch_amd import inference, synth
    cfg, model, _ = bench.build_model("R-101", "bfloat16", dev)
    host = synth.make_clip(16, 600, 1000, seed=0).numpy()
    videos = [{"start": 0, "pattern": "v/%06d", "seg_len": T}]
    kw = dict(source_kwargs={"opener": lambda f: host[f % 16]})
    out = {}
    legs = [("plain", None), ("k1", dict(H_FLIP=False, SCALES=(), SCALE_H_FLIP=False)),
            ("k4", dict(H_FLIP=True, SCALES=(500,), MAX_SIZE=1000, SCALE_H_FLIP=True))]
    for name, aug in legs:
        c = cfg.clone()
        if aug is not None:
            c.TEST.BBOX_AUG.ENABLED = True
            c.TEST.BBOX_AUG.update(aug)
        # two runs per leg, the second timed (host-side caches warm).  Every compute_on_dataset call builds its own
        # engine, so the timed run includes that engine's graph captures, in every leg alike; the views of one call
        # share the engine as consecutive videos do
        for rep in range(2):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            res = inference.compute_on_dataset(model, None, "", dev, videos=videos,
                                               bbox_aug_cfg=c if aug is not None else None, **kw)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
        out[name] = round(dt, 3)
        out[name + "_dets"] = sum(len(r) for r in res.values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ms, F = merge_time(dev, a.reps)
    v = video_times(dev, a.frames)
    print(json.dumps({"merge_ms": round(ms, 3), "merge_frames": F, "merge_us_per_frame": round(1000 * ms / F, 1),
                      "video_frames": a.frames, "video_s": v,
                      "k4_over_plain": round(v["k4"] / v["plain"], 2), "k1_over_plain": round(v["k1"] / v["plain"], 3)}))


if __name__ == "__main__":
    main()
