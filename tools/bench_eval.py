"""Times the VID evaluation (mega.pytorch_amd.vid_eval) on a seeded synthetic set the size of ImageNet VID val:
176,126 frames, 300 detections each, 0-12 GT boxes per frame with motion IoUs in [0, 1], motion-specific (4 ranges).

  python tools/bench_eval.py [--frames 176126] [--dets 300] [--warmup 1] [--repeats 5]
      wall time list[BoxList] -> result dict (host packing, one copy, sorts, kernels, synchronise): median of the
      repeats after the warm-up; one JSON line.  Kernel times: run it under  rocprofv3 --kernel-trace --stats -- ...
  python tools/bench_eval.py --reference-cpu --subset 2000
      CPU only, never on the GPU path: the reference's own calc_detection_vid_prec_rec / calc_detection_vid_ap (loaded
      as tests/golden/make_vid_eval.py does, so the reference tree must be present) on the first --subset frames of the
      same set, 4 ranges; reports the measured time and a LINEAR EXTRAPOLATION to the full frame count, with the host.
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_set(frames, dets, seed=0):
    """flat arrays of the synthetic set: detections jittered around GT boxes plus clutter, 375 x 500 annotations,
    predictions in a 600 x 800 frame."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 13, frames)
    G = int(g.sum())
    gt_off = np.zeros(frames + 1, np.int64)
    gt_off[1:] = np.cumsum(g)
    x1, y1 = rng.uniform(0, 380, G), rng.uniform(0, 280, G)
    gt_box = np.round(np.stack([x1, y1, np.minimum(x1 + rng.uniform(10, 200, G), 499),
                                np.minimum(y1 + rng.uniform(10, 150, G), 374)], 1)).astype(np.float32)
    gt_label = rng.integers(1, 31, G)
    motion = rng.uniform(0, 1, G)
    N = frames * dets
    fid = np.repeat(np.arange(frames), dets)
    has = g[fid] > 0
    src = gt_off[fid] + (rng.integers(0, 1 << 30, N) % np.maximum(g[fid], 1))
    src = np.where(has, src, 0)
    near = has & (rng.random(N) < 0.3)
    box = np.where(near[:, None], gt_box[np.minimum(src, max(G - 1, 0))] + rng.normal(0, 6, (N, 4)),
                   rng.uniform(0, 400, (N, 4))).astype(np.float32)
    box = np.sort(box.reshape(N, 2, 2), axis=1).reshape(N, 4)
    box = np.clip(box, 0, [499, 374, 499, 374]).astype(np.float32) * np.float32(1.6)
    label = np.where(near, gt_label[np.minimum(src, max(G - 1, 0))], rng.integers(1, 31, N)).astype(np.int64)
    score = rng.random(N).astype(np.float32)
    return {"box": box, "score": score, "label": label, "gt_box": gt_box, "gt_label": gt_label, "gt_off": gt_off,
            "motion": motion, "frames": frames, "dets": dets}


def to_inputs(s, frames=None):
    import torch
    from mega.pytorch_amd import vid_eval
    from mega.pytorch_amd.structures import BoxList
    F, D = s["frames"] if frames is None else frames, s["dets"]
    boxes = torch.from_numpy(s["box"][:F * D]).split(D)
    scores = torch.from_numpy(s["score"][:F * D]).split(D)
    labels = torch.from_numpy(s["label"][:F * D]).split(D)
    preds = []
    for b, sc, lb in zip(boxes, scores, labels):
        p = BoxList(b, (800, 600))
        p.add_field("scores", sc)
        p.add_field("labels", lb)
        preds.append(p)
    off = s["gt_off"][:F + 1]
    gt = vid_eval.VIDGroundTruth.from_annotations([])
    gt._set(s["gt_box"][:off[-1]], s["gt_label"][:off[-1]], off, np.full(F, 375), np.full(F, 500))
    motion = [s["motion"][off[i]:off[i + 1]] if off[i + 1] > off[i] else np.zeros(1) for i in range(F)]
    return preds, gt, motion


def run_gpu(a):
    import torch
    from mega.pytorch_amd import _lib, vid_eval
    _lib.load()
    t0 = time.perf_counter()
    s = make_set(a.frames, a.dets, a.seed)
    preds, gt, motion = to_inputs(s)
    t_setup = time.perf_counter() - t0
    times, res = [], None
    for i in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = vid_eval.evaluate_detections(preds, gt, motion_iou=motion, device="cuda:0")
        torch.cuda.synchronize()
        if i >= a.warmup:
            times.append(time.perf_counter() - t)
    print(json.dumps({"metric": "vid_eval_wall_s", "frames": a.frames, "dets_per_frame": a.dets,
                      "detections": a.frames * a.dets, "gt_boxes": int(s["gt_off"][-1]), "ranges": 4,
                      "median_s": float(np.median(times)), "min_s": float(np.min(times)), "repeats": len(times),
                      "warmup": a.warmup, "setup_s": round(t_setup, 2),
                      "map": [None if np.isnan(res[k]["map"]) else round(float(res[k]["map"]), 6) for k in range(4)],
                      "device": torch.cuda.get_device_name(0)}))


def run_reference_cpu(a):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import torch
    import make_vid_eval
    ve = make_vid_eval.load_ref_vid_eval()
    from mega_core.structures.bounding_box import BoxList as RefBoxList
    s = make_set(a.frames, a.dets, a.seed)
    F, D = a.subset, a.dets
    pred_bl, gt_bl = [], []
    for f in range(F):
        b = RefBoxList(torch.from_numpy(s["box"][f * D:(f + 1) * D]), (800, 600), mode="xyxy")
        b.add_field("scores", torch.from_numpy(s["score"][f * D:(f + 1) * D]))
        b.add_field("labels", torch.from_numpy(s["label"][f * D:(f + 1) * D]))
        pred_bl.append(b)
        o0, o1 = s["gt_off"][f], s["gt_off"][f + 1]
        t = RefBoxList(torch.from_numpy(s["gt_box"][o0:o1]).reshape(-1, 4), (500, 375), mode="xyxy")
        t.add_field("labels", torch.from_numpy(s["gt_label"][o0:o1]))
        gt_bl.append(t)
    motion = [list(s["motion"][s["gt_off"][f]:s["gt_off"][f + 1]]) or [0.0] for f in range(F)]
    import contextlib
    import io
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):      # the reference prints n_pos per range
        preds = [p.resize((500, 375)) for p in pred_bl]
        for r in [[0.0, 1.0], [0.0, 0.7], [0.7, 0.9], [0.9, 1.0]]:
            prec, rec = ve.calc_detection_vid_prec_rec(gt_boxlists=gt_bl, pred_boxlists=preds, motion_ious=motion,
                                                       iou_thresh=0.5, motion_range=r)
            ve.calc_detection_vid_ap(prec, rec)
    dt = time.perf_counter() - t0
    print(json.dumps({"metric": "reference_cpu_eval_s", "subset_frames": F, "dets_per_frame": D, "ranges": 4,
                      "measured_s": round(dt, 2), "extrapolated_full_s": round(dt * a.frames / F, 1),
                      "extrapolation": "linear in frames, %d -> %d" % (F, a.frames), "host": platform.node(),
                      "platform": platform.platform(), "cpus": os.cpu_count(), "torch_threads": torch.get_num_threads()}))


def main():
    ap = argparse.ArgumentParser(description="VID evaluation timing")
    ap.add_argument("--frames", type=int, default=176126)
    ap.add_argument("--dets", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reference-cpu", action="store_true")
    ap.add_argument("--subset", type=int, default=2000)
    a = ap.parse_args()
    if a.reference_cpu:
        run_reference_cpu(a)
    else:
        run_gpu(a)


if __name__ == "__main__":
    main()
