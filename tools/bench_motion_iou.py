"""Times the motion IoU derivation (mega.pytorch_amd.motion_iou) on the seeded synthetic set of tools/bench_seq_nms.py, the
size of ImageNet VID val: 555 videos, 176,126 frames, with the tracks the detections were jittered around as ground-truth
tracks (the GT of tools/bench_track_eval.py).

  python tools/bench_motion_iou.py [--videos 555] [--frames 176126] [--dets 300] [--window 10] [--warmup 1] [--repeats 3]
      [--twin-videos 5]

One JSON line: the device time of mega_motion_iou (HIP events around the entry point; it does not synchronise), the wall
time of motion_iou.derive ground truth -> per-frame lists (host checks, one copy in, the kernel, one copy back, the
per-frame split; median of the repeats after the warm-up) and of its host checks alone, and for scale the wall time of the
motion-specific vid_eval.evaluate_detections on the same set with the derived table (--dets detections per frame;
--no-eval skips it) and the wall time of the numpy twin (tests/motion_iou_twin.py) on the first --twin-videos videos,
scaled to the whole set by frame count.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_seq_nms  # noqa: E402  (the generator of the input set)
from bench_track_eval import groundtruth  # noqa: E402
from bench_tracks import _timed  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--videos", type=int, default=555)
    ap.add_argument("--frames", type=int, default=176126)
    ap.add_argument("--dets", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--twin-videos", type=int, default=5, help="videos the numpy twin is timed on (0: skip)")
    ap.add_argument("--no-eval", action="store_true", help="do not time the motion-specific evaluate_detections")
    a = ap.parse_args(argv)
    from mega.pytorch_amd import motion_iou, vid_eval
    s = bench_seq_nms.make_set(a.videos, a.frames, a.dets, seed=a.seed)
    gt = groundtruth(s)
    F = len(gt)
    dev = "cuda:0"
    times, fam, table = _timed(lambda: motion_iou.derive(gt, s["videos"], a.window, device=dev), a.warmup, a.repeats)
    t0 = time.perf_counter()
    motion_iou._pack(gt, s["videos"], a.window)
    pack_s = time.perf_counter() - t0
    values, counts = motion_iou.run(gt, s["videos"], a.window, device=dev)
    allm = np.concatenate(table)
    res = {"metric": "motion_iou_derive", "videos": len(s["videos"]), "frames": F, "gt_boxes": int(values.size),
           "window": a.window, "host": platform.node(), "warmup": a.warmup,
           "motion_iou_kernel_ms": round(fam["motion_iou"], 3), "derive_wall_s": round(float(np.median(times)), 4),
           "derive_wall_times_s": [round(t, 4) for t in times], "derive_host_checks_s": round(pack_s, 4),
           "pairs_found": int(counts.sum()), "lone_boxes": int((counts == 0).sum()),
           "most_boxes_in_a_frame": int(np.diff(gt.off).max())}
    for name, (lo, hi) in zip(vid_eval.MOTION_NAMES[1:], vid_eval.MOTION_RANGES[1:]):
        res["share_" + name] = round(float(((allm >= lo) & (allm <= hi)).mean()), 4)
    if a.twin_videos > 0:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import motion_iou_twin
        sub = s["videos"][:a.twin_videos]
        hi = sub[-1][0] + sub[-1][1]
        g1 = int(gt.off[hi])
        t0 = time.perf_counter()
        tv, tc = motion_iou_twin.run(gt.boxes[:g1], gt.off[:hi + 1], gt.track_ids[:g1], sub, a.window)
        twin_s = time.perf_counter() - t0
        res.update(twin_videos=len(sub), twin_frames=hi, twin_wall_s=round(twin_s, 3),
                   twin_wall_scaled_s=round(twin_s * F / hi, 1),
                   twin_bit_identical=bool((tv.view(np.int64) == values[:g1].view(np.int64)).all() and
                                           (tc == counts[:g1]).all()))
    if not a.no_eval:
        preds = bench_seq_nms.to_boxlists(s)
        times, fam, _ = _timed(lambda: vid_eval.evaluate_detections(preds, gt, motion_iou=table, device=dev), a.warmup,
                               a.repeats)
        res.update(dets_per_frame=a.dets, eval_motion_wall_s=round(float(np.median(times)), 4),
                   eval_match_kernel_ms=round(fam.get("vid_eval_match", float("nan")), 3),
                   eval_ap_kernel_ms=round(fam.get("vid_eval_ap", float("nan")), 3))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
