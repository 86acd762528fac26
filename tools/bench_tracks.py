"""Times track linking (mega.pytorch_amd.tracks) on the seeded synthetic set of tools/bench_seq_nms.py, the size of
ImageNet VID val: 555 videos, 176,126 frames, 300 detections per frame over 30 classes.

  python tools/bench_tracks.py [--videos 555] [--frames 176126] [--dets 300] [--warmup 1] [--repeats 3]
      [--score-thresh 0.05] [--link-iou 0.5] [--max-gap 1] [--min-len 1] [--rescore none|avg|max]

One JSON line: the device time of the linking kernel (HIP events around mega_link_tracks, which include its status read-
back), the wall time of tracks.link list[BoxList] -> list[BoxList] (host packing and checks, one copy in, the sorts, the
kernel, the id / rescoring segment operations, one copy back, the per-frame split; median of the repeats after the warm-
up), the number of tracks, and for context the wall time of seq_nms.seq_nms and the device time of its kernel on the same
input (--no-seq-nms skips them).
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


def _timed(fn, warmup, repeats):
    """-> (wall times of the repeats, device ms per kernel family of the last repeat, fn's last result)"""
    import torch
    from mega.pytorch_amd import ops
    times, fam, out = [], {}, None
    for r in range(warmup + repeats):
        prof = ops.Profiler() if r == warmup + repeats - 1 else None
        ops.set_profiler(prof)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            ops.set_profiler(None)
        if r >= warmup:
            times.append(dt)
        if prof is not None:
            fam = {k: v["ms"] for k, v in prof.summary().items()}
    return times, fam, out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--videos", type=int, default=555)
    ap.add_argument("--frames", type=int, default=176126)
    ap.add_argument("--dets", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--score-thresh", type=float, default=0.05)
    ap.add_argument("--link-iou", type=float, default=0.5)
    ap.add_argument("--max-gap", type=int, default=1)
    ap.add_argument("--min-len", type=int, default=1)
    ap.add_argument("--rescore", choices=("none", "avg", "max"), default="avg")
    ap.add_argument("--no-seq-nms", action="store_true", help="do not time Seq-NMS on the same input")
    a = ap.parse_args(argv)
    from mega.pytorch_amd import seq_nms, tracks
    s = bench_seq_nms.make_set(a.videos, a.frames, a.dets, seed=a.seed)
    F = len(s["score"]) // a.dets
    preds = bench_seq_nms.to_boxlists(s)
    dev = "cuda:0"
    kw = dict(score_thresh=a.score_thresh, link_iou=a.link_iou, max_gap=a.max_gap, min_len=a.min_len,
              rescore=None if a.rescore == "none" else a.rescore)
    times, fam, (out, table) = _timed(lambda: tracks.link(preds, s["videos"], device=dev, **kw), a.warmup, a.repeats)
    res = {"metric": "tracks_link", "videos": len(s["videos"]), "frames": F, "boxes": len(s["score"]),
           "longest_video": max(n for _, n in s["videos"]), "host": platform.node(), "warmup": a.warmup,
           "params": dict(kw, rescore=a.rescore), "link_kernel_ms": round(fam["link_tracks"], 3),
           "link_wall_s": round(float(np.median(times)), 4), "link_wall_times_s": [round(t, 4) for t in times],
           "tracks": int(len(table)), "tracks_of_10_or_more": int((table["count"] >= 10).sum()),
           "linked_boxes": int(table["count"].sum())}
    if not a.no_seq_nms:
        times, fam, kept = _timed(lambda: seq_nms.seq_nms(preds, s["videos"], device=dev), a.warmup, a.repeats)
        res.update(seq_nms_kernel_ms=round(fam["seq_nms"], 3), seq_nms_wall_s=round(float(np.median(times)), 4),
                   seq_nms_kept=int(sum(len(p) for p in kept)))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
