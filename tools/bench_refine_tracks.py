"""Times track refinement (mega.pytorch_amd.tracks.refine) on the seeded synthetic set of tools/bench_tracks.py, the size
of ImageNet VID val: 555 videos, 176,126 frames, 300 detections per frame over 30 classes, linked by tracks.link first.

  python tools/bench_refine_tracks.py [--videos 555] [--frames 176126] [--dets 300] [--warmup 1] [--repeats 3]
      [--smooth 2] [--fill-scale 1.0] [--no-fill] [--max-gap 1]

One JSON line: the device time of the refinement kernel (HIP events around mega_refine_tracks) with that of the linking
kernel beside it, the wall time of tracks.refine list[BoxList] -> list[BoxList] (host checks and the member sort, one copy
in, the kernel, the scatter back, one copy back, the per-frame assembly; median of the repeats after the warm-up), the
output box count, the filled count, the slot count, and the device time of copying the kernel's output arrays once (a
device-to-device copy of arrays of that size, HIP events, in the same run): the memory floor the kernel is compared against.
"""
import argparse
import json
import os
import platform
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_seq_nms  # noqa: E402  (the generator of the input set)
from bench_tracks import _timed  # noqa: E402


def _copy_ms(slots, dev, repeats=5):
    """The device time of one copy of the kernel's per-slot outputs (box 16 + score 4 + frame 4 + track 4 + src 4 + filled 1
    bytes a slot): the best of `repeats` after a warm-up."""
    import torch
    src = torch.zeros(max(slots, 1) * 33, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    best = None
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return best


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--videos", type=int, default=555)
    ap.add_argument("--frames", type=int, default=176126)
    ap.add_argument("--dets", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-gap", type=int, default=1, help="of the linking that makes the input")
    ap.add_argument("--no-fill", action="store_true")
    ap.add_argument("--smooth", type=int, default=2)
    ap.add_argument("--fill-scale", type=float, default=1.0)
    a = ap.parse_args(argv)
    from mega.pytorch_amd import tracks
    s = bench_seq_nms.make_set(a.videos, a.frames, a.dets, seed=a.seed)
    F = len(s["score"]) // a.dets
    preds = bench_seq_nms.to_boxlists(s)
    dev = "cuda:0"
    _, fam_link, (linked, table) = _timed(lambda: tracks.link(preds, s["videos"], max_gap=a.max_gap, device=dev), 0, 1)
    kw = dict(fill=not a.no_fill, smooth=a.smooth, fill_scale=a.fill_scale)
    times, fam, (out, info) = _timed(lambda: tracks.refine(linked, s["videos"], device=dev, **kw), a.warmup, a.repeats)
    slots = int(table["count"].sum()) + info["filled"]
    res = {"metric": "tracks_refine", "videos": len(s["videos"]), "frames": F, "boxes": len(s["score"]),
           "host": platform.node(), "warmup": a.warmup, "params": dict(kw, max_gap=a.max_gap),
           "refine_kernel_ms": round(fam["refine_tracks"], 3), "link_kernel_ms": round(fam_link["link_tracks"], 3),
           "refine_wall_s": round(float(np.median(times)), 4), "refine_wall_times_s": [round(t, 4) for t in times],
           "tracks": info["tracks"], "slots": slots, "filled": info["filled"], "output_boxes": int(sum(len(p) for p in out)),
           "copy_outputs_ms": round(_copy_ms(slots, dev), 3)}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
