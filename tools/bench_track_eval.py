"""Times the tubelet AP (mega.pytorch_amd.track_eval) on the seeded synthetic set of tools/bench_seq_nms.py, the size of
ImageNet VID val: 555 videos, 176,126 frames, 300 detections per frame over 30 classes, with the tracks the detections
were jittered around as ground-truth tracks.

  python tools/bench_track_eval.py [--videos 555] [--frames 176126] [--dets 300] [--warmup 1] [--repeats 3]
      [--tubelet-score mean|max] [--max-gap 1]

The detections are linked first (tracks.link, defaults, --max-gap), as tools/bench_tracks.py does; its linking times are
shown for context.  One JSON line: the device time of mega_tubelet_match (HIP events around the entry point; it does not
synchronise) and of the other two kernels of the evaluation, the wall time of track_eval.evaluate_tracks list[BoxList] ->
result (host checks and packing, copies in, the segment operations, the kernels, one copy back; median of the repeats
after the warm-up), the wall time of its host checks and packing alone, the task / tubelet / pair counts, and the result.
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
from bench_tracks import _timed  # noqa: E402


def groundtruth(s):
    """The set's GT tracks as a VIDTrackGroundTruth (annotations of the predictions' 640 x 480)."""
    from mega.pytorch_amd import vid_eval
    gt = vid_eval.VIDTrackGroundTruth.__new__(vid_eval.VIDTrackGroundTruth)
    gt.image_set_index = None
    F = len(s["gt_off"]) - 1
    gt._set(s["gt_box"], s["gt_label"], s["gt_off"], np.full(F, 480), np.full(F, 640))
    gt.track_ids = np.ascontiguousarray(s["gt_track"], np.int64)
    return gt


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--videos", type=int, default=555)
    ap.add_argument("--frames", type=int, default=176126)
    ap.add_argument("--dets", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-gap", type=int, default=1)
    ap.add_argument("--tubelet-score", choices=("mean", "max"), default="mean")
    a = ap.parse_args(argv)
    from mega.pytorch_amd import track_eval, tracks
    s = bench_seq_nms.make_set(a.videos, a.frames, a.dets, seed=a.seed)
    F = len(s["score"]) // a.dets
    preds = bench_seq_nms.to_boxlists(s)
    gt = groundtruth(s)
    dev = "cuda:0"
    times, fam, (linked, table) = _timed(lambda: tracks.link(preds, s["videos"], max_gap=a.max_gap, device=dev), a.warmup,
                                         a.repeats)
    res = {"metric": "tubelet_ap", "videos": len(s["videos"]), "frames": F, "boxes": len(s["score"]),
           "gt_boxes": int(len(s["gt_label"])), "host": platform.node(), "warmup": a.warmup,
           "link_kernel_ms": round(fam["link_tracks"], 3), "link_wall_s": round(float(np.median(times)), 4),
           "tracks": int(len(table))}
    del preds
    times, fam, out = _timed(lambda: track_eval.evaluate_tracks(linked, gt, s["videos"], tubelet_score=a.tubelet_score,
                                                                device=dev), a.warmup, a.repeats)
    t0 = time.perf_counter()
    mem, _, _, g, _ = track_eval._pack(linked, gt, s["videos"])
    pack_s = time.perf_counter() - t0
    r = track_eval.run(linked, gt, s["videos"], tubelet_score=a.tubelet_score, device=dev, pairs=True)
    pg = [v["hits"].size for v in r["pairs"].values()]
    res.update(tubelet_match_kernel_ms=round(fam["tubelet_match"], 3), tubelet_scores_kernel_ms=round(fam["tubelet_scores"], 3),
               ap_kernel_ms=round(fam["vid_eval_ap"], 3), eval_wall_s=round(float(np.median(times)), 4),
               eval_wall_times_s=[round(t, 4) for t in times], eval_host_pack_s=round(pack_s, 4),
               tubelet_boxes=int(mem["N"]), tubelets=int(len(r["tubelets"])), gt_tracks=int(g["J"]), tasks=len(pg),
               pairs=int(sum(pg)), largest_task_pairs=int(max(pg) if pg else 0), workspace_pairs=int(r["ws_pairs"]),
               thresholds=["%d/%d" % nd for nd in out["thresholds"]], map=[round(float(m), 4) for m in out["map"]],
               mean=round(float(out["mean"]), 4),
               gt_tracks_taken_at_half=int((out["gt_table"]["tubelet"] >= 0).sum()))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
