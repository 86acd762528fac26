"""Times the detection error diagnosis (mega.pytorch_amd.diagnose) on the seeded synthetic set of tools/bench_eval.py, the
size of ImageNet VID val: 176,126 frames, 300 detections each, 0-12 GT boxes per frame.

  python tools/bench_diagnose.py [--frames 176126] [--dets 300] [--warmup 1] [--repeats 2] [--out FILE]

One JSON line (also written to --out): the device time of mega_diagnose_match and, on the same input, of the unchanged
mega_vid_eval_match for one range (R = 1, no motion list: the matching the diagnosis repeats as its first pass) and of
mega_vid_eval_ap for that one row -- HIP events around the entry points, which do not synchronise -- the device time of the
diagnosis' own two vid_eval_ap calls (6 rows + the cls row), and the wall time of diagnose.evaluate_errors list[BoxList] ->
result dict (host packing, one copy, sorts, kernels, copies back, host tables; median of the repeats after the warm-up).
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

import bench_eval  # noqa: E402  (the generator of the input set)
from bench_tracks import _timed  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=176126)
    ap.add_argument("--dets", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args(argv)
    import torch
    from mega.pytorch_amd import _lib, diagnose, vid_eval
    _lib.load()
    dev = "cuda:0"
    s = bench_eval.make_set(a.frames, a.dets, a.seed)
    preds, gt, _ = bench_eval.to_inputs(s)
    sys.stderr.write("bench_diagnose: set built (%d detections, %d GT boxes)\n" % (a.frames * a.dets, int(gt.off[-1])))
    times, fam, res = _timed(lambda: diagnose.evaluate_errors(preds, gt, device=dev), a.warmup, a.repeats)
    sys.stderr.write("bench_diagnose: evaluate_errors timed\n")
    _, fam1, ref = _timed(lambda: vid_eval.evaluate_detections(preds, gt, device=dev), a.warmup, 1)
    out = {"metric": "diagnose", "frames": a.frames, "dets_per_frame": a.dets, "detections": a.frames * a.dets,
           "gt_boxes": int(gt.off[-1]), "most_boxes_in_a_frame": int(np.diff(gt.off).max()), "host": platform.node(),
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "repeats": len(times),
           "diagnose_match_kernel_ms": round(fam["diagnose_match"], 3),
           "vid_eval_match_kernel_ms": round(fam1["vid_eval_match"], 3),
           "vid_eval_ap_kernel_ms": round(fam1["vid_eval_ap"], 3),
           "diagnose_ap_kernels_ms": round(fam["vid_eval_ap"], 3),
           "evaluate_errors_wall_s": round(float(np.median(times)), 4),
           "evaluate_errors_wall_times_s": [round(t, 4) for t in times],
           "map": None if np.isnan(res["map"]) else round(res["map"], 6),
           "map_equals_evaluate_detections": bool(res["map"] == ref[0]["map"]),
           "dap": {k: round(v, 6) for k, v in res["dap"].items()},
           "kind_counts": dict(zip(diagnose.KINDS, (int(v) for v in res["kind_counts"]))),
           "gt_state_counts": dict(zip(diagnose.GT_STATES, (int(v) for v in res["gt_state_counts"])))}
    line = json.dumps(out)
    print(line)
    if a.out:
        d = os.path.dirname(os.path.abspath(a.out))
        os.makedirs(d, exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
