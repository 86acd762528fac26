"""Derives the motion IoU table of a VID-style index from its annotations' <trackid> tracks (mega.pytorch_amd.motion_iou)
and writes it in the layout of vid_groundtruth_motion_iou.mat, for eval_vid.py --motion-iou FILE.mat or the reference's
own --motion-specific evaluation.

  python tools/make_motion_iou.py --img-index ImageSets/VID_val_videos.txt --anno-path Annotations/VID/val \\
      --out motion_iou.mat [--window 10] [--compare vid_groundtruth_motion_iou.mat] [--cache gt.npz]

One JSON line: the frames, GT boxes, boxes without a neighbour and the share of the entries in fast / medium / slow; with
--compare REF.mat (a table of the same frames, e.g. the published file on the full val index) also motion_iou.compare's
numbers: the frames whose entry counts differ, the max and median |derived - REF| and the share of entries that land in
another range.  The derived values follow mega.pytorch_amd.motion_iou's definition; agreement with the published file
is what --compare measures, not something this tool assumes.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--img-index", required=True, help="the 4-column VID index file")
    ap.add_argument("--anno-path", required=True, help="directory of <video>/<frame>.xml annotations")
    ap.add_argument("--out", required=True, help="the .mat to write")
    ap.add_argument("--window", type=int, default=10, help="neighbour frames on each side (1 .. 64)")
    ap.add_argument("--compare", default=None, help="a motion IoU .mat of the same frames to compare with")
    ap.add_argument("--cache", default=None, help="optional .npz cache of the parsed annotations")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if not 1 <= a.window <= 64:
        ap.error("--window must be in 1 .. 64, got %d" % a.window)
    if not a.out.endswith(".mat"):
        ap.error("--out must end in .mat, got %r" % a.out)
    import numpy as np
    from mega.pytorch_amd import inference, motion_iou, vid_eval
    gt = vid_eval.VIDTrackGroundTruth(a.img_index, a.anno_path, cache=a.cache)
    values, counts = motion_iou.run(gt, inference.VIDTestIndex(a.img_index).videos, a.window, device=a.device)
    table = motion_iou.to_per_frame(values, gt.off)
    motion_iou.save_mat(a.out, table, off=gt.off)
    res = {"frames": len(gt), "gt_boxes": int(values.size), "window": a.window, "lone_boxes": int((counts == 0).sum()),
           "nan_values": int(np.isnan(values).sum())}
    allm = np.concatenate(table) if table else np.zeros(0)
    for name, (lo, hi) in zip(vid_eval.MOTION_NAMES[1:], vid_eval.MOTION_RANGES[1:]):
        res["share_" + name] = round(float(((allm >= lo) & (allm <= hi)).mean()), 6) if allm.size else 0.0
    if a.compare:
        res["compare"] = motion_iou.compare(table, vid_eval.load_motion_iou(a.compare))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
