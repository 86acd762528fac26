"""ImageNet VID evaluation of a saved predictions.pth: AP50 (and motion-specific AP) -> result.txt.  The counterpart of
the reference's inference_no_model (mega_core/engine/inference.py:135-160), matching on the GPU (mega.pytorch_amd.vid_eval).

  python tools/eval_vid.py --predictions OUT/predictions.pth --img-index ImageSets/VID_val_videos.txt \\
      --anno-path Annotations/VID/val [--motion-iou vid_groundtruth_motion_iou.mat] [--output-folder OUT] [--cache gt.npz]

predictions.pth may be written by this package or by the reference.  result.txt goes to --output-folder (default: the
folder of predictions.pth); the text is also printed.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--predictions", required=True, help="predictions.pth (list[BoxList])")
    ap.add_argument("--img-index", required=True, help="the 4-column VID index file the predictions were made on")
    ap.add_argument("--anno-path", required=True, help="directory of <video>/<frame>.xml annotations")
    ap.add_argument("--motion-iou", default=None, help="vid_groundtruth_motion_iou.mat: adds fast / medium / slow AP")
    ap.add_argument("--output-folder", default=None, help="where result.txt goes (default: next to predictions.pth)")
    ap.add_argument("--cache", default=None, help="optional .npz cache of the parsed annotations")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    from mega.pytorch_amd import inference, vid_eval
    preds = inference.load_predictions(a.predictions)
    gt = vid_eval.VIDGroundTruth(a.img_index, a.anno_path, cache=a.cache)
    motion = vid_eval.load_motion_iou(a.motion_iou) if a.motion_iou else None
    out = a.output_folder or os.path.dirname(os.path.abspath(a.predictions))
    res = vid_eval.evaluate_detections(preds, gt, motion_iou=motion, output_folder=out, device=a.device)
    sys.stdout.write(vid_eval.format_result(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
