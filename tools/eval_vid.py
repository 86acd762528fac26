"""ImageNet VID evaluation of a saved predictions.pth: AP50 (and motion-specific AP) -> result.txt.  The counterpart of
the reference's inference_no_model (mega_core/engine/inference.py:135-160), matching on the GPU (mega.pytorch_amd.vid_eval).

  python tools/eval_vid.py --predictions OUT/predictions.pth --img-index ImageSets/VID_val_videos.txt \\
      --anno-path Annotations/VID/val [--motion-iou vid_groundtruth_motion_iou.mat | derive] [--output-folder OUT]
      [--cache gt.npz]

predictions.pth may be written by this package or by the reference.  result.txt goes to --output-folder (default: the
folder of predictions.pth); the text is also printed.

--motion-iou derive (the literal word instead of a path; with --motion-window N, default 10) derives the motion IoU table
from the annotations' <trackid> tracks (mega.pytorch_amd.motion_iou) instead of reading the file, so that motion-specific
AP works on any subset of videos or VID-style dataset; the table goes to every evaluation of the run (raw, --seq-nms,
--tracks).  --save-motion-iou PATH also writes it as a .mat in the file's layout.

--seq-nms (with --seq-nms-link-iou / --seq-nms-iou / --seq-nms-rescore) also applies Seq-NMS (mega.pytorch_amd.seq_nms)
over the videos of --img-index, writes predictions_seq_nms.pth and result_seq_nms.txt to the output folder and prints
that evaluation too.

--tracks (with --tracks-score-thresh / --tracks-link-iou / --tracks-max-gap / --tracks-min-len / --tracks-rescore) links
the detections (what Seq-NMS kept, with --seq-nms) into tracks (mega.pytorch_amd.tracks): predictions_tracks.pth with the
field "track_ids", tracks.txt with one line per track, and with --tracks-rescore avg|max result_tracks.txt, the evaluation
of the rescored detections.  --tracks-fill / --tracks-smooth R / --tracks-fill-scale X (only with --tracks) then refine the
tracks (tracks.refine): gap frames filled by interpolation, boxes averaged over +-R frames; predictions_tracks.pth gets the
field "filled", and result_tracks.txt and --tubelet-ap judge the refined list.

--tubelet-ap (with --tubelet-score mean|max) scores tracks against the annotations' <trackid> tracks
(mega.pytorch_amd.track_eval): the tubelet AP at temporal IoU 0.25 / 0.5 / 0.75 -> result_tubelets.txt.  With --tracks it
judges the tracks just linked; without, --predictions must already carry the field "track_ids" (a
predictions_tracks.pth).

--diagnose (with --diagnose-score-thresh X / --diagnose-bg-thresh X) adds the error diagnosis of the raw detections
(mega.pytorch_amd.diagnose): every detection's kind (TP / DUPE / LOC / CLS / BOTH / BKG), every GT box's state and the mAP
each error type costs -> result_diagnosis.txt, with the per-motion-range rows when --motion-iou is given.

--box-only evaluates proposals instead (predictions made with MODEL.RPN_ONLY True, field "objectness"): the recall of the
GT boxes at IoU 0.5 by each frame's first --limit proposals -> proposal_result.txt ("Recall: x", the reference's
do_vid_evaluation(box_only=True)); --recall-table adds the recall at limits 10 / 50 / 100 / 300 and IoU 0.50 .. 0.95 with
its mean (AR) -> proposal_recall_table.txt.

  python tools/eval_vid.py --box-only --predictions OUT/predictions.pth --img-index ImageSets/VID_val_videos.txt \\
      --anno-path Annotations/VID/val [--limit 300] [--recall-table]
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
    ap.add_argument("--motion-iou", default=None, help="vid_groundtruth_motion_iou.mat, or the word 'derive' (the table "
                    "is computed from the annotations' tracks): adds fast / medium / slow AP")
    ap.add_argument("--motion-window", type=int, default=None, help="--motion-iou derive: neighbour frames on each side "
                    "(1 .. 64, default 10)")
    ap.add_argument("--save-motion-iou", default=None, help="--motion-iou derive: also write the derived table to this .mat")
    ap.add_argument("--output-folder", default=None, help="where result.txt goes (default: next to predictions.pth)")
    ap.add_argument("--cache", default=None, help="optional .npz cache of the parsed annotations")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--seq-nms", action="store_true", help="also evaluate the Seq-NMS-rescored predictions")
    ap.add_argument("--seq-nms-link-iou", type=float, default=0.5, help="Seq-NMS: IoU above which boxes of adjacent "
                    "frames link")
    ap.add_argument("--seq-nms-iou", type=float, default=0.3, help="Seq-NMS: IoU above which a path box suppresses")
    ap.add_argument("--seq-nms-rescore", choices=("avg", "max"), default="avg")
    ap.add_argument("--tracks", action="store_true", help="link the detections into tracks (predictions_tracks.pth, "
                    "tracks.txt)")
    ap.add_argument("--tracks-score-thresh", type=float, default=0.05, help="tracks: boxes scoring less take no part")
    ap.add_argument("--tracks-link-iou", type=float, default=0.5, help="tracks: IoU above which a box joins a track")
    ap.add_argument("--tracks-max-gap", type=int, default=1, help="tracks: frames a track may go without a box")
    ap.add_argument("--tracks-min-len", type=int, default=1, help="tracks: shorter tracks get no id")
    ap.add_argument("--tracks-rescore", choices=("none", "avg", "max"), default="none",
                    help="tracks: replace a linked box's score by its track's mean / max -> result_tracks.txt")
    ap.add_argument("--tracks-fill", action="store_true", help="tracks: fill each track's gap frames by interpolation "
                    "(predictions_tracks.pth gets the field \"filled\"; result_tracks.txt judges the refined list)")
    ap.add_argument("--tracks-smooth", type=int, default=None, metavar="R", help="tracks: replace every track box by the "
                    "mean of its track's boxes within R frames (0 .. 64)")
    ap.add_argument("--tracks-fill-scale", type=float, default=None, metavar="X", help="--tracks-fill: a filled box scores "
                    "X times the smaller of its two neighbours' scores (0 < X <= 1, default 1)")
    ap.add_argument("--tubelet-ap", action="store_true", help="tubelet AP of the tracks against the GT tracks "
                    "(result_tubelets.txt)")
    ap.add_argument("--tubelet-score", choices=("mean", "max"), default="mean", help="--tubelet-ap: a tubelet's score")
    ap.add_argument("--diagnose", action="store_true", help="error diagnosis of the detections: error kinds, GT states and "
                    "the mAP each error type costs (result_diagnosis.txt)")
    ap.add_argument("--diagnose-score-thresh", type=float, default=None, metavar="X", help="--diagnose: the count tables "
                    "also cover the detections scoring at least X (default 0.5)")
    ap.add_argument("--diagnose-bg-thresh", type=float, default=None, metavar="X", help="--diagnose: a detection below "
                    "this IoU with every GT box is background (0 < X < 0.5, default 0.1)")
    ap.add_argument("--box-only", action="store_true", help="proposal recall of RPN-only predictions (proposal_result.txt)")
    ap.add_argument("--limit", type=int, default=300, help="--box-only: proposals used per frame (at most 1024)")
    ap.add_argument("--recall-table", action="store_true", help="--box-only: also the recall per limit and IoU threshold")
    a = ap.parse_args(argv)
    if a.box_only and (a.seq_nms or a.motion_iou):
        ap.error("--box-only evaluates proposals: --seq-nms / --motion-iou apply to detections")
    if a.box_only and a.tracks:
        ap.error("--box-only evaluates proposals: --tracks applies to detections")
    if a.box_only and a.tubelet_ap:
        ap.error("--box-only evaluates proposals: --tubelet-ap applies to tracks")
    if a.box_only and a.diagnose:
        ap.error("--box-only evaluates proposals: --diagnose applies to detections")
    if not a.diagnose and (a.diagnose_score_thresh is not None or a.diagnose_bg_thresh is not None):
        ap.error("--diagnose-score-thresh / --diagnose-bg-thresh apply to --diagnose")
    if a.diagnose:
        from mega.pytorch_amd import diagnose
        try:
            diag = diagnose.check_params(diagnose.SCORE_THRESH if a.diagnose_score_thresh is None else a.diagnose_score_thresh,
                                         diagnose.BG_THRESH if a.diagnose_bg_thresh is None else a.diagnose_bg_thresh)
        except ValueError as e:
            ap.error(str(e))
    if not a.tracks and (a.tracks_fill or a.tracks_smooth is not None or a.tracks_fill_scale is not None):
        ap.error("--tracks-fill / --tracks-smooth / --tracks-fill-scale refine linked tracks: they need --tracks")
    if a.tracks:
        from mega.pytorch_amd import tracks
        try:
            refine = tracks.check_refine_params(a.tracks_fill, 0 if a.tracks_smooth is None else a.tracks_smooth,
                                                1.0 if a.tracks_fill_scale is None else a.tracks_fill_scale)
        except ValueError as e:
            ap.error(str(e))
    derive = a.motion_iou == "derive"
    if not derive and (a.motion_window is not None or a.save_motion_iou):
        ap.error("--motion-window / --save-motion-iou apply to --motion-iou derive")
    if derive and a.motion_window is not None and not 1 <= a.motion_window <= 64:
        ap.error("--motion-window must be in 1 .. 64, got %d" % a.motion_window)
    from mega.pytorch_amd import inference, vid_eval
    preds = inference.load_predictions(a.predictions)
    if a.tubelet_ap and not a.tracks and not all(p.has_field("track_ids") for p in preds):
        ap.error("--tubelet-ap without --tracks needs predictions with the field \"track_ids\" (predictions_tracks.pth)")
    if a.tubelet_ap or derive:      # (the same boxes and labels, plus each object's <trackid>; its cache holds the ids too)
        gt = vid_eval.VIDTrackGroundTruth(a.img_index, a.anno_path, cache=a.cache)
    else:
        gt = vid_eval.VIDGroundTruth(a.img_index, a.anno_path, cache=a.cache)
    if derive:
        from mega.pytorch_amd import motion_iou
        motion = motion_iou.derive(gt, inference.VIDTestIndex(a.img_index).videos,
                                   motion_iou.WINDOW if a.motion_window is None else a.motion_window, device=a.device)
        if a.save_motion_iou:
            motion_iou.save_mat(a.save_motion_iou, motion, off=gt.off)
    else:
        motion = vid_eval.load_motion_iou(a.motion_iou) if a.motion_iou else None
    out = a.output_folder or os.path.dirname(os.path.abspath(a.predictions))
    if a.box_only:
        res = vid_eval.evaluate_proposals(preds, gt, limit=a.limit, output_folder=out, device=a.device,
                                          limits=vid_eval.PROPOSAL_LIMITS if a.recall_table else None)
        sys.stdout.write("Recall: {:.4f}\n".format(res["recall"]))
        if a.recall_table:
            sys.stdout.write(vid_eval.format_recall_table(res["limits"], res["iou_thresholds"], res["table"], res["ar"],
                                                          res["num_pos"]))
        return 0
    res = vid_eval.evaluate_detections(preds, gt, motion_iou=motion, output_folder=out, device=a.device)
    sys.stdout.write(vid_eval.format_result(res))
    if a.diagnose:
        res = diagnose.evaluate_errors(preds, gt, motion_iou=motion, score_thresh=diag[0], bg_thresh=diag[1],
                                       output_folder=out, device=a.device)
        sys.stdout.write("Diagnosis:\n" + res["text"])
    if a.seq_nms:
        from mega.pytorch_amd import seq_nms
        videos = [(v["start"], v["seg_len"]) for v in inference.VIDTestIndex(a.img_index).videos]
        rescored = seq_nms.seq_nms(preds, videos, link_iou=a.seq_nms_link_iou, nms_iou=a.seq_nms_iou,
                                   rescore=a.seq_nms_rescore, device=a.device)
        os.makedirs(out, exist_ok=True)
        inference.save_predictions(rescored, os.path.join(out, "predictions_seq_nms.pth"))
        res = vid_eval.evaluate_detections(rescored, gt, motion_iou=motion, output_folder=out, device=a.device,
                                           result_name="result_seq_nms.txt")
        sys.stdout.write("Seq-NMS:\n" + vid_eval.format_result(res))
        preds = rescored
    if a.tracks:
        from mega.pytorch_amd import tracks
        videos = [(v["start"], v["seg_len"]) for v in inference.VIDTestIndex(a.img_index).videos]
        rescore = None if a.tracks_rescore == "none" else a.tracks_rescore
        tracked, table = tracks.link(preds, videos, score_thresh=a.tracks_score_thresh, link_iou=a.tracks_link_iou,
                                     max_gap=a.tracks_max_gap, min_len=a.tracks_min_len, rescore=rescore, device=a.device)
        refined = refine[0] or refine[1] > 0
        if refined:
            tracked, info = tracks.refine(tracked, videos, fill=refine[0], smooth=refine[1], fill_scale=refine[2],
                                          device=a.device)
        os.makedirs(out, exist_ok=True)
        inference.save_predictions(tracked, os.path.join(out, "predictions_tracks.pth"))
        with open(os.path.join(out, "tracks.txt"), "w") as f:
            f.write(tracks.format_table(table))
        sys.stdout.write("Tracks: %d\n" % len(table))
        if refined:
            sys.stdout.write("Filled boxes: %d\n" % info["filled"])
        if rescore is not None or refined:
            res = vid_eval.evaluate_detections(tracked, gt, motion_iou=motion, output_folder=out, device=a.device,
                                               result_name="result_tracks.txt")
            sys.stdout.write("Tracks, %s:\n" % " and ".join(w for w, on in (("rescored", rescore is not None),
                                                                             ("refined", refined)) if on)
                             + vid_eval.format_result(res))
        preds = tracked
    if a.tubelet_ap:
        from mega.pytorch_amd import track_eval
        videos = [(v["start"], v["seg_len"]) for v in inference.VIDTestIndex(a.img_index).videos]
        res = track_eval.evaluate_tracks(preds, gt, videos, tubelet_score=a.tubelet_score, output_folder=out,
                                         device=a.device)
        sys.stdout.write("Tubelets:\n" + res["text"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
