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


def _parser():
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
    return ap


# how this tool words postrun.ProposalOnly, by the option it names
APPLIES = {"seq_nms": "--seq-nms / --motion-iou apply to detections", "tracks": "--tracks applies to detections",
           "tubelet_ap": "--tubelet-ap applies to tracks", "diagnose": "--diagnose applies to detections"}


def build_plan(argv=None):
    """The command line -> (the parsed arguments, their postrun.Plan); an argument error exits with status 2."""
    ap = _parser()
    a = ap.parse_args(argv)
    derive = a.motion_iou == "derive"
    if a.box_only and a.motion_iou:
        ap.error("--box-only evaluates proposals: " + APPLIES["seq_nms"])
    if not a.diagnose and (a.diagnose_score_thresh is not None or a.diagnose_bg_thresh is not None):
        ap.error("--diagnose-score-thresh / --diagnose-bg-thresh apply to --diagnose")
    if not a.tracks and (a.tracks_fill or a.tracks_smooth is not None or a.tracks_fill_scale is not None):
        ap.error("--tracks-fill / --tracks-smooth / --tracks-fill-scale refine linked tracks: they need --tracks")
    if not derive and (a.motion_window is not None or a.save_motion_iou):
        ap.error("--motion-window / --save-motion-iou apply to --motion-iou derive")
    if derive and a.motion_window is not None and not 1 <= a.motion_window <= 64:
        ap.error("--motion-window must be in 1 .. 64, got %d" % a.motion_window)

    def given(**kw):
        return {k: v for k, v in kw.items() if v is not None}
    options = {
        "seq_nms": a.seq_nms and {"link_iou": a.seq_nms_link_iou, "nms_iou": a.seq_nms_iou, "rescore": a.seq_nms_rescore},
        "tracks": a.tracks and given(score_thresh=a.tracks_score_thresh, link_iou=a.tracks_link_iou,
                                     max_gap=a.tracks_max_gap, min_len=a.tracks_min_len, fill=a.tracks_fill,
                                     rescore=None if a.tracks_rescore == "none" else a.tracks_rescore,
                                     smooth=a.tracks_smooth, fill_scale=a.tracks_fill_scale),
        "tubelet_score": a.tubelet_score if a.tubelet_ap else None,
        "diagnose": a.diagnose and given(score_thresh=a.diagnose_score_thresh, bg_thresh=a.diagnose_bg_thresh),
        "motion_iou": given(derive=True, window=a.motion_window) if derive else a.motion_iou}
    from mega.pytorch_amd import postrun
    try:
        plan = postrun.plan(box_only=a.box_only, limit=a.limit, recall_table=a.recall_table, cache=a.cache,
                            save_motion_iou=a.save_motion_iou, anno_path=a.anno_path, **options)
    except postrun.ProposalOnly as e:
        ap.error("--box-only evaluates proposals: " + APPLIES[e.option])
    except ValueError as e:
        ap.error(str(e))
    return a, plan


def main(argv=None):
    a, plan = build_plan(argv)
    from mega.pytorch_amd import inference, postrun, vid_eval
    preds = inference.load_predictions(a.predictions)
    if plan.tubelet_score is not None and plan.tracks is None and not all(p.has_field("track_ids") for p in preds):
        _parser().error("--tubelet-ap without --tracks needs predictions with the field \"track_ids\" "
                        "(predictions_tracks.pth)")

    def report(title, res):
        if title == "Recall":
            sys.stdout.write("Recall: {:.4f}\n".format(res["recall"]))
            if plan.recall_table:
                sys.stdout.write(vid_eval.format_recall_table(res["limits"], res["iou_thresholds"], res["table"], res["ar"],
                                                              res["num_pos"]))
        elif title == "Tracks":
            sys.stdout.write("Tracks: %d\n" % len(res["table"]))
            if res["refine_info"] is not None:
                sys.stdout.write("Filled boxes: %d\n" % res["refine_info"]["filled"])
        else:
            text = res["text"] if "text" in res else vid_eval.format_result(res)
            sys.stdout.write((title + ":\n" if title else "") + text)
    out = a.output_folder or os.path.dirname(os.path.abspath(a.predictions))
    postrun.run(plan, preds, a.img_index, a.anno_path, out, a.device, report=report)
    return 0


if __name__ == "__main__":
    sys.exit(main())
