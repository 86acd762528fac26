"""What happens once the detections exist, for inference.inference() and tools/eval_vid.py alike: the VID evaluation of
the raw list, the error diagnosis, Seq-NMS, track linking and refinement with their evaluations, the tubelet AP; for
proposals (MODEL.RPN_ONLY / --box-only) the recall alone.  The two front ends keep their own vocabulary and documentation
(inference()'s docstring, the tool's); the decisions are made here, once:

  plan(...)   the options, decoded and checked -> a Plan.  No file, no device: a bad value raises before the run.
  run(...)    the chain of a Plan on a list of predictions, in the one order its docstring gives.

A stage is called through its module (seq_nms.seq_nms, tracks.link, ...), so what a file holds is that module's call on
the stage's input; no stage is implemented here.
"""
import collections
import inspect
import logging
import os

from . import diagnose as dg, inference as inf, motion_iou as mi, seq_nms as sn, track_eval, tracks as tr, vid_eval

# the options that work on detections, in the order they are refused for proposals, as inference() words them
DETECTION_OPTIONS = (("seq_nms", "Seq-NMS rescoring (seq_nms=...)"), ("tracks", "track linking (tracks=...)"),
                     ("tubelet_ap", "the tubelet AP (tubelet_ap)"), ("diagnose", "the error diagnosis (diagnose=...)"))


class ProposalOnly(ValueError):
    """An option of DETECTION_OPTIONS was asked for together with box_only; `option` is its name, for a front end that
    words the refusal itself."""

    def __init__(self, option):
        ValueError.__init__(self, "MODEL.RPN_ONLY returns proposals: %s needs detections" % dict(DETECTION_OPTIONS)[option])
        self.option = option


class Plan(collections.namedtuple("Plan", "box_only limit recall_table motion_iou window save_motion_iou cache diagnose "
                                          "seq_nms tracks refine tubelet_score")):
    """plan()'s result, immutable.  A stage that is off is None; one that is on holds its module's keywords, every default
    filled in, as a tuple of (name, value) pairs in name order (dict(...) gives the keywords back).
      box_only, limit, recall_table   proposals: vid_eval.evaluate_proposals' limit, and whether its table is wanted
      motion_iou                      a path or vid_eval.load_motion_iou's lists, or
      window, save_motion_iou         an int: the table is derived from the annotations' tracks; the .mat it is also written to
      cache                           the ground truth's .npz cache
      diagnose, seq_nms, tracks       diagnose.evaluate_errors', seq_nms.seq_nms' and tracks.link's keywords
      refine                          tracks.refine's keywords, when fill or smooth is on
      tubelet_score                   "mean" | "max": the tubelet AP is on"""
    __slots__ = ()


def _on(option):
    return option is not None and option is not False


def _keywords(checker, option, **defaults):
    """An option's None | False | True | dict form -> None when it is off, else `checker`'s keywords (its own defaults,
    then `defaults`, then the dict), checked by it, as Plan holds them."""
    if not _on(option):
        return None
    params = {k: p.default for k, p in inspect.signature(checker).parameters.items()}
    params.update(defaults)
    params.update({} if option is True else option)
    checker(**params)
    return tuple(sorted(params.items()))


def plan(seq_nms=None, tracks=None, diagnose=None, motion_iou=None, box_only=False, limit=300, recall_table=False,
         save_motion_iou=None, cache=None, anno_path=None, tubelet_score=None):
    """inference()'s options (its docstring describes them) plus the evaluation tool's -> Plan; ValueError for a bad
    value, ProposalOnly for an option that needs detections next to box_only.  tubelet_score asks for the tubelet AP of
    predictions that carry "track_ids" already; the tracks dict's "tubelet_ap" / "tubelet_score" ask for that of the
    tracks it links."""
    refine = None
    if _on(tracks):
        tracks = {} if tracks is True else dict(tracks)
        asked, score = tracks.pop("tubelet_ap", False), tracks.pop("tubelet_score", "mean")
        tubelet_score = score if asked else tubelet_score
        refine = {k: tracks.pop(k) for k in ("fill", "smooth", "fill_scale") if k in tracks}
    asked = {"seq_nms": _on(seq_nms), "tracks": _on(tracks), "tubelet_ap": tubelet_score is not None,
             "diagnose": _on(diagnose)}
    for option, _ in DETECTION_OPTIONS:
        if box_only and asked[option]:
            raise ProposalOnly(option)
    diagnose, seq_nms = _keywords(dg.check_params, diagnose), _keywords(sn.check_params, seq_nms)
    if tubelet_score is not None:
        track_eval.check_params(tubelet_score=tubelet_score)
    refine = _keywords(tr.check_refine_params, refine, fill=False)
    if refine is not None and not (dict(refine)["fill"] or dict(refine)["smooth"] > 0):
        refine = None
    tracks = _keywords(tr.check_params, tracks)
    window = mi.check_request(motion_iou, anno_path)
    return Plan(bool(box_only), limit, bool(recall_table), motion_iou if window is None else None, window, save_motion_iou,
                cache, diagnose, seq_nms, tracks, refine, tubelet_score)


def _save(predictions, output_folder, name):
    if output_folder:
        os.makedirs(output_folder, exist_ok=True)
        inf.save_predictions(predictions, os.path.join(output_folder, name))


def run(plan, predictions, img_index, anno_path, output_folder, device, logger=None, report=None):
    """The chain of `plan` on `predictions` (list[BoxList] over the frames of the index file img_index), in this order:
      1. the ground truth, with anno_path only, parsed once: vid_eval.VIDTrackGroundTruth when the motion IoU table is
         derived from it or the tubelet AP is on, else VIDGroundTruth; the motion IoU table, derived or loaded;
      2. box_only: vid_eval.evaluate_proposals, and nothing else;
      3. vid_eval.evaluate_detections of `predictions` -> result.txt;
      4. diagnose.evaluate_errors of `predictions` -> result_diagnosis.txt;
      5. seq_nms.seq_nms -> predictions_seq_nms.pth, its evaluation -> result_seq_nms.txt;
      6. tracks.link of what Seq-NMS kept (of `predictions` without it), then tracks.refine -> predictions_tracks.pth,
         tracks.txt (the linker's table); the list's evaluation -> result_tracks.txt when it was rescored or refined;
      7. track_eval.evaluate_tracks of the latest list (which must carry "track_ids") -> result_tubelets.txt.
    Without anno_path nothing is evaluated; 5 and 6 still make and write their lists.  Files go to output_folder (none
    without one); logger goes to every evaluation (default: each module's own) and gets the track counts.
    report(title, result), if given, is called after every step that has something to show: "Recall", "" (the raw
    evaluation), "Diagnosis", "Seq-NMS", "Tracks" (with this function's return value so far), "Tracks, rescored and
    refined" or what applies of it, "Tubelets" -- otherwise with the evaluation's result.
    -> {"rescored": Seq-NMS's list, "tracked": the linked and refined list, "table": the track table, "refine_info":
    tracks.refine's counts}, each None where the stage did not run."""
    report = report or (lambda title, result: None)
    videos = [(v["start"], v["seg_len"]) for v in inf.VIDTestIndex(img_index).videos]
    out = {"rescored": None, "tracked": None, "table": None, "refine_info": None}
    to = {"output_folder": output_folder, "device": device, "logger": logger}
    gt = motion = None
    if anno_path is not None:
        with_tracks = plan.window is not None or plan.tubelet_score is not None
        gt = (vid_eval.VIDTrackGroundTruth if with_tracks else vid_eval.VIDGroundTruth)(img_index, anno_path, cache=plan.cache)
        if plan.window is not None:
            motion = mi.derive(gt, videos, plan.window, device=device)
            if plan.save_motion_iou:
                mi.save_mat(plan.save_motion_iou, motion, off=gt.off)
        else:
            motion = vid_eval.load_motion_iou(plan.motion_iou) if isinstance(plan.motion_iou, str) else plan.motion_iou

    def evaluate(title, preds, **kw):
        if gt is not None:
            report(title, vid_eval.evaluate_detections(preds, gt, motion_iou=motion, **to, **kw))

    if plan.box_only:
        if gt is not None:
            report("Recall", vid_eval.evaluate_proposals(predictions, gt, limit=plan.limit, **to,
                                                         limits=vid_eval.PROPOSAL_LIMITS if plan.recall_table else None))
        return out
    evaluate("", predictions)
    if gt is not None and plan.diagnose is not None:
        report("Diagnosis", dg.evaluate_errors(predictions, gt, motion_iou=motion, **dict(plan.diagnose), **to))
    if plan.seq_nms is not None:
        predictions = out["rescored"] = sn.seq_nms(predictions, videos, device=device, **dict(plan.seq_nms))
        _save(predictions, output_folder, "predictions_seq_nms.pth")
        evaluate("Seq-NMS", predictions, result_name="result_seq_nms.txt")
    if plan.tracks is not None:
        predictions, out["table"] = tr.link(predictions, videos, device=device, **dict(plan.tracks))
        how = ["rescored"] if dict(plan.tracks)["rescore"] is not None else []
        if plan.refine is not None:                              # after the linking and its rescoring
            predictions, out["refine_info"] = tr.refine(predictions, videos, device=device, **dict(plan.refine))
            how.append("refined")
        out["tracked"] = predictions
        log = logger or logging.getLogger("mega.pytorch_amd.postrun")
        if out["refine_info"] is not None:
            log.info("Refined %d tracks: %d boxes filled", out["refine_info"]["tracks"], out["refine_info"]["filled"])
        log.info("Linked %d tracks", len(out["table"]))
        _save(predictions, output_folder, "predictions_tracks.pth")
        if output_folder:
            with open(os.path.join(output_folder, "tracks.txt"), "w") as f:
                f.write(tr.format_table(out["table"]))
        report("Tracks", out)
        if how:
            evaluate("Tracks, " + " and ".join(how), predictions, result_name="result_tracks.txt")
    if gt is not None and plan.tubelet_score is not None:
        report("Tubelets", track_eval.evaluate_tracks(predictions, gt, videos, tubelet_score=plan.tubelet_score, **to))
    return out
