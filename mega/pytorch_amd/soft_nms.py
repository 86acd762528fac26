"""Soft-NMS (TEST.SOFT_NMS) and box voting (TEST.BBOX_VOTE): the final filter of the detections, for every detector.

Neither is in the reference (it has no Seq-NMS either), so this docstring is the specification.  ops.soft_merge
(csrc/soft_nms.hip) and the numpy twin tests/soft_nms_twin.py both implement it.

Soft-NMS (Bodla et al. 2017) decays the scores of boxes that overlap a kept box instead of deleting them; box voting
replaces every kept box by the score-weighted mean of the candidates that overlap it.  Both run on the candidates of the
box head (PostProcessor.candidates), so they sit in the merge slot of TEST.BBOX_AUG: with box augmentation its views feed
this filter, without it the video runs as the identity view alone (one pass, bbox_aug.detect_video).

Input rows.  What ops.bbox_aug_merge takes: candidates [K][F][NC-1][R], score -1 for dead rows.  Rows are mapped into
view 0's image exactly as csrc/bbox_aug.hip does (flip: x' = (W_k - x_max) - 1, two f32 ops; resize: one f32 multiply by
the f32 ratio).  Per (frame, class) the K*R rows are taken in (view, row) order.  A row is LIVE when its score is
> SCORE_THRESH.  IoU is the package's +1-area f32 IoU in nms.cu's devIoU order of operations:
    inter = max(min(x2) - max(x1) + 1, 0) * max(min(y2) - max(y1) + 1, 0);  iou = inter / (Sa + Sb - inter).
A NaN IoU neither decays nor votes.  Everything is f32 except where stated.

1. Soft-NMS (SOFT_NMS.ENABLED; otherwise the greedy NMS with ROI_HEADS.NMS and NMS_STRICT_GT, as without this filter).
   A = the live rows, s = their scores.  While A is non-empty: m = the row of A with the largest s (equal s: the smallest
   row index); m moves to KEPT with its current s; for every j still in A, o = iou(m, j) and s_j = s_j * w with
       linear    w = 1 - o if o exceeds ROI_HEADS.NMS (o > NMS, or o >= NMS when NMS_STRICT_GT is False), else w = 1
       gaussian  w = expf(-(o * o) / SIGMA), for every j
   and a row leaves A unkept as soon as its score is no longer > SCORE_THRESH.  Every pass removes at least m, so the
   loop runs at most as often as there are rows.

2. Box voting (BBOX_VOTE.ENABLED).  For every kept row k the voters are all live rows j of the same (frame, class) with
   iou(k, j) >= VOTE_TH -- with their ORIGINAL candidate boxes and scores, not decayed or voted ones; k always votes for
   itself.  The new box is sum(s_j * b_j) / sum(s_j) per coordinate, products and sums in f64, rounded once to f32.
   Score, SCORING_METHOD "ID": unchanged (the soft-NMS score if step 1 ran); "AVG": the f32 of the f64 mean of the
   voters' original scores.  Voted boxes go to a buffer of their own: no vote sees another's result.

3. Finalize.  The post-processor's class-major, row-ascending compaction and the DETECTIONS_PER_IMG k-th value cut
   (>= the k-th score, ties kept) on the final scores.

With both options off the result is ops.bbox_aug_merge's, bit for bit.  No accuracy claim is made: VID mAP with these
options has not been measured.
"""
from .config import FinalFilter, final_filter      # noqa: F401  (TEST.SOFT_NMS / TEST.BBOX_VOTE -> the merge's settings)


def enabled_filter(cfg):
    """The cfg's FinalFilter if either option is on, else None (values are validated either way)."""
    ff = final_filter(cfg)
    return ff if ff.enabled else None
