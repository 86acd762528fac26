"""Test-time box augmentation (TEST.BBOX_AUG): mega_core/engine/bbox_aug.py for every detector of the package.

Views (bbox_aug.py:26-51, in this order): the identity at INPUT.MIN_SIZE_TEST / MAX_SIZE_TEST; its horizontal flip if
H_FLIP; for every s in SCALES the size s at TEST.BBOX_AUG.MAX_SIZE, then its flip if SCALE_H_FLIP.  A view's frame size
is feed.get_size of the video's frame size; a flip mirrors the RESIZED uint8 frame (TT.RandomHorizontalFlip after
T.Resize).

One pass per view: every view is an independent pass of the whole video through the unchanged detector, the view's
transform applied to every frame it reads (key, local, global and memory frames for MEGA / RDN, the window for FGFA, key
and non-key frames for DFF), with the same global-frame schedule.  The box head runs in candidate mode
(PostProcessor.candidates): each frame yields its (NC-1) x R candidates, decoded and clipped in the view's own image.

Merge (ops.bbox_aug_merge, csrc/bbox_aug.hip), per frame: flipped views' boxes are un-flipped (BoxList.transpose), views
after the first are scaled into the identity view's image (BoxList.resize), then filter_results runs on the (view,
proposal row) concatenation.  The result is a BoxList in the identity view's coordinates with "scores" / "labels", what
predictions.pth holds without augmentation.  With the identity view alone the result is bit-identical to running
without TEST.BBOX_AUG.
"""
import contextlib
from collections import namedtuple

import torch

from . import feed, ops
from .structures import BoxList

View = namedtuple("View", "min_size max_size hflip size")      # size = (w, h) of the view's frames


def views_from_cfg(cfg, in_wh):
    """The views of a video whose frames are in_wh = (w, h), in the reference's order (bbox_aug.py:26-51)."""
    aug = cfg.TEST.BBOX_AUG

    def view(min_size, max_size, hflip):
        h, w = feed.get_size(tuple(in_wh), min_size, max_size)
        return View(int(min_size), int(max_size), bool(hflip), (int(w), int(h)))
    views = [view(cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, False)]
    if aug.H_FLIP:
        views.append(view(cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, True))
    for s in aug.SCALES:
        views.append(view(s, aug.MAX_SIZE, False))
        if aug.SCALE_H_FLIP:
            views.append(view(s, aug.MAX_SIZE, True))
    if len(views) > ops.BBOX_AUG_MAX_VIEWS:
        raise ValueError("TEST.BBOX_AUG: %d views; the merge takes at most %d" % (len(views), ops.BBOX_AUG_MAX_VIEWS))
    return views


def identity_view(cfg, in_wh):
    """The view a video has without TEST.BBOX_AUG: INPUT.MIN_SIZE_TEST / MAX_SIZE_TEST, not flipped."""
    h, w = feed.get_size(tuple(in_wh), cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)
    return View(int(cfg.INPUT.MIN_SIZE_TEST), int(cfg.INPUT.MAX_SIZE_TEST), False, (int(w), int(h)))


@contextlib.contextmanager
def candidate_mode(model, on=True):
    """The model's box head emits candidates (PostProcessor.candidates) inside the block."""
    pp = model.roi_heads.box.post_processor
    old = pp.candidates
    pp.candidates = bool(on)
    try:
        yield pp
    finally:
        pp.candidates = old


def stack_candidates(dets, num_classes):
    """A view's per-frame candidate BoxLists ((NC-1)*R_f rows each, class-major) -> (boxes [T,NC-1,R,4],
    scores [T,NC-1,R]) with R = max R_f; the rows past a frame's own R_f hold score -1 (dropped by the merge, so the
    (view, row) order of the live rows is kept)."""
    C1 = num_classes - 1
    rs = [len(d) // C1 for d in dets]
    for d, r in zip(dets, rs):
        if r * C1 != len(d):
            raise ValueError("a candidate BoxList has %d rows, not a multiple of NC-1 = %d" % (len(d), C1))
    R = max(rs) if rs else 0
    if rs and min(rs) == R:
        return (torch.stack([d.bbox.view(C1, R, 4) for d in dets]),
                torch.stack([d.get_field("scores").view(C1, R) for d in dets]))
    dev = dets[0].bbox.device
    cb = torch.zeros((len(dets), C1, R, 4), dtype=torch.float32, device=dev)
    cs = torch.full((len(dets), C1, R), -1.0, dtype=torch.float32, device=dev)
    for t, (d, r) in enumerate(zip(dets, rs)):
        cb[t, :, :r] = d.bbox.view(C1, r, 4)
        cs[t, :, :r] = d.get_field("scores").view(C1, r)
    return cb, cs


def merge(per_view, views, post_processor, chunk=16, final=None):
    """per_view[k] = (boxes [T,NC-1,R_k,4], scores [T,NC-1,R_k]) of view k (stack_candidates) -> list of T BoxLists
    in view 0's image.  The merge runs `chunk` frames at a time, so its workspace does not grow with the video.
    final: a config.FinalFilter (TEST.SOFT_NMS / TEST.BBOX_VOTE); when one of its options is on the final filter is
    ops.soft_merge with its settings instead of ops.bbox_aug_merge."""
    pp = post_processor
    K = len(per_view)
    T = per_view[0][1].shape[0]
    R = max(s.shape[2] for _, s in per_view)
    out = []
    sizes, flips = [v.size for v in views], [v.hflip for v in views]
    for f0 in range(0, T, chunk):
        f1 = min(T, f0 + chunk)
        if K == 1 and per_view[0][1].shape[2] == R:
            cb = per_view[0][0][f0:f1].unsqueeze(0).contiguous()
            cs = per_view[0][1][f0:f1].unsqueeze(0).contiguous()
        else:
            F, C1 = f1 - f0, per_view[0][1].shape[1]
            dev = per_view[0][1].device
            cb = torch.zeros((K, F, C1, R, 4), dtype=torch.float32, device=dev)
            cs = torch.full((K, F, C1, R), -1.0, dtype=torch.float32, device=dev)
            for k, (b, s) in enumerate(per_view):
                cb[k, :, :, :b.shape[2]] = b[f0:f1]
                cs[k, :, :, :s.shape[2]] = s[f0:f1]
        if final is not None and final.enabled:
            ob, os_, ol, oc = ops.soft_merge(cb, cs, sizes, flips, pp.score_thresh, pp.nms, pp.detections_per_img,
                                             pp.strict_gt, **final.kwargs())
        else:
            ob, os_, ol, oc = ops.bbox_aug_merge(cb, cs, sizes, flips, pp.score_thresh, pp.nms, pp.detections_per_img,
                                                 pp.strict_gt)
        for f, n in enumerate(oc.tolist()):
            # copies of the live rows: a view would keep the chunk's whole (NC-1)*K*R-row output buffers alive
            res = BoxList(ob[f, :n].clone(), sizes[0], "xyxy")
            res.add_field("scores", os_[f, :n].clone())
            res.add_field("labels", ol[f, :n].clone())
            out.append(res)
    return out


def detect_video(model, views, run_view, chunk=16, final=None):
    """The views of one video through run_view(view) -> that pass's per-frame outputs (list of BoxLists, candidate mode on
    for the call), then the merge -> list of BoxLists (one per frame, in view 0's image).  final: merge()'s."""
    nc = model.cfg.MODEL.ROI_BOX_HEAD.NUM_CLASSES
    per_view = []
    with candidate_mode(model) as pp:
        for v in views:
            dets = run_view(v)
            per_view.append(stack_candidates(dets, nc))
            del dets
    if final is not None and final.enabled:
        return merge(per_view, views, pp, chunk=chunk, final=final)
    return merge(per_view, views, pp, chunk=chunk)


def run_video(model, run, v, src, make_source, aug_cfg=None, final=None, chunk=16):
    """One video through its views and the merge, for the test loop and the demo.  run(source, v) is the engine's pass
    over one feed; src the identity view's feed.FrameSource, make_source(min_size, max_size, hflip) the feed of another
    view (closed here).  aug_cfg: the config whose TEST.BBOX_AUG views are used, or None: the identity view alone (what
    TEST.SOFT_NMS / TEST.BBOX_VOTE need without box augmentation: candidate mode, one pass)."""
    in_wh = (src.in_hw[1], src.in_hw[0])
    views = views_from_cfg(aug_cfg, in_wh) if aug_cfg is not None else [identity_view(model.cfg, in_wh)]

    def run_view(view):
        if view == views[0]:
            return run(src, v)
        s = make_source(view.min_size, view.max_size, view.hflip)
        try:
            return run(s, v)
        finally:
            s.close()
    return detect_video(model, views, run_view, chunk=chunk, final=final)
