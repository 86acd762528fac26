"""ImageNet VID evaluation: AP50 and motion-specific AP ("fast" / "medium" / "slow") of a list[BoxList], the step the
reference's inference() ends with (mega_core/engine/inference.py:129-132, inference_no_model :135-160).

Mirror of  mega_core/data/datasets/vid.py:22-40, :139-192        class lists, _preprocess_annotation, annotation cache
           mega_core/data/datasets/evaluation/vid/vid_eval.py      do_vid_evaluation / eval_detection_vid /
                                                                   calc_detection_vid_prec_rec / calc_detection_vid_ap

What changes: the per-frame / per-class / per-detection Python loops run as two HIP kernels (csrc/vid_eval.hip): one wave
per (frame, motion range) matches detections to GT boxes, one workgroup per (class, motion range) scans precision /
recall and reduces AP.  The predictions are packed into flat arrays on the host and copied to the device once.

What is defined here where the reference leaves it to the platform:
  - ORDER ON TIES.  The reference sorts with numpy's argsort()[::-1], whose order of equal scores depends on numpy's sort
    implementation.  Here equal scores are ordered by DESCENDING position: within a frame, the position in the
    prediction list; per class over the dataset, the position in the frame-by-frame concatenation (of the frames' already
    ordered detections).  This is a stable ascending argsort reversed -- what numpy gives for runs of 16 or fewer.
  - Motion IoUs are read into per-frame lists (load_motion_iou); the reference's np.array over those ragged lists
    (vid_eval.py:133-137) fails on numpy >= 1.24.
  - empty_weight (the pred_ignore of a detection whose class has no GT box in its frame) is, as in the reference, the
    fraction of ALL entries of the motion file inside the range, even when fewer frames are evaluated.
  - PROPOSAL ORDER ON TIES (evaluate_proposals).  The reference orders a frame's proposals with torch's
    sort(descending=True), which is not stable.  Here they are ordered by descending objectness and equal values keep
    their ASCENDING position in the prediction list (a stable descending sort); the RPN's keep order is already that.
    In the greedy matching, equal IoUs go to the lower GT index, then to the lower proposal position: what torch's CPU
    max(dim) -- the first maximum -- gives the reference.
Proposal recall (do_vid_evaluation(box_only=True), eval_proposals_vid, vid_eval.py:26-37 / :72-119) is
evaluate_proposals(): a third HIP kernel (csrc/proposal_recall.hip), one wave per (frame, proposal limit).
Not provided (a clear error): the VOC07 11-point metric; evaluate_detections(box_only=True) points to evaluate_proposals.
There is no CPU path: the matching and the AP reduction run on a HIP device.
"""
import logging
import os
import warnings
import xml.etree.ElementTree as ET

import numpy as np
import torch

from . import flat
from .structures import BoxList

CLASSES = ['__background__',  # always index 0
           'airplane', 'antelope', 'bear', 'bicycle',
           'bird', 'bus', 'car', 'cattle',
           'dog', 'domestic_cat', 'elephant', 'fox',
           'giant_panda', 'hamster', 'horse', 'lion',
           'lizard', 'monkey', 'motorcycle', 'rabbit',
           'red_panda', 'sheep', 'snake', 'squirrel',
           'tiger', 'train', 'turtle', 'watercraft',
           'whale', 'zebra']
CLASSES_MAP = ['__background__',  # always index 0
               'n02691156', 'n02419796', 'n02131653', 'n02834778',
               'n01503061', 'n02924116', 'n02958343', 'n02402425',
               'n02084071', 'n02121808', 'n02503517', 'n02118333',
               'n02510455', 'n02342885', 'n02374451', 'n02129165',
               'n01674464', 'n02484322', 'n03790512', 'n02324045',
               'n02509815', 'n02411705', 'n01726692', 'n02355227',
               'n02129604', 'n04468005', 'n01662784', 'n04530566',
               'n02062744', 'n02391049']
CLASSES_TO_IND = dict(zip(CLASSES_MAP, range(len(CLASSES_MAP))))

# vid_eval.py:39-44
MOTION_RANGES = [[0.0, 1.0], [0.0, 0.7], [0.7, 0.9], [0.9, 1.0]]
MOTION_NAMES = ["all", "fast", "medium", "slow"]
MAX_GT_PER_FRAME = 4096     # the matching kernel keeps 64 selected flags per lane
MAX_PROPOSAL_LIMIT = 1024   # the proposal kernel keeps 16 proposals per lane
PROPOSAL_LIMITS = (10, 50, 100, 300)
PROPOSAL_IOU_THRESHOLDS = tuple(round(0.5 + 0.05 * i, 2) for i in range(10))


def parse_annotation(root, classes_to_ind=CLASSES_TO_IND):
    """vid.py:139-166 (_preprocess_annotation) on a parsed XML root -> {"boxes": [n,4] f32, "labels": [n] i64,
    "im_info": (height, width)}.  An object is kept when its raw name is a known wnid; its box is clipped to the frame."""
    size = root.find("size")
    im_info = tuple(map(int, (size.find("height").text, size.find("width").text)))
    boxes, labels = [], []
    for obj in root.findall("object"):
        if obj.find("name").text not in classes_to_ind:
            continue
        bb = obj.find("bndbox")
        boxes.append([max(float(bb.find("xmin").text), 0.0), max(float(bb.find("ymin").text), 0.0),
                      min(float(bb.find("xmax").text), im_info[1] - 1), min(float(bb.find("ymax").text), im_info[0] - 1)])
        labels.append(classes_to_ind[obj.find("name").text.lower().strip()])
    return {"boxes": np.asarray(boxes, dtype=np.float32).reshape(-1, 4), "labels": np.asarray(labels, dtype=np.int64),
            "im_info": im_info}


class VIDGroundTruth(object):
    """The GT boxes of every frame of a VID index file (inference.VIDTestIndex), flat: boxes [G,4] f32, labels [G] i64,
    off [F+1] (frame i's boxes are off[i] .. off[i+1]), height / width [F] (the annotation's frame size).

    cache: an optional .npz path.  When it exists and lists the same frames it is read instead of the XML files; else it
    is written after parsing (what the reference's <image_set>_anno.pkl is for, vid.py:168-192)."""

    classes = CLASSES

    def __init__(self, img_index, anno_path, cache=None):
        from .inference import VIDTestIndex
        self.image_set_index = list(VIDTestIndex(img_index).image_set_index)
        if cache and os.path.exists(cache):
            z = np.load(cache, allow_pickle=False)
            if list(z["image_set_index"]) == self.image_set_index:
                self._set(z["boxes"], z["labels"], z["off"], z["height"], z["width"])
                return
            logging.getLogger("mega.pytorch_amd.vid_eval").warning("%s lists other frames: re-reading the XML files", cache)
        annos = [parse_annotation(ET.parse(os.path.join(anno_path, name + ".xml")).getroot())
                 for name in self.image_set_index]
        self._set_annos(annos)
        if cache:
            d = os.path.dirname(os.path.abspath(cache))
            os.makedirs(d, exist_ok=True)
            np.savez(cache, image_set_index=np.asarray(self.image_set_index), boxes=self.boxes, labels=self.labels,
                     off=self.off, height=self.height, width=self.width)

    @classmethod
    def from_annotations(cls, annos):
        """From a list of parse_annotation() dicts (one per frame)."""
        self = cls.__new__(cls)
        self.image_set_index = None
        self._set_annos(annos)
        return self

    def _set_annos(self, annos):
        n = [len(a["labels"]) for a in annos]
        off = np.zeros(len(annos) + 1, dtype=np.int64)
        off[1:] = np.cumsum(n)
        boxes = np.concatenate([np.asarray(a["boxes"], np.float32).reshape(-1, 4) for a in annos]) if annos else \
            np.zeros((0, 4), np.float32)
        labels = np.concatenate([np.asarray(a["labels"], np.int64).reshape(-1) for a in annos]) if annos else \
            np.zeros((0,), np.int64)
        self._set(boxes, labels, off, [a["im_info"][0] for a in annos], [a["im_info"][1] for a in annos])

    def _set(self, boxes, labels, off, height, width):
        self.boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)
        self.labels = np.ascontiguousarray(labels, dtype=np.int64)
        self.off = np.ascontiguousarray(off, dtype=np.int64)
        self.height = np.asarray(height, dtype=np.int64)
        self.width = np.asarray(width, dtype=np.int64)

    def __len__(self):
        return len(self.off) - 1

    def get_img_info(self, idx):
        return {"height": int(self.height[idx]), "width": int(self.width[idx])}

    def get_groundtruth(self, idx):
        """vid.py:220-227: BoxList of frame idx in the annotation's size, field "labels"."""
        s, e = self.off[idx], self.off[idx + 1]
        b = BoxList(torch.from_numpy(self.boxes[s:e].copy()), (int(self.width[idx]), int(self.height[idx])))
        b.add_field("labels", torch.from_numpy(self.labels[s:e].copy()))
        return b

    def map_class_id_to_class_name(self, class_id):
        return self.classes[class_id]


def parse_track_ids(root, name="<annotation>", classes_to_ind=CLASSES_TO_IND):
    """The <trackid> of every object parse_annotation keeps, in its order -> [n] i64.  ValueError (naming the file) for a
    kept object without one."""
    ids = []
    for obj in root.findall("object"):
        if obj.find("name").text not in classes_to_ind:
            continue
        t = obj.find("trackid")
        if t is None or t.text is None or not t.text.strip():
            raise ValueError("%s: an object has no <trackid>" % name)
        ids.append(int(t.text))
    return np.asarray(ids, dtype=np.int64)


class VIDTrackGroundTruth(VIDGroundTruth):
    """VIDGroundTruth plus track_ids [G] i64: the <trackid> of every kept object, what track_eval.evaluate_tracks judges
    linked tracks against.  Its .npz cache holds the same arrays and "track_ids" (a VIDGroundTruth cache, which has none,
    is re-read from the XML files and overwritten)."""

    def __init__(self, img_index, anno_path, cache=None):
        from .inference import VIDTestIndex
        self.image_set_index = list(VIDTestIndex(img_index).image_set_index)
        if cache and os.path.exists(cache):
            z = np.load(cache, allow_pickle=False)
            if "track_ids" in z.files and list(z["image_set_index"]) == self.image_set_index:
                self._set(z["boxes"], z["labels"], z["off"], z["height"], z["width"])
                self.track_ids = np.ascontiguousarray(z["track_ids"], dtype=np.int64)
                return
            logging.getLogger("mega.pytorch_amd.vid_eval").warning("%s lists other frames or no track ids: re-reading the "
                                                                   "XML files", cache)
        annos = []
        for name in self.image_set_index:
            path = os.path.join(anno_path, name + ".xml")
            root = ET.parse(path).getroot()
            annos.append(dict(parse_annotation(root), track_ids=parse_track_ids(root, path)))
        self._set_annos(annos)
        if cache:
            d = os.path.dirname(os.path.abspath(cache))
            os.makedirs(d, exist_ok=True)
            np.savez(cache, image_set_index=np.asarray(self.image_set_index), boxes=self.boxes, labels=self.labels,
                     off=self.off, height=self.height, width=self.width, track_ids=self.track_ids)

    @classmethod
    def from_annotations(cls, annos):
        """From a list of per-frame dicts: parse_annotation()'s keys plus "track_ids" [n]."""
        self = cls.__new__(cls)
        self.image_set_index = None
        self._set_annos(annos)
        return self

    def _set_annos(self, annos):
        super(VIDTrackGroundTruth, self)._set_annos(annos)
        for a in annos:
            if "track_ids" not in a or len(np.asarray(a["track_ids"]).reshape(-1)) != len(a["labels"]):
                raise ValueError("VIDTrackGroundTruth: every frame needs one track id per GT box")
        self.track_ids = np.concatenate([np.asarray(a["track_ids"], np.int64).reshape(-1) for a in annos]) if annos else \
            np.zeros((0,), np.int64)


def load_motion_iou(path):
    """vid_groundtruth_motion_iou.mat -> list (one entry per frame) of f64 arrays, entry j of frame i =
    m['motion_iou'][i][0][j][0], or 0 where that cell is empty (the values vid_eval.py:133-137 means to build).  In the
    reference's file frame i is an [n_gt x 1] array, and a frame without GT boxes a [1 x 0] one: one entry, 0."""
    import scipy.io as sio
    m = sio.loadmat(path)["motion_iou"]
    out = []
    for i in range(len(m)):
        cells = m[i][0]
        out.append(np.asarray([float(cells[j][0]) if len(cells[j]) != 0 else 0.0 for j in range(len(cells))],
                              dtype=np.float64))
    return out


def empty_weights(motion_iou, motion_ranges):
    """vid_eval.py:163-168: per range, the fraction of ALL motion entries (every frame of the file) inside [lo, hi];
    0 when that fraction is 1 or without motion IoUs."""
    if motion_iou is None:
        return [0.0] * len(motion_ranges)
    allm = np.concatenate([np.asarray(m, np.float64).reshape(-1) for m in motion_iou]) if len(motion_iou) else np.zeros(0)
    if allm.size == 0:
        raise ValueError("the motion IoU list holds no entries")
    out = []
    for lo, hi in motion_ranges:
        w = int(np.count_nonzero((allm >= lo) & (allm <= hi))) / float(allm.size)
        out.append(0.0 if w == 1 else w)
    return out


def format_result(result, classes=CLASSES, motion_names=None):
    """do_vid_evaluation's result text (vid_eval.py:53-64), byte for byte."""
    names = motion_names or (MOTION_NAMES if len(result) == len(MOTION_NAMES) else MOTION_NAMES[:len(result)])
    s = ""
    for mi in range(len(names)):
        s += 'AP50 | motion={:>6s} = {:0.4f}\n'.format(names[mi], result[mi]["map"])
    s += "Category AP:\n"
    for i, ap in enumerate(result[0]["ap"]):
        if i == 0:  # skip background
            continue
        s += "{:<16}: {:.4f}\n".format(classes[i], ap)
    return s


def write_result(text, logger, module, output_folder, file_name, lead="\n"):
    """How every evaluation of the package ends: `text` goes to the log (`logger`, or the logger of the package's `module`)
    behind `lead`, and to <output_folder>/<file_name> when a folder is given."""
    (logger or logging.getLogger("mega.pytorch_amd." + module)).info(lead + text)
    if output_folder:
        os.makedirs(output_folder, exist_ok=True)
        with open(os.path.join(output_folder, file_name), "w") as f:
            f.write(text)


def _resize_ratios(predictions, groundtruth):
    """[F,2] f32 (width, height): BoxList.resize (bounding_box.py:95) to the annotation's frame size -- ratios as Python
    floats, applied in f32."""
    pw = np.asarray([float(p.size[0]) for p in predictions])
    ph = np.asarray([float(p.size[1]) for p in predictions])
    return np.stack([groundtruth.width / pw, groundtruth.height / ph], axis=1).astype(np.float32)


def _pack(predictions, groundtruth, motion_iou, motion_ranges):
    """The checked flat host arrays of the whole evaluation, [(name, ndarray)] for flat.upload, and the sizes."""
    F = len(predictions)
    if F == 0:
        raise ValueError("evaluate_detections: no predictions")
    if len(groundtruth) != F:
        raise ValueError("Length of gt and pred lists need to be same (%d predictions, %d GT frames)" % (F, len(groundtruth)))
    counts, det_off, boxes, scores, labels = flat.concat_predictions(predictions)
    N = int(det_off[-1])
    if not np.isfinite(boxes).all():
        raise ValueError("evaluate_detections: a prediction box is not finite")
    if np.isnan(scores).any():
        raise ValueError("evaluate_detections: a prediction score is NaN")
    gl = groundtruth.labels
    if (N and labels.min() < 0) or (gl.size and gl.min() < 0):
        raise ValueError("evaluate_detections: negative class label")
    if not np.isfinite(groundtruth.boxes).all():
        raise ValueError("evaluate_detections: a GT box is not finite")
    C = int(max(labels.max() if N else -1, gl.max() if gl.size else -1)) + 1     # n_fg_class = max(seen) + 1
    if C <= 0:
        raise ValueError("evaluate_detections: no class occurs in the predictions or the GT")
    gcount = np.diff(groundtruth.off)
    max_gt = int(gcount.max()) if F else 0
    if max_gt > MAX_GT_PER_FRAME:
        raise ValueError("evaluate_detections: a frame holds %d GT boxes (at most %d)" % (max_gt, MAX_GT_PER_FRAME))
    ratio = _resize_ratios(predictions, groundtruth)
    G = int(groundtruth.off[-1])
    motion = None
    if motion_iou is not None:
        if len(motion_iou) < F:
            raise ValueError("the motion IoU list covers %d frames, %d are evaluated" % (len(motion_iou), F))
        motion = np.full(G, np.nan, np.float64)       # NaN: the frame has no motion list, nothing is ignored
        for i in np.nonzero(gcount)[0]:
            m = motion_iou[i]
            if len(m) == 0:
                continue
            if len(m) < gcount[i]:
                raise ValueError("frame %d: %d GT boxes, %d motion IoUs" % (i, gcount[i], len(m)))
            motion[groundtruth.off[i]:groundtruth.off[i + 1]] = np.asarray(m, np.float64)[:gcount[i]]
    ranges = np.asarray([[lo, hi, w] for (lo, hi), w in zip(motion_ranges, empty_weights(motion_iou, motion_ranges))],
                        np.float64)
    parts = [("det_box", boxes.astype(np.float32)), ("score", (scores + np.float32(0)).astype(np.float32)),   # -0 -> +0
             ("det_label", labels.astype(np.int32)), ("det_off", det_off), ("ratio", ratio),
             ("gt_box", groundtruth.boxes), ("gt_label", gl.astype(np.int32)), ("gt_off", groundtruth.off),
             ("ranges", ranges)]
    if motion is not None:
        parts.append(("gt_motion", motion))
    return parts, {"F": F, "N": N, "C": C, "max_gt": max_gt, "counts": counts}


def class_orders(scores, labels, counts, C, dev):
    """The two orders of the evaluation, on the device: scores [N] f32 and labels [N] i32 (flat, frame by frame), counts [F]
    (host) -> order [N] i32 (each frame's run by label, score descending, position descending: what the matching walks),
    gorder [N] i32 (each class's run over the dataset: score descending, then descending position in the frame-by-frame
    concatenation of the frames' ordered detections) and seg_off [C+1] i64 (class l's run of gorder)."""
    N = scores.shape[0]
    if N:
        # within-frame order: frame, label, score descending, position descending
        key = flat.frame_ids(counts, dev) * C + labels.long()
        order = flat.segment_order(scores, key, start=torch.arange(N - 1, -1, -1, device=dev))
        # per class over the dataset: score descending, then descending position in that frame-by-frame concatenation
        gorder = flat.segment_order(scores, labels, start=order.flip(0))
        order, gorder = order.int(), gorder.int()
        seg_off = torch.zeros(C + 1, dtype=torch.int64, device=dev)
        seg_off[1:] = torch.cumsum(torch.bincount(labels.long(), minlength=C), 0)
    else:
        order = gorder = torch.zeros(0, dtype=torch.int32, device=dev)
        seg_off = torch.zeros(C + 1, dtype=torch.int64, device=dev)
    return order, gorder, seg_off


def match_and_ap(predictions, groundtruth, motion_iou=None, device="cuda", ap_only=False):
    """The kernels' outputs (numpy): match [R,N] u8 and pred_ignore [R,N] f64 per detection (flat, frame by frame, in
    each BoxList's order), n_pos [R,C] i32, ap [R,C] f64, with R = 4 motion ranges (1 without motion IoUs).
    ap_only: copy back only ap (the per-detection arrays stay on the device and are freed)."""
    from . import ops
    dev = torch.device(device)
    flat.require_hip(dev, "evaluate_detections", device)
    motion_ranges = MOTION_RANGES if motion_iou is not None else MOTION_RANGES[:1]
    parts, meta = _pack(predictions, groundtruth, motion_iou, motion_ranges)
    F, N, C = meta["F"], meta["N"], meta["C"]
    t = flat.upload(parts, dev)
    labels = t["det_label"]
    order, gorder, seg_off = class_orders(t["score"], labels, meta["counts"], C, dev)
    with torch.cuda.device(dev):
        match, pign, n_pos = ops.vid_eval_match(t["det_box"], labels, t["det_off"], order, t["ratio"], t["gt_box"],
                                                t["gt_label"], t.get("gt_motion"), t["gt_off"], t["ranges"], C,
                                                meta["max_gt"])
        ap = ops.vid_eval_ap(match, pign, gorder, seg_off, n_pos)
    if ap_only:
        return {"ap": ap.cpu().numpy()}
    return {"match": match.cpu().numpy(), "pred_ignore": pign.cpu().numpy(), "n_pos": n_pos.cpu().numpy(),
            "ap": ap.cpu().numpy()}


def evaluate_detections(predictions, groundtruth, motion_iou=None, output_folder=None, device="cuda", box_only=False,
                        use_07_metric=False, logger=None, result_name="result.txt"):
    """eval_detection_vid (+ do_vid_evaluation's result.txt) for `predictions` (list[BoxList] with "scores" / "labels",
    boxes in the size each BoxList carries: what inference() returns or inference.load_predictions() reads, written by this
    package or by the reference) against `groundtruth` (VIDGroundTruth, same frames, same order).
    motion_iou: None (one range, "all") or load_motion_iou()'s per-frame lists (the 4 ranges all / fast / medium / slow);
    motion_iou.derive() computes such lists from the annotations' tracks.
    result_name: the file the text goes to in output_folder (result_seq_nms.txt for Seq-NMS-rescored predictions).
    -> {motion_index: {"ap": ndarray [n_fg_class] f64 (NaN: class not seen or without non-ignored GT), "map": nanmean}}."""
    if box_only:
        raise NotImplementedError("box_only proposal recall (eval_proposals_vid) is not provided by evaluate_detections: "
                                  "call vid_eval.evaluate_proposals on predictions with the field \"objectness\"")
    if use_07_metric:
        raise NotImplementedError("the VOC07 11-point metric is not provided (the reference hard-codes use_07_metric=False)")
    flat.require_hip(torch.device(device), "evaluate_detections", device)
    ap = match_and_ap(predictions, groundtruth, motion_iou, device, ap_only=True)["ap"]
    motion_ranges = MOTION_RANGES if motion_iou is not None else MOTION_RANGES[:1]
    result = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # nanmean of an all-NaN row is NaN, as in the reference
        for ri in range(len(motion_ranges)):
            result[ri] = {"ap": ap[ri].copy(), "map": np.nanmean(ap[ri])}
    write_result(format_result(result), logger, "vid_eval", output_folder, result_name)
    return result


# ------------------------------------------------------------------------------------------------ proposal recall
def proposal_inputs(predictions, groundtruth, limits, device="cuda"):
    """The checked, flat device arrays of ops.proposal_recall_match, in its argument order (one host-to-device copy, the
    within-frame objectness order sorted on the device) -> (box, off, order, ratio, gt_box, gt_off, limits, max_limit,
    max_gt)."""
    dev = torch.device(device)
    flat.require_hip(dev, "evaluate_detections", device)
    limits = [int(l) for l in limits]
    if not limits or min(limits) < 0:
        raise ValueError("evaluate_proposals: limits must be non-negative integers, got %r" % (limits,))
    if max(limits) > MAX_PROPOSAL_LIMIT:
        raise ValueError("evaluate_proposals: limit %d (at most %d)" % (max(limits), MAX_PROPOSAL_LIMIT))
    F = len(predictions)
    if F == 0:
        raise ValueError("evaluate_proposals: no predictions")
    if len(groundtruth) != F:
        raise ValueError("Length of gt and pred lists need to be same (%d predictions, %d GT frames)" % (F, len(groundtruth)))
    for p in predictions:
        if not p.has_field("objectness"):
            raise ValueError("evaluate_proposals: a prediction has no field \"objectness\" (fields: %r); proposals come "
                             "from a detector run with MODEL.RPN_ONLY True" % (sorted(p.fields()),))
    counts, off, boxes, obj = flat.concat_predictions(predictions, ("objectness",))
    N = int(off[-1])
    if not np.isfinite(boxes).all():
        raise ValueError("evaluate_proposals: a proposal box is not finite")
    if np.isnan(obj).any():
        raise ValueError("evaluate_proposals: an objectness value is NaN")
    if not np.isfinite(groundtruth.boxes).all():
        raise ValueError("evaluate_proposals: a GT box is not finite")
    gcount = np.diff(groundtruth.off)
    max_gt = int(gcount.max())
    if max_gt > MAX_GT_PER_FRAME:
        raise ValueError("evaluate_proposals: a frame holds %d GT boxes (at most %d)" % (max_gt, MAX_GT_PER_FRAME))
    t = flat.upload([("box", boxes), ("obj", (obj + np.float32(0)).astype(np.float32)),       # -0 -> +0
                     ("off", off), ("ratio", _resize_ratios(predictions, groundtruth)),
                     ("gt_box", groundtruth.boxes), ("gt_off", groundtruth.off),
                     ("limits", np.asarray(limits, np.int32))], dev)
    if N:
        # within a frame: objectness descending, equal values by ascending position
        order = flat.segment_order(t["obj"], flat.frame_ids(counts, dev)).int()
    else:
        order = torch.zeros(0, dtype=torch.int32, device=dev)
    return t["box"], t["off"], order, t["ratio"], t["gt_box"], t["gt_off"], t["limits"], max(limits), max_gt


def match_proposals(predictions, groundtruth, limits, device="cuda"):
    """eval_proposals_vid's greedy matching (vid_eval.py:79-111) of every frame, for all `limits` in one kernel launch
    -> (gt_overlap [nL,G] f32, gt_prop [nL,G] i32) on the device, indexed like groundtruth.boxes: the IoU each GT box was
    matched with (0: never matched) and the matched proposal's position in its frame's objectness order (-1: none)."""
    from . import ops
    args = proposal_inputs(predictions, groundtruth, limits, device)
    with torch.cuda.device(args[0].device):
        return ops.proposal_recall_match(*args)


def format_recall_table(limits, iou_thresholds, table, ar, num_pos):
    """The text of proposal_recall_table.txt: one row per proposal limit, AR (the mean over the IoU thresholds) and the
    recall at each threshold."""
    s = "Proposal recall, %d GT boxes\n" % num_pos
    s += "{:>6s} {:>6s}".format("limit", "AR") + "".join(" {:>6s}".format("@%.2f" % t) for t in iou_thresholds) + "\n"
    for li, lim in enumerate(limits):
        s += "{:>6d} {:.4f}".format(lim, ar[li]) + "".join(" {:.4f}".format(v) for v in table[li]) + "\n"
    return s


def evaluate_proposals(predictions, groundtruth, iou_thresh=0.5, limit=300, limits=None, iou_thresholds=None,
                       output_folder=None, device="cuda", logger=None):
    """do_vid_evaluation(box_only=True) / eval_proposals_vid (vid_eval.py:26-37, :72-119) for `predictions` (list[BoxList]
    with the field "objectness", boxes in the size each BoxList carries: what inference() returns under MODEL.RPN_ONLY)
    against `groundtruth` (VIDGroundTruth, same frames, same order): the recall of the GT boxes at IoU >= iou_thresh by
    each frame's first `limit` proposals, every proposal matched to at most one GT box.  num_pos counts every GT box,
    those of frames without proposals too; recall = f32(matched) / f32(num_pos) (NaN without GT boxes).
    "Recall: {:.4f}" goes to the log and to <output_folder>/proposal_result.txt, as the reference writes it.
    limits / iou_thresholds: when either is given (the other takes PROPOSAL_LIMITS / PROPOSAL_IOU_THRESHOLDS), also the
    recall table [limit, threshold] and its mean over thresholds (AR) per limit, written to proposal_recall_table.txt;
    all limits are matched in the same kernel launch.  Thresholds are compared in f32 and must be > 0 (an unmatched GT
    box has overlap 0).
    -> {"recall": f32, "num_pos": int, "gt_overlaps": [G] f32, "gt_prop": [G] i32 (by GT box: the IoU it was matched with
    and the matched proposal's position in the frame's objectness order, 0 / -1 if none)} and, with a table, "limits",
    "iou_thresholds", "table" [nL,nT] f32, "ar" [nL] f32."""
    flat.require_hip(torch.device(device), "evaluate_detections", device)
    want_table = limits is not None or iou_thresholds is not None
    tl = [int(l) for l in (PROPOSAL_LIMITS if limits is None else limits)] if want_table else []
    tt = [float(t) for t in (PROPOSAL_IOU_THRESHOLDS if iou_thresholds is None else iou_thresholds)] if want_table else []
    if want_table and (not tl or not tt):
        raise ValueError("evaluate_proposals: limits and iou_thresholds must not be empty")
    for t in [float(iou_thresh)] + tt:
        if not t > 0:
            raise ValueError("evaluate_proposals: IoU thresholds must be > 0, got %r" % (t,))
    launch = [int(limit)] + [l for l in tl if l != int(limit)]
    launch = sorted(set(launch), key=launch.index)
    ov, prop = match_proposals(predictions, groundtruth, launch, device)
    num_pos = int(groundtruth.off[-1])
    thr = torch.tensor([float(iou_thresh)] + tt, dtype=torch.float32, device=ov.device)
    hits = (ov[:, :, None] >= thr[None, None, :]).sum(dim=1).cpu().numpy()            # [launch, 1 + nT]

    def rec(n):
        return np.float32(n) / np.float32(num_pos) if num_pos else np.float32(np.nan)
    out = {"recall": rec(hits[0, 0]), "num_pos": num_pos, "gt_overlaps": ov[0].cpu().numpy(),
           "gt_prop": prop[0].cpu().numpy()}
    write_result("Recall: {:.4f}".format(out["recall"]), logger, "vid_eval", output_folder, "proposal_result.txt", lead="")
    if want_table:
        table = np.asarray([[rec(hits[launch.index(l), 1 + ti]) for ti in range(len(tt))] for l in tl], np.float32)
        ar = table.mean(axis=1, dtype=np.float32)
        out.update({"limits": tl, "iou_thresholds": tt, "table": table, "ar": ar})
        write_result(format_recall_table(tl, tt, table, ar, num_pos), logger, "vid_eval", output_folder,
                     "proposal_recall_table.txt")
    return out
