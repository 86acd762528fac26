"""Generates tests/golden/ref_vid_eval.npz FROM THE REFERENCE ITSELF (run on CPU where the reference tree is available;
the fixture is committed so that the tests never need the reference).

  python tests/golden/make_vid_eval.py

The reference's evaluation/vid/vid_eval.py is loaded by file path (its package __init__ imports the COCO / cityscapes
evaluators) under oracle/ref_shim.py and run unmodified on CPU:
  - predictions are resized with the reference's BoxList.resize, as do_vid_evaluation does (vid_eval.py:16-21);
  - calc_detection_vid_prec_rec / calc_detection_vid_ap are called directly with the motion IoUs as Python lists
    (eval_detection_vid reads the .mat itself and builds a ragged np.array, which numpy >= 1.24 rejects);
  - the per-class match / pred_ignore lists and n_pos are read from calc_detection_vid_prec_rec's locals when it
    returns (a profile hook: nothing in the reference is changed).
Cases: "motion" (4 motion ranges) and "nomotion" (one range) on seeded synthetic frames (tests/vid_twin.make_frames)
whose scores are free of ties within each (frame, class) and each class -- asserted here, because numpy's order of
equal scores is platform-defined -- plus the reference's _preprocess_annotation (vid.py:139-166) on synthetic XML.
"""
import importlib.util
import os
import sys
import xml.etree.ElementTree as ET

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_shim  # noqa: E402
import vid_twin  # noqa: E402

OUT = os.path.join(HERE, "ref_vid_eval.npz")
SEED, FRAMES = 20261015, 80

XMLS = [
    # two known wnids, one unknown, one box past the frame, one with negative coordinates
    """<annotation><size><width>500</width><height>375</height></size>
<object><name>n02691156</name><bndbox><xmax>120</xmax><xmin>10</xmin><ymax>90</ymax><ymin>20</ymin></bndbox></object>
<object><name>n99999999</name><bndbox><xmax>50</xmax><xmin>1</xmin><ymax>50</ymax><ymin>1</ymin></bndbox></object>
<object><name>n02391049</name><bndbox><xmax>700</xmax><xmin>-5</xmin><ymax>400</ymax><ymin>-3</ymin></bndbox></object>
</annotation>""",
    # no objects
    """<annotation><size><width>1280</width><height>720</height></size></annotation>""",
    # only an unknown class, then a known one with fractional coordinates
    """<annotation><size><width>640</width><height>480</height></size>
<object><name>n00000001</name><bndbox><xmax>5</xmax><xmin>1</xmin><ymax>5</ymax><ymin>1</ymin></bndbox></object>
<object><name>n02084071</name><bndbox><xmax>639.5</xmax><xmin>0.5</xmin><ymax>479</ymax><ymin>2.25</ymin></bndbox></object>
</annotation>""",
]


def load_ref_vid_eval():
    ref_shim.install()
    path = os.path.join(ref_shim.REF_ROOT, "mega_core", "data", "datasets", "evaluation", "vid", "vid_eval.py")
    spec = importlib.util.spec_from_file_location("ref_vid_eval", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assert_no_ties(preds):
    by_class = {}
    for p in preds:
        for l in np.unique(p["label"]):
            s = p["score"][p["label"] == l]
            assert len(np.unique(s)) == len(s), "tied scores within a frame's class"
            by_class.setdefault(int(l), []).append(s)
    for l, ss in by_class.items():
        s = np.concatenate(ss)
        assert len(np.unique(s)) == len(s), "tied scores within class %d" % l


def run_reference(ve, preds, gts, motion, ranges):
    from mega_core.structures.bounding_box import BoxList as RefBoxList
    pred_bl, gt_bl = [], []
    for p, g in zip(preds, gts):
        b = RefBoxList(torch.from_numpy(p["box"].copy()), p["size"], mode="xyxy")
        b.add_field("scores", torch.from_numpy(p["score"].copy()))
        b.add_field("labels", torch.from_numpy(p["label"].copy()))
        pred_bl.append(b.resize((g["im_info"][1], g["im_info"][0])))
        t = RefBoxList(torch.from_numpy(g["box"].copy()), (g["im_info"][1], g["im_info"][0]), mode="xyxy")
        t.add_field("labels", torch.from_numpy(g["label"].copy()))
        gt_bl.append(t)
    out = []
    for r in ranges:
        captured = {}

        def hook(frame, event, arg):
            if event == "return" and frame.f_code is ve.calc_detection_vid_prec_rec.__code__:
                captured.update({k: frame.f_locals[k] for k in ("match", "pred_ignore", "n_pos")})
        sys.setprofile(hook)
        try:
            prec, rec = ve.calc_detection_vid_prec_rec(gt_boxlists=gt_bl, pred_boxlists=pred_bl, motion_ious=motion,
                                                       iou_thresh=0.5, motion_range=r)
        finally:
            sys.setprofile(None)
        ap = ve.calc_detection_vid_ap(prec, rec, use_07_metric=False)
        out.append((prec, rec, ap, captured))
    return out


def main():
    ve = load_ref_vid_eval()
    import mega_core.data.datasets.vid as ref_vid
    d = {}
    preds, gts, motion = vid_twin.make_frames(SEED, F=FRAMES)
    assert_no_ties(preds)
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dt).reshape((-1,) + np.asarray(x).shape[1:]) for x in xs])  # noqa
    d["pred_box"] = cat([p["box"] for p in preds], np.float32).reshape(-1, 4)
    d["pred_score"] = cat([p["score"] for p in preds], np.float32)
    d["pred_label"] = cat([p["label"] for p in preds], np.int64)
    d["pred_off"] = np.concatenate([[0], np.cumsum([len(p["score"]) for p in preds])]).astype(np.int64)
    d["pred_size"] = np.asarray([p["size"] for p in preds], np.int64)
    d["gt_box"] = cat([g["box"] for g in gts], np.float32).reshape(-1, 4)
    d["gt_label"] = cat([g["label"] for g in gts], np.int64)
    d["gt_off"] = np.concatenate([[0], np.cumsum([len(g["label"]) for g in gts])]).astype(np.int64)
    d["gt_hw"] = np.asarray([g["im_info"] for g in gts], np.int64)
    d["motion"] = np.concatenate([np.asarray(m, np.float64) for m in motion])
    d["motion_off"] = np.concatenate([[0], np.cumsum([len(m) for m in motion])]).astype(np.int64)
    for case, mot, ranges in (("motion", motion, vid_twin.MOTION_RANGES), ("nomotion", None, vid_twin.MOTION_RANGES[:1])):
        for ri, (prec, rec, ap, cap) in enumerate(run_reference(ve, preds, gts, mot, ranges)):
            key = "%s_r%d_" % (case, ri)
            d[key + "ap"] = np.asarray(ap, np.float64)
            n_pos = np.zeros(len(prec), np.int64)
            for l, v in cap["n_pos"].items():
                n_pos[l] = int(v)
            d[key + "n_pos"] = n_pos
            for l in range(len(prec)):
                if l in cap["match"]:
                    d[key + "match_%d" % l] = np.asarray(cap["match"][l], np.int64)
                    d[key + "pred_ignore_%d" % l] = np.asarray(cap["pred_ignore"][l], np.float64)
                if prec[l] is not None:
                    d[key + "prec_%d" % l] = np.asarray(prec[l], np.float64)
                if rec[l] is not None:
                    d[key + "rec_%d" % l] = np.asarray(rec[l], np.float64)
            print(case, ri, "mAP %.6f" % np.nanmean(ap))
    # _preprocess_annotation on a stub that only carries classes_to_ind (vid.py:81)
    stub = type("Stub", (), {})()
    stub.classes_to_ind = dict(zip(ref_vid.VIDDataset.classes_map, range(len(ref_vid.VIDDataset.classes_map))))
    d["xml"] = np.asarray(XMLS)
    for i, x in enumerate(XMLS):
        res = ref_vid.VIDDataset._preprocess_annotation(stub, ET.fromstring(x))
        d["xml%d_boxes" % i] = res["boxes"].numpy()
        d["xml%d_labels" % i] = res["labels"].numpy().astype(np.int64)
        d["xml%d_im_info" % i] = np.asarray(res["im_info"], np.int64)
    d["classes"] = np.asarray(ref_vid.VIDDataset.classes)
    d["classes_map"] = np.asarray(ref_vid.VIDDataset.classes_map)
    np.savez_compressed(OUT, **d)
    print("wrote", OUT, "%d detections, %d GT boxes" % (len(d["pred_score"]), len(d["gt_label"])))


if __name__ == "__main__":
    main()
