"""Generates tests/golden/ref_proposal_recall.npz FROM THE REFERENCE ITSELF (run on CPU where the reference tree is
available; the fixture is committed so that the tests never need the reference).

  python tests/golden/make_proposal_recall.py

The reference's evaluation/vid/vid_eval.py is loaded by file path under oracle/ref_shim.py (as make_vid_eval.py does) and
its do_vid_evaluation(box_only=True) is run unmodified on CPU, on a stub dataset that hands out the seeded frames'
sizes and GT BoxLists: the predictions are resized with the reference's BoxList.resize, eval_proposals_vid matches them,
and proposal_result.txt is written by the reference.  eval_proposals_vid's sorted `gt_overlaps` and `num_pos` are read
from its locals when it returns (a profile hook: nothing in the reference is changed), the recall from its return value.

Frames: tests/proposal_recall_twin.make_frames; asserted here: no frame has tied objectness values (torch's descending
sort is not stable), and the set holds a frame without GT, one without proposals, one with more GT boxes than
proposals, one with more than 300 proposals, one with duplicate proposals and one whose width / height ratios differ.
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import make_vid_eval  # noqa: E402
import proposal_recall_twin as twin  # noqa: E402

OUT = os.path.join(HERE, "ref_proposal_recall.npz")
SEED, FRAMES = 20261017, 80


def check_cases(preds, gts):
    has = dict.fromkeys(("no_gt", "no_prop", "gt_gt_prop", "gt_300", "dup", "ratio"), False)
    for p, g in zip(preds, gts):
        n, k = len(p["obj"]), len(g["box"])
        assert len(np.unique(p["obj"])) == n, "tied objectness within a frame"
        has["no_gt"] |= k == 0 and n > 0
        has["no_prop"] |= n == 0 and k > 0
        has["gt_gt_prop"] |= k > n > 0
        has["gt_300"] |= n > 300 and k > 0
        has["dup"] |= k > 0 and len(np.unique(p["box"], axis=0)) < n
        H, W = g["im_info"]
        has["ratio"] |= k > 0 and n > 0 and float(W) / p["size"][0] != float(H) / p["size"][1]
    assert all(has.values()), has


def run_reference(ve, preds, gts, folder):
    from mega_core.structures.bounding_box import BoxList as RefBoxList

    class Dataset(object):
        def get_img_info(self, i):
            return {"height": gts[i]["im_info"][0], "width": gts[i]["im_info"][1]}

        def get_groundtruth(self, i):
            g = gts[i]
            return RefBoxList(torch.from_numpy(g["box"].copy()), (g["im_info"][1], g["im_info"][0]), mode="xyxy")

    class Logger(object):
        lines = []

        def info(self, s):
            self.lines.append(s)

    pred_bl = []
    for p in preds:
        b = RefBoxList(torch.from_numpy(p["box"].copy()), p["size"], mode="xyxy")
        b.add_field("objectness", torch.from_numpy(p["obj"].copy()))
        pred_bl.append(b)
    captured = {}

    def hook(frame, event, arg):
        if event == "return" and frame.f_code is ve.eval_proposals_vid.__code__:
            captured.update({"gt_overlaps": frame.f_locals["gt_overlaps"].clone(), "num_pos": frame.f_locals["num_pos"],
                             "recall": arg["recall"]})
    sys.setprofile(hook)
    try:
        ve.do_vid_evaluation(Dataset(), pred_bl, folder, box_only=True, motion_specific=False, logger=Logger())
    finally:
        sys.setprofile(None)
    captured["text"] = open(os.path.join(folder, "proposal_result.txt")).read()
    assert Logger.lines == [captured["text"]]
    return captured


def main():
    ve = make_vid_eval.load_ref_vid_eval()
    preds, gts = twin.make_frames(SEED, F=FRAMES)
    check_cases(preds, gts)
    with tempfile.TemporaryDirectory() as td:
        cap = run_reference(ve, preds, gts, td)
    d = {}
    d["pred_box"] = np.concatenate([p["box"] for p in preds]).astype(np.float32).reshape(-1, 4)
    d["pred_obj"] = np.concatenate([p["obj"] for p in preds]).astype(np.float32)
    d["pred_off"] = np.concatenate([[0], np.cumsum([len(p["obj"]) for p in preds])]).astype(np.int64)
    d["pred_size"] = np.asarray([p["size"] for p in preds], np.int64)
    d["gt_box"] = np.concatenate([g["box"] for g in gts]).astype(np.float32).reshape(-1, 4)
    d["gt_off"] = np.concatenate([[0], np.cumsum([len(g["box"]) for g in gts])]).astype(np.int64)
    d["gt_hw"] = np.asarray([g["im_info"] for g in gts], np.int64)
    d["ref_gt_overlaps_sorted"] = cap["gt_overlaps"].numpy().astype(np.float32)
    d["ref_num_pos"] = np.asarray(int(cap["num_pos"]), np.int64)
    assert cap["recall"].dtype == torch.float32
    d["ref_recall"] = np.asarray(cap["recall"].item(), np.float32)
    d["ref_text"] = np.asarray(cap["text"])
    np.savez_compressed(OUT, **d)
    print("wrote", OUT, "%d proposals, %d GT boxes," % (len(d["pred_obj"]), len(d["gt_box"])), cap["text"],
          "(f32 %r)" % float(d["ref_recall"]))


if __name__ == "__main__":
    main()
