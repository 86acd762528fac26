"""CPU: the VID evaluation's host side and its spec.  The numpy twin (tests/vid_twin.py) of what the HIP kernels compute
reproduces the reference's own outputs recorded in tests/golden/ref_vid_eval.npz (make_vid_eval.py); the annotation
parser, the motion-IoU reader, result.txt and the new C entry points' argument checks need no GPU."""
import os

import numpy as np
import pytest
import torch

import vid_twin
from mega.pytorch_amd import _lib, vid_eval
from mega.pytorch_amd.structures import BoxList

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vid_eval.npz")


def golden_frames(z):
    preds, gts, motion = [], [], []
    po, go, mo = z["pred_off"], z["gt_off"], z["motion_off"]
    for i in range(len(po) - 1):
        preds.append({"box": z["pred_box"][po[i]:po[i + 1]], "score": z["pred_score"][po[i]:po[i + 1]],
                      "label": z["pred_label"][po[i]:po[i + 1]], "size": tuple(int(v) for v in z["pred_size"][i])})
        gts.append({"box": z["gt_box"][go[i]:go[i + 1]], "label": z["gt_label"][go[i]:go[i + 1]],
                    "im_info": tuple(int(v) for v in z["gt_hw"][i])})
        motion.append([float(v) for v in z["motion"][mo[i]:mo[i + 1]]])
    return preds, gts, motion


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("case", ["motion", "nomotion"])
def test_twin_reproduces_reference(gold, case):
    preds, gts, motion = golden_frames(gold)
    res = vid_twin.evaluate(preds, gts, motion if case == "motion" else None)
    assert len(res) == (4 if case == "motion" else 1)
    for ri, d in enumerate(res):
        key = "%s_r%d_" % (case, ri)
        np.testing.assert_array_equal(d["n_pos"], gold[key + "n_pos"])
        C = len(gold[key + "ap"])
        assert len(d["ap"]) == C
        for l in range(C):
            if key + "match_%d" % l in gold:
                np.testing.assert_array_equal(d["match_l"][l], gold[key + "match_%d" % l])
                np.testing.assert_array_equal(d["pred_ignore_l"][l], gold[key + "pred_ignore_%d" % l])
            else:
                assert len(d["match_l"].get(l, [])) == 0
            for what in ("prec", "rec"):
                if key + "%s_%d" % (what, l) in gold:
                    np.testing.assert_array_equal(d[what][l], gold[key + "%s_%d" % (what, l)])
                else:
                    assert d[what][l] is None
        np.testing.assert_allclose(d["ap"], gold[key + "ap"], rtol=0, atol=1e-12, equal_nan=True)


def test_golden_covers_the_edge_cases(gold):
    preds, gts, motion = golden_frames(gold)
    assert any(len(p["score"]) == 0 for p in preds) and any(len(g["label"]) == 0 for g in gts)
    assert any(len(m) == 0 and len(g["label"]) for m, g in zip(motion, gts))
    assert any(p["size"] != (g["im_info"][1], g["im_info"][0]) and
               p["size"][0] / g["im_info"][1] != p["size"][1] / g["im_info"][0] for p, g in zip(preds, gts))
    m = gold["motion"]
    assert (m == 0.7).any() and (m == 0.9).any()
    ap = gold["motion_r0_ap"]
    assert np.isnan(ap).any() and (ap == 0).any() or np.isnan(ap[15])
    # an IoU of exactly 0.5 and a 0 / 0 IoU occur among same-class pairs
    seen_half = seen_nan = False
    for p, g in zip(preds, gts):
        pb = vid_twin.rescale(p["box"], p["size"], g["im_info"])
        for l in np.unique(p["label"]):
            a, b = pb[p["label"] == l].copy(), g["box"][g["label"] == l].copy()
            if len(a) and len(b):
                a[:, 2:] += 1
                b[:, 2:] += 1
                iou = vid_twin.iou_f32(a, b)
                seen_half |= bool((iou == 0.5).any())
                seen_nan |= bool(np.isnan(iou).any())
    assert seen_half and seen_nan


def test_twin_tie_order():
    # one frame, one class, three equal scores: ordered by descending position within the frame ...
    p = {"box": np.float32([[0, 0, 9, 9], [0, 0, 9, 9], [0, 0, 9, 9]]), "score": np.float32([0.5, 0.5, 0.5]),
         "label": np.int64([1, 1, 1]), "size": (100, 100)}
    g = {"box": np.float32([[0, 0, 9, 9]]), "label": np.int64([1]), "im_info": (100, 100)}
    d = vid_twin.prec_rec([p], [g])
    np.testing.assert_array_equal(d["match"], [0, 0, 1])          # the LAST listed box takes the GT
    # ... and over the dataset by descending position in the frame-by-frame concatenation: frame 1's tied match first
    p2 = {"box": np.float32([[50, 50, 60, 60]]), "score": np.float32([0.5]), "label": np.int64([1]), "size": (100, 100)}
    g2 = {"box": np.float32([[0, 0, 9, 9]]), "label": np.int64([1]), "im_info": (100, 100)}
    d = vid_twin.prec_rec([p2, p], [g2, g])
    # concatenation (within-frame order): [f0 miss, f1 pos2 (tp), f1 pos1, f1 pos0]; global descending position:
    # f1 pos0 (fp), f1 pos1 (fp), f1 pos2 (tp), f0 (fp)
    np.testing.assert_allclose(d["prec"][1], [0, 0, 1 / 3, 1 / 4], atol=1e-15)
    assert vid_twin.desc_order(np.float32([0.5, 0.7, 0.5, 0.5])).tolist() == [1, 3, 2, 0]


def test_parse_annotation_matches_reference(gold):
    import xml.etree.ElementTree as ET
    assert list(gold["classes"]) == vid_eval.CLASSES and list(gold["classes_map"]) == vid_eval.CLASSES_MAP
    for i, x in enumerate(gold["xml"]):
        res = vid_eval.parse_annotation(ET.fromstring(str(x)))
        assert res["boxes"].dtype == np.float32
        np.testing.assert_array_equal(res["boxes"], gold["xml%d_boxes" % i].reshape(-1, 4))
        np.testing.assert_array_equal(res["labels"], gold["xml%d_labels" % i])
        assert tuple(res["im_info"]) == tuple(gold["xml%d_im_info" % i])


def _write_dataset(tmp_path, xmls):
    ann = tmp_path / "Annotations"
    (ann / "vid_a").mkdir(parents=True)
    lines = []
    for i, x in enumerate(xmls):
        (ann / "vid_a" / ("%06d.xml" % i)).write_text(x)
        lines.append("vid_a 1 %d %d" % (i, len(xmls)))
    idx = tmp_path / "index.txt"
    idx.write_text("\n".join(lines) + "\n")
    return str(idx), str(ann)


def test_groundtruth_and_cache(gold, tmp_path):
    xmls = [str(x) for x in gold["xml"]]
    idx, ann = _write_dataset(tmp_path, xmls)
    cache = str(tmp_path / "cache" / "gt.npz")
    gt = vid_eval.VIDGroundTruth(idx, ann, cache=cache)
    assert len(gt) == 3 and os.path.exists(cache)
    for i in range(3):
        b = gt.get_groundtruth(i)
        np.testing.assert_array_equal(b.bbox.numpy(), gold["xml%d_boxes" % i].reshape(-1, 4))
        np.testing.assert_array_equal(b.get_field("labels").numpy(), gold["xml%d_labels" % i])
        h, w = gold["xml%d_im_info" % i]
        assert gt.get_img_info(i) == {"height": h, "width": w} and b.size == (w, h)
    os.rename(ann, ann + ".gone")              # the cache alone serves the same frames
    gt2 = vid_eval.VIDGroundTruth(idx, ann, cache=cache)
    for a in ("boxes", "labels", "off", "height", "width"):
        np.testing.assert_array_equal(getattr(gt2, a), getattr(gt, a))


def test_load_motion_iou(tmp_path):
    sio = pytest.importorskip("scipy.io")
    # the reference file's nesting: motion_iou [n_frames x 1] cells; frame i an [n_gt x 1] f64 array, [1 x 0] without GT
    frames = [np.array([[0.25], [0.75]]), np.zeros((1, 0)), np.array([[0.5], [0.0], [0.95]])]
    outer = np.empty((len(frames), 1), dtype=object)
    for i, f in enumerate(frames):
        outer[i, 0] = f
    path = str(tmp_path / "motion.mat")
    sio.savemat(path, {"motion_iou": outer})
    m = vid_eval.load_motion_iou(path)
    assert len(m) == 3
    np.testing.assert_array_equal(m[0], [0.25, 0.75])
    np.testing.assert_array_equal(m[1], [0.0])          # one empty cell -> one entry 0
    assert m[1].dtype == np.float64
    np.testing.assert_array_equal(m[2], [0.5, 0.0, 0.95])
    # the reference's own indexing on the same file gives the same values
    raw = sio.loadmat(path)["motion_iou"]
    ref = [[raw[i][0][j][0] if len(raw[i][0][j]) != 0 else 0 for j in range(len(raw[i][0]))] for i in range(len(raw))]
    for a, b in zip(m, ref):
        np.testing.assert_array_equal(a, np.asarray(b, np.float64).reshape(-1))


def test_empty_weights_over_the_whole_file():
    motion = [[0.1, 0.8], [], [0.95, 0.7, 0.9]]
    w = vid_eval.empty_weights(motion, vid_eval.MOTION_RANGES)
    assert w == [0.0, 0.4, 0.6, 0.4]           # "all" holds every entry: 1 -> 0
    for (lo, hi), x in zip(vid_eval.MOTION_RANGES, w):
        assert x == vid_twin.empty_weight(motion, lo, hi)
    assert vid_eval.empty_weights(None, vid_eval.MOTION_RANGES[:1]) == [0.0]


def test_result_text_format():
    ap = np.full(31, np.nan)
    ap[1], ap[2], ap[30] = 0.5, 0.123456, 1.0
    res = {0: {"ap": ap, "map": np.nanmean(ap)}, 1: {"ap": ap, "map": 0.25}, 2: {"ap": ap, "map": np.nan},
           3: {"ap": ap, "map": 0.0}}
    s = vid_eval.format_result(res)
    lines = s.split("\n")
    assert lines[0] == "AP50 | motion=   all = 0.5412"
    assert lines[1] == "AP50 | motion=  fast = 0.2500"
    assert lines[2] == "AP50 | motion=medium = nan"
    assert lines[3] == "AP50 | motion=  slow = 0.0000"
    assert lines[4] == "Category AP:"
    assert lines[5] == "airplane        : 0.5000"
    assert lines[6] == "antelope        : 0.1235"
    assert lines[7] == "bear            : nan"
    assert lines[34] == "zebra           : 1.0000" and lines[35] == "" and len(lines) == 36
    one = vid_eval.format_result({0: res[0]})
    assert one.startswith("AP50 | motion=   all = 0.5412\nCategory AP:\nairplane")


def test_out_of_scope_and_bad_input_errors():
    p = BoxList(torch.zeros((1, 4)), (10, 10))
    p.add_field("scores", torch.ones(1))
    p.add_field("labels", torch.ones(1, dtype=torch.int64))
    gt = vid_eval.VIDGroundTruth.from_annotations([{"boxes": np.zeros((0, 4)), "labels": np.zeros(0), "im_info": (10, 10)}])
    with pytest.raises(NotImplementedError):
        vid_eval.evaluate_detections([p], gt, box_only=True)
    with pytest.raises(NotImplementedError):
        vid_eval.evaluate_detections([p], gt, use_07_metric=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vid_eval.evaluate_detections([p], gt, device="cpu")
    with pytest.raises(ValueError, match="same"):
        vid_eval._pack([p, p], gt, None, vid_eval.MOTION_RANGES[:1])
    with pytest.raises(ValueError, match="motion IoU list covers"):
        vid_eval._pack([p], gt, [], vid_eval.MOTION_RANGES)


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    # NULL pointers / non-positive sizes come back as MEGA_ERR_ARG before any launch
    assert lib.mega_vid_eval_match(None, None, None, None, None, None, None, None, None, None, 1, 1, 1, 0, 0,
                                   None, None, None, None) == 1
    assert lib.mega_vid_eval_match(None, None, 8, None, 8, None, None, None, 8, 8, 0, 1, 1, 0, 0, None, None, 8, None) == 1
    assert lib.mega_vid_eval_match(None, None, 8, None, 8, None, None, None, 8, 8, 1, 1, 1, 4, 0, None, None, 8, None) == 1
    assert lib.mega_vid_eval_match(8, 8, 8, 8, 8, 8, 8, None, 8, 8, 1, 1, 1, 4, 4097, 8, 8, 8, None) == 1
    assert lib.mega_vid_eval_ap(None, None, None, None, None, 1, 1, 0, None, None, 0, None) == 1
    assert lib.mega_vid_eval_ap(None, None, None, 8, 8, 0, 1, 0, 8, 8, 1 << 20, None) == 1
    assert lib.mega_vid_eval_ap(None, None, None, 8, 8, 2, 1, 5, 8, 8, 1 << 20, None) == 1
    nb = lib.mega_vid_eval_workspace_bytes(5000, 31, 4)
    assert nb >= 4 * (5000 // 1024 + 32) * 12
    assert lib.mega_vid_eval_ap(8, 8, 8, 8, 8, 31, 4, 5000, 8, 8, nb - 1, None) == 3      # workspace too small
    assert lib.mega_vid_eval_workspace_bytes(-1, 31, 4) == 0 and lib.mega_vid_eval_workspace_bytes(10, 0, 4) == 0
