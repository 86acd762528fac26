"""Value types and small host functions against what the reference package returns for the same inputs
(tests/golden/ref_live.npz: seeded inputs and the reference's outputs, recorded from the reference itself by
tests/golden/make_golden.py golden_live)."""
import os

import numpy as np
import pytest
import torch

from mega.pytorch_amd import config, modeling, structures, synth

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_live.npz"))


def _t(key):
    return torch.from_numpy(GOLD[key])


def test_boxlist_semantics():
    """bounding_box.py: clip_to_image (in place, remove_empty), indexing, fields, copy_with_fields, to()."""
    for seed in range(5):
        b, s = _t("bl%d_boxes" % seed), _t("bl%d_scores" % seed)
        mine = structures.BoxList(b.clone(), (256, 160), "xyxy")
        mine.add_field("scores", s.clone())
        mine.add_field("labels", torch.arange(40))
        for remove_empty in (False, True):
            k = "bl%d_clip%d_" % (seed, remove_empty)
            m2 = structures.BoxList(b.clone(), (256, 160), "xyxy"); m2.add_field("scores", s.clone())
            mo_ = m2.clip_to_image(remove_empty)
            assert torch.equal(mo_.bbox, _t(k + "bbox")) and torch.equal(mo_.get_field("scores"), _t(k + "scores"))
            assert torch.equal(m2.bbox, _t(k + "inplace_bbox"))        # the clamp happened in place, as in the reference
        idx = torch.tensor([3, 1, 7])
        assert torch.equal(mine[idx].bbox, _t("bl%d_idx_bbox" % seed))
        assert torch.equal(mine[idx].get_field("labels"), _t("bl%d_idx_labels" % seed))
        keep = s > 0.5
        assert torch.equal(mine[keep].bbox, _t("bl%d_keep_bbox" % seed)) and len(mine[keep]) == len(GOLD["bl%d_keep_bbox" % seed])
        assert mine.fields() == GOLD["bl_fields"].tolist() and mine.size == tuple(GOLD["bl_size"].tolist())
        assert mine.mode == str(GOLD["bl_mode"])
        c1 = mine.copy_with_fields(["scores"])
        assert c1.fields() == GOLD["bl_copy_fields"].tolist() and torch.equal(c1.bbox, _t("bl%d_copy_bbox" % seed))
        with pytest.raises(KeyError):
            mine.copy_with_fields(["nope"])
        assert repr(mine).startswith("BoxList(num_boxes=40")


def test_cat_boxlist_and_image_list():
    def mk(x, f):
        bl = structures.BoxList(x.clone(), (100, 80), "xyxy")
        bl.add_field("scores", f.clone())
        return bl
    m = structures.cat_boxlist([mk(_t("cat_a"), _t("cat_fa")), mk(_t("cat_b"), _t("cat_fb"))])
    assert torch.equal(m.bbox, _t("cat_bbox")) and torch.equal(m.get_field("scores"), _t("cat_scores"))
    assert m.size == tuple(GOLD["cat_size"].tolist())
    img = _t("img")
    for k, inp in enumerate((img, [img], (img,))):
        mi = structures.to_image_list(inp)
        assert torch.equal(mi.tensors, _t("il%d_tensors" % k))
        assert [tuple(x) for x in mi.image_sizes] == [tuple(x) for x in GOLD["il%d_sizes" % k].tolist()]
    assert structures.to_image_list(mi) is mi


def test_convert_to_roi_format_and_anchor_buffers():
    """poolers.py:78-89 (batch index column, concatenation order) and the anchor generator's cell anchors as they sit
    in the reference model's state_dict."""
    boxes = [structures.BoxList(_t("roi_boxes%d" % i), (64, 64)) for i in range(2)]
    assert torch.equal(modeling.convert_to_roi_format(boxes), _t("roi_format"))
    mcfg = config.get_cfg("R-50")
    mcfg.MODEL.DEVICE = "cpu"
    mine = modeling.build_detection_model(mcfg)
    key = "rpn.anchor_generator.cell_anchors.0"
    assert torch.equal(mine.state_dict()[key], _t("cell_anchors0"))
    assert torch.equal(synth._cell_anchors(16, (64, 128, 256, 512), (0.5, 1.0, 2.0)), _t("cell_anchors0"))
    a = mine.state_dict()
    assert list(a.keys()) == GOLD["sd_keys"].tolist()
    assert [",".join(str(d) for d in v.shape) for v in a.values()] == GOLD["sd_shapes"].tolist()
