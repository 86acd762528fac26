"""Generates tests/golden/ref_bbox_aug.npz FROM THE REFERENCE ITSELF: the unmodified
mega_core/engine/bbox_aug.py im_detect_bbox_aug on CPU under oracle/ref_shim.py, on the single-frame base detector
(configs/vid_R_50_C4_1x.yaml, weights synth.make_fgfa_state_dict as make_golden.golden_base uses) and two seeded
synth.make_clip frames as PIL images.

  python tests/golden/make_bbox_aug.py

Views: identity at 128 / 192 (a fixed point of Resize.get_size for the 192x128 frames: no resample), its flip, scale
97 at MAX_SIZE 1000 (145x97: unequal width / height ratios, BoxList.resize's per-axis branch) and its flip.

torchvision is absent here.  Its calls are bound to the exact Pillow / torch calls torchvision implements them with, as
make_golden.golden_feed does: F.resize -> PIL resize BILINEAR, F.to_tensor -> HWC u8 / 255 -> CHW, F.normalize ->
(x - mean) / std, TT.RandomHorizontalFlip(1.0) -> Image.transpose(FLIP_LEFT_RIGHT), TT.ToTensor -> F.to_tensor.  The
TT.Compose stand-in takes element 0 of the (image, target) tuples that MEGA's T.Resize / T.Normalize return: upstream
maskrcnn-benchmark's T.Resize returned the image alone when given no target, the behaviour bbox_aug.py was written
for; MEGA's returns a tuple, which torchvision's Compose would hand on to ToTensor as it is.

Recorded: each view's raw model output for frame 0 (the PostProcessor's candidates with bbox_aug_enabled: R * NC rows,
background included, scores not thresholded; a flipped view's before BoxList.transpose) with its image size, and the
merged detections of both frames.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_shim  # noqa: E402
from mega.pytorch_amd import synth  # noqa: E402

CASE = dict(H=128, W=192, seed_w=2, seed_clip=4, min_size=128, max_size=192, scale=97, aug_max_size=1000)


def main():
    from PIL import Image
    c = CASE
    cfg = ref_shim.make_cfg("configs/vid_R_50_C4_1x.yaml", opts=[
        "INPUT.MIN_SIZE_TEST", c["min_size"], "INPUT.MAX_SIZE_TEST", c["max_size"],
        "TEST.BBOX_AUG.ENABLED", True, "TEST.BBOX_AUG.H_FLIP", True, "TEST.BBOX_AUG.SCALES", (c["scale"],),
        "TEST.BBOX_AUG.MAX_SIZE", c["aug_max_size"], "TEST.BBOX_AUG.SCALE_H_FLIP", True])
    import mega_core.data.transforms.transforms as T
    F = types.SimpleNamespace(
        resize=lambda img, size: img.resize(size[::-1], Image.BILINEAR),
        to_tensor=lambda img: torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).float().div(255),
        normalize=lambda t, mean, std: (t - torch.tensor(mean).view(-1, 1, 1)) / torch.tensor(std).view(-1, 1, 1))
    T.F = F

    class Compose(object):
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, x):
            for t in self.transforms:
                x = t(x)
                if isinstance(x, tuple):
                    x = x[0]
            return x

    class RandomHorizontalFlip(object):
        def __init__(self, p):
            assert p == 1.0

        def __call__(self, img):
            return img.transpose(Image.FLIP_LEFT_RIGHT)

    class ToTensor(object):
        def __call__(self, img):
            return F.to_tensor(img)
    tt = sys.modules["torchvision.transforms"]
    tt.Compose, tt.RandomHorizontalFlip, tt.ToTensor = Compose, RandomHorizontalFlip, ToTensor
    from mega_core.engine.bbox_aug import im_detect_bbox_aug

    model = ref_shim.build_model(cfg)
    assert model.roi_heads.box.post_processor.bbox_aug_enabled
    sd = {k: v for k, v in synth.make_fgfa_state_dict(seed=c["seed_w"]).items()
          if not k.startswith(("flownet.", "embednet."))}
    model.load_state_dict(sd, strict=True)
    calls = []
    model.register_forward_hook(lambda m, i, o: calls.append([(b.bbox.clone(), b.get_field("scores").clone(), b.size)
                                                              for b in o]))
    clip = synth.make_clip(2, c["H"], c["W"], seed=c["seed_clip"]).numpy()
    out = {}
    for idx in range(2):
        del calls[:]
        with torch.no_grad():
            det = im_detect_bbox_aug(model, [Image.fromarray(clip[idx])], torch.device("cpu"))[0]
        assert len(calls) == 4
        out["boxes%d" % idx] = det.bbox.numpy()
        out["scores%d" % idx] = det.get_field("scores").numpy()
        out["labels%d" % idx] = det.get_field("labels").numpy()
        out["size%d" % idx] = np.array(det.size, np.int64)
        if idx == 0:
            for k, call in enumerate(calls):
                b, s, size = call[0]
                out["cand_boxes_v%d" % k] = b.numpy()
                out["cand_scores_v%d" % k] = s.numpy()
                out["cand_size_v%d" % k] = np.array(size, np.int64)
        print("frame", idx, "merged", det.bbox.shape[0], "view sizes", [call[0][2] for call in calls])
    out["view_flip"] = np.array([0, 1, 0, 1], np.int64)
    for k, v in c.items():
        out["cfg_" + k] = np.int64(v)
    np.savez_compressed(os.path.join(HERE, "ref_bbox_aug.npz"), **out)


if __name__ == "__main__":
    if not ref_shim.available():
        sys.exit("needs /root/reference")
    torch.set_num_threads(8)
    main()
