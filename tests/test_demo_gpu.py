"""GPU: the overlay kernel (csrc/overlay.hip through ops.overlay_detections) against the numpy twin
(tests/overlay_twin.py) bit for bit, its argument checks, and VIDDemo end to end for mega and base: detections equal to
compute_on_dataset, every returned frame equal to the twin on the host-decoded original, JPEG files as Pillow encodes
them.  Every GPU step runs once."""
import io
import os

import numpy as np
import pytest
import torch

import overlay_twin as tw
from mega.pytorch_amd import _lib, config, demo, inference, modeling, ops, synth

pytestmark = pytest.mark.gpu

ATLAS = demo.LabelAtlas(*demo.glyph_atlas(16))
PALETTE = demo.class_palette(len(demo.CATEGORIES))


def _run(dev, frames, box, score, label, counts, rhw, thr, thickness, label_dtype=torch.int64):
    d = ops.overlay_detections(torch.from_numpy(frames).to(dev), torch.from_numpy(box).to(dev),
                               torch.from_numpy(score).to(dev), torch.from_numpy(label).to(dev).to(label_dtype),
                               torch.from_numpy(counts).to(dev), rhw, thr, thickness, torch.from_numpy(PALETTE).to(dev),
                               ATLAS.to(dev))
    return d.cpu().numpy()


# (original size, resized size, F, R, thickness, threshold): every size, F, R, thickness and threshold of the list below
# appears, the 720 x 1280 frames with the non-power-of-two ratio from 562 x 1000
CASES = [
    ((720, 1280), (562, 1000), 16, 300, 1, 0.0),
    ((720, 1280), (562, 1000), 5, 300, 3, 0.7),
    ((720, 1280), (562, 1000), 1, 37, 5, 0.0),
    ((720, 1280), (600, 1067), 5, 1, 1, 0.7),
    ((720, 1280), (562, 1000), 5, 37, 3, 1.0),
    ((375, 500), (600, 800), 16, 37, 5, 0.7),
    ((375, 500), (600, 800), 1, 300, 3, 0.0),
    ((375, 500), (375, 500), 5, 0, 1, 0.0),
    ((375, 500), (600, 800), 5, 1, 5, 1.0),
    ((16, 64), (16, 64), 1, 37, 1, 0.0),
    ((16, 64), (32, 128), 16, 300, 5, 0.7),
    ((16, 64), (40, 160), 5, 1, 3, 0.0),
    ((16, 64), (16, 64), 1, 0, 3, 0.7),
]


@pytest.mark.parametrize("hw,rhw,F,R,thickness,thr", CASES)
def test_kernel_equals_twin(dev, hw, rhw, F, R, thickness, thr):
    """seeded frames and detections: score ties (a grid of 1/64, 0.7 and 1.0 as f32), boxes crossing all four edges,
    wholly outside, degenerate, classes outside the palette, counts smaller than R"""
    seed = hash((hw, rhw, F, R, thickness)) % 1000
    frames = np.random.default_rng(seed).integers(0, 256, (F,) + hw + (3,)).astype(np.uint8)
    box, score, label, counts = tw.random_detections(seed, F, R, rhw)
    if R > 1:
        assert (counts < R).any() or F == 1
    got = _run(dev, frames, box, score, label, counts, rhw, thr, thickness)
    want = tw.draw_batch(frames, box, score, label, counts, rhw, thr, thickness, PALETTE, ATLAS, demo.CATEGORIES)
    changed = int((want != frames).any(3).sum())
    print("overlay %s <- %s F=%d R=%d t=%d thr=%.1f: %d pixels drawn, %d differ" % (
        hw, rhw, F, R, thickness, thr, changed, int((got != want).any(3).sum())))
    np.testing.assert_array_equal(got, want)
    if thr == 1.0 or R == 0:
        assert changed == 0
    elif R >= 37 and thr == 0.0:
        assert changed > 0
    for f in range(F):      # a frame with no kept detection is unchanged bit for bit
        if not tw.draw_list(box[f], score[f], label[f], counts[f], hw, rhw, thr, len(PALETTE)):
            np.testing.assert_array_equal(got[f], frames[f])


def test_i32_labels_and_a_frame_without_kept_detections(dev):
    hw = rhw = (96, 160)
    frames = np.random.default_rng(1).integers(0, 256, (3,) + hw + (3,)).astype(np.uint8)
    box, score, label, counts = tw.random_detections(11, 3, 40, rhw)
    score[1] = np.minimum(score[1], np.float32(0.5))      # frame 1 keeps nothing at 0.5 (strict)
    counts[:] = 40
    got = _run(dev, frames, box, score, label, counts, rhw, 0.5, 3, label_dtype=torch.int32)
    want = tw.draw_batch(frames, box, score, label, counts, rhw, 0.5, 3, PALETTE, ATLAS, demo.CATEGORIES)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[1], frames[1])
    assert (got[0] != frames[0]).any() and (got[2] != frames[2]).any()


def test_limits_are_refused_before_any_launch(dev):
    hw = (32, 64)
    frames = np.random.default_rng(2).integers(0, 256, (1,) + hw + (3,)).astype(np.uint8)
    for R, thickness, code in ((513, 1, "code 4"), (8, 2, "code 1"), (8, 0, "code 1")):
        box, score, label, counts = tw.random_detections(3, 1, R, hw)
        counts[:] = R
        d = torch.from_numpy(frames).to(dev)
        with pytest.raises(RuntimeError, match=code):
            ops.overlay_detections(d, torch.from_numpy(box).to(dev), torch.from_numpy(score).to(dev),
                                   torch.from_numpy(label).to(dev), torch.from_numpy(counts).to(dev), hw, 0.0, thickness,
                                   torch.from_numpy(PALETTE).to(dev), ATLAS.to(dev))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(d.cpu().numpy(), frames)
    assert _lib.load().mega_overlay_detections(None, 1, 32, 64, None, None, None, 1, None, 513, 1.0, 1.0, 0.0, 1, None, 31,
                                               None, 14, None, None, None, 40, 19, 9, 0, None, 0, None) == 4


# ------------------------------------------------------------------------------------------------ VIDDemo end to end
L, H0, W0 = 32, 90, 160


def _folder(tmp_path):
    from PIL import Image
    clip0 = synth.make_clip(L, H0, W0, seed=9).numpy()
    os.makedirs(str(tmp_path / "Data" / "v"), exist_ok=True)
    lines = []
    for t in range(L):
        Image.fromarray(clip0[t]).save(str(tmp_path / "Data" / "v" / ("%06d.JPEG" % t)), format="JPEG", quality=92)
        lines.append("v %d %d %d" % (t + 1, t, L))
    (tmp_path / "index.txt").write_text("\n".join(lines) + "\n")
    return str(tmp_path / "Data"), str(tmp_path / "index.txt")


def _model(dev, method):
    import mega.pytorch_amd.fgfa  # noqa: F401
    cfg = config.get_cfg("R-50", method)
    cfg.MODEL.DEVICE = str(dev)
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 180, 320      # the resized frame is twice the original
    if method == "mega":
        sd = synth.make_state_dict(blocks=(3, 4, 6), reduce_channel=True, global_res_stage=0, seed=1)
    else:
        sd = {k: v for k, v in synth.make_fgfa_state_dict(seed=3).items() if not k.startswith(("flownet.", "embednet."))}
    model = modeling.build_detection_model(cfg)
    model.load_state_dict(sd)
    model.to(dev)
    return cfg, model


@pytest.mark.parametrize("method", ["mega", "base"])
def test_viddemo_end_to_end(dev, tmp_path, method):
    from PIL import Image
    img_dir, idx = _folder(tmp_path)
    cfg, model = _model(dev, method)
    index = inference.VIDTestIndex(idx)
    ref = inference.compute_on_dataset(model, index, img_dir, dev, steps_per_batch=4)
    ref = [ref[i] for i in range(L)]
    assert sum(len(p) for p in ref) > 0
    # (c) the threshold comes from the fixture's own scores: the smallest per-frame best score, so the frame that holds it
    # draws nothing (strict >) and the frames with a better best score draw at least that detection
    origs = [np.asarray(Image.open(os.path.join(img_dir, "v", "%06d.JPEG" % t)).convert("RGB")) for t in range(L)]
    best = [float(p.get_field("scores").max()) if len(p) else 0.0 for p in ref]
    thr = min(best)

    def kept(t):
        p = ref[t]
        return len(tw.draw_list(p.bbox.numpy(), p.get_field("scores").numpy(), p.get_field("labels").numpy(), len(p),
                                (H0, W0), (180, 320), thr, len(PALETTE)))
    n_kept = [kept(t) for t in range(L)]
    print("%s: per-frame best scores %.4f .. %.4f, threshold %.6f, frames drawing: %d of %d" % (
        method, min(best), max(best), thr, sum(n > 0 for n in n_kept), L))
    assert sum(n > 0 for n in n_kept) * 2 >= L and any(n == 0 for n in n_kept)
    out = tmp_path / "out"
    d = demo.VIDDemo(cfg, model, confidence_threshold=thr, thickness=3, output_folder=str(out), steps_per_batch=4,
                     render_chunk=10)
    frames = d.run_on_image_folder(os.path.join(img_dir, "v"))
    assert len(frames) == L and len(d.predictions) == L
    for t in range(L):
        p, r = d.predictions[t], ref[t]
        # (a) the detections of the test loop, bit for bit
        assert p.size == r.size == (320, 180) and len(p) == len(r)
        assert torch.equal(p.bbox, r.bbox) and torch.equal(p.get_field("scores"), r.get_field("scores"))
        assert torch.equal(p.get_field("labels"), r.get_field("labels"))
        # (b) the twin on the host-decoded original
        want = tw.draw(origs[t], p.bbox.numpy(), p.get_field("scores").numpy(), p.get_field("labels").numpy(), len(p),
                       (180, 320), thr, 3, d.palette, d.atlas, demo.CATEGORIES)
        assert frames[t].shape == (H0, W0, 3) and frames[t].dtype == np.uint8
        np.testing.assert_array_equal(frames[t], want)
        assert bool((want != origs[t]).any()) == (n_kept[t] > 0)
        # (d) the files
        buf = io.BytesIO()
        Image.fromarray(frames[t]).save(buf, format="JPEG", quality=demo.JPEG_QUALITY)
        assert (out / ("%06d.jpg" % t)).read_bytes() == buf.getvalue()
