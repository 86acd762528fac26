"""GPU: test-time box augmentation -- the flip-resize entry against PIL, the candidate entries against the twin, the merge
kernel (csrc/bbox_aug.hip) against the numpy twin (tests/bbox_aug_twin.py) bit for bit, the K = 1 identity merge against
mega_postprocess, and inference() with TEST.BBOX_AUG for the engines of every method."""
import os

import numpy as np
import pytest
import torch

import bbox_aug_twin as tw
from mega.pytorch_amd import bbox_aug, config, feed, inference, modeling, ops, synth

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("in_hw,out_hw", [((37, 53), (60, 90)), ((48, 64), (48, 40)), ((48, 64), (30, 64)),
                                          ((30, 50), (30, 50)), ((64, 48), (21, 17))])
def test_flip_resize_equals_pil(dev, in_hw, out_hw):
    from PIL import Image
    frames = synth.make_clip(3, in_hw[0], in_hw[1], seed=sum(in_hw) + sum(out_hw))
    tables = feed.ResizeTables(in_hw, out_hw, dev) if in_hw != out_hw else None
    got = ops.resize_bilinear_u8_flip(frames.to(dev).contiguous(), out_hw, tables).cpu().numpy()
    for t in range(3):
        im = Image.fromarray(frames[t].numpy())
        if in_hw != out_hw:
            im = im.resize((out_hw[1], out_hw[0]), Image.BILINEAR)
        want = np.asarray(im.transpose(Image.FLIP_LEFT_RIGHT))
        np.testing.assert_array_equal(got[t], want)
    if tables is not None:       # hflip = 0 is the plain resize
        plain = ops.resize_bilinear_u8(frames.to(dev).contiguous(), out_hw, tables)
        assert torch.equal(ops.resize_bilinear_u8_flip(frames.to(dev).contiguous(), out_hw, tables, hflip=False), plain)


def test_frame_source_hflip(dev):
    host = synth.make_clip(4, 40, 70, seed=5).numpy()
    a = feed.FrameSource(None, None, 4, dev, min_size=30, max_size=100, opener=lambda f: host[f], workers=1)
    b = feed.FrameSource(None, None, 4, dev, min_size=30, max_size=100, opener=lambda f: host[f], workers=1, hflip=True)
    x, y = a.fetch([0, 1, 2, 3]), b.fetch([0, 1, 2, 3])
    assert torch.equal(x.flip(2), y)
    a.close(), b.close()


def _head_inputs(seed, R, NC=31, W=1000, H=600):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((R, NC), generator=g) * 1.5
    deltas = torch.randn((R, NC * 4), generator=g) * 0.5
    ctr = torch.rand((R, 2), generator=g) * torch.tensor([W - 100., H - 100.])
    wh = torch.rand((R, 2), generator=g) * 200 + 10
    props = torch.cat([ctr - wh / 2, ctr + wh / 2], dim=1).clamp(min=0)
    props[:, 2].clamp_(max=W - 1); props[:, 3].clamp_(max=H - 1)
    return logits, deltas, props


def test_candidates_match_twin_and_batched_equals_single(dev):
    B, R, NC = 3, 300, 31
    ins = [_head_inputs(b, R) for b in range(B)]
    lg, dl, pr = (torch.cat([x[i] for x in ins]).to(dev).contiguous() for i in range(3))
    nprop = torch.tensor([300, 217, 5], dtype=torch.int32, device=dev)
    w = (10.0, 10.0, 5.0, 5.0)
    cb, cs = ops.postprocess_candidates_batched(lg, dl, pr, B, w, 1000, 600, 0.001, nprop=nprop)
    for b in range(B):
        sl = slice(b * R, (b + 1) * R)
        sb, ss = ops.postprocess_candidates(lg[sl].contiguous(), dl[sl].contiguous(), pr[sl].contiguous(), nprop[b:b + 1], w,
                                            1000, 600, 0.001)
        assert torch.equal(sb, cb[b]) and torch.equal(ss, cs[b])
        tb, ts = tw.candidates(*ins[b], 1000, 600, nprop=int(nprop[b]))
        live = ts >= 0
        np.testing.assert_array_equal(cs[b].cpu().numpy() >= 0, live)
        np.testing.assert_allclose(cs[b].cpu().numpy(), ts, rtol=0, atol=1e-6)
        np.testing.assert_allclose(cb[b].cpu().numpy()[live], tb[live], rtol=0, atol=1e-3)


@pytest.mark.parametrize("R", [300, 77])
def test_k1_identity_merge_equals_postprocess(dev, R):
    """the merge of one identity view is the post-processor's P2-P4 on the same candidates: the same bits"""
    lg, dl, pr = (x.to(dev).contiguous() for x in _head_inputs(R, R))
    w = (10.0, 10.0, 5.0, 5.0)
    for strict in (True, False):
        ob, os_, ol, oc = ops.postprocess(lg, dl, pr, None, w, 1000, 600, 0.001, 0.5, 300, strict)
        cb, cs = ops.postprocess_candidates(lg, dl, pr, None, w, 1000, 600, 0.001)
        mb, ms, ml, mc = ops.bbox_aug_merge(cb[None, None].contiguous(), cs[None, None].contiguous(), [(1000, 600)], [False],
                                            0.001, 0.5, 300, strict)
        n = int(oc.item())
        assert int(mc[0].item()) == n and n > 0
        assert torch.equal(mb[0, :n], ob[:n]) and torch.equal(ms[0, :n], os_[:n]) and torch.equal(ml[0, :n], ol[:n])


def _merge_case(dev, frames, sizes, flips, max_det=300, strict=True):
    """frames[f] = list of K (boxes [C1,R,4], scores [C1,R]); the kernel on all frames == the twin per frame, bit for bit"""
    K = len(sizes)
    cb = torch.from_numpy(np.stack([np.stack([fr[k][0] for fr in frames]) for k in range(K)])).to(dev).contiguous()
    cs = torch.from_numpy(np.stack([np.stack([fr[k][1] for fr in frames]) for k in range(K)])).to(dev).contiguous()
    ob, os_, ol, oc = ops.bbox_aug_merge(cb, cs, sizes, flips, 0.001, 0.5, max_det, strict)
    counts = oc.tolist()
    for f, fr in enumerate(frames):
        wb, ws, wl = tw.merge(fr, sizes, flips, max_det=max_det, strict_gt=strict)
        n = counts[f]
        assert n == len(ws), "frame %d: %d vs twin %d" % (f, n, len(ws))
        np.testing.assert_array_equal(ol[f, :n].cpu().numpy(), wl)
        np.testing.assert_array_equal(_bits(os_[f, :n].cpu().numpy()), _bits(ws))
        np.testing.assert_array_equal(_bits(ob[f, :n].cpu().numpy()), _bits(wb))
    return counts


def test_merge_equals_twin_flip_scales_ties_empty(dev):
    """4 views (identity, its flip, a scale with unequal w / h ratios, its flip), scores on a coarse grid (exact ties, the
    k-th value cut with ties), 1,200 rows per class, and an empty frame"""
    sizes = [(160, 96), (160, 96), (203, 117), (203, 117)]
    flips = [False, True, False, True]
    frames = []
    for f in range(3):
        v, _ = tw.random_views(10 + f, 4, 300, C1=30, sizes=sizes, grid=25, empty=(f == 1))
        frames.append(v)
    counts = _merge_case(dev, frames, sizes, flips)
    assert counts[1] == 0 and counts[0] >= 300 and counts[2] >= 300      # (the cut keeps every tie of the 300th score)
    _merge_case(dev, frames, sizes, flips, max_det=0, strict=False)


def test_merge_equals_twin_at_the_row_and_view_limits(dev):
    """K = 16 views x R = 512 rows = 8,192 rows per class (the limit), and K = 2 x 1,000 rows"""
    sizes = [(120 + 7 * k, 80 + 3 * (k % 5)) for k in range(16)]
    flips = [k % 2 == 1 for k in range(16)]
    v, _ = tw.random_views(77, 16, 512, C1=2, sizes=sizes, grid=50, p_live=0.5)
    _merge_case(dev, [v], sizes, flips)
    v, _ = tw.random_views(78, 2, 1000, C1=3, sizes=sizes[:2], p_live=0.9)
    _merge_case(dev, [v], sizes[:2], flips[:2])


def test_merge_refuses_over_the_limit(dev):
    cs = torch.full((17, 1, 2, 4), -1.0, device=dev)
    cb = torch.zeros((17, 1, 2, 4, 4), device=dev)
    with pytest.raises(ValueError):
        ops.bbox_aug_merge(cb, cs, [(10, 10)] * 17, [False] * 17, 0.001, 0.5, 300)
    cs = torch.full((2, 1, 2, 4097), -1.0, device=dev)
    cb = torch.zeros((2, 1, 2, 4097, 4), device=dev)
    with pytest.raises(ValueError):
        ops.bbox_aug_merge(cb, cs, [(10, 10)] * 2, [False] * 2, 0.001, 0.5, 300)
    from mega.pytorch_amd import _lib
    lib = _lib.load()        # the C entry itself refuses (MEGA_ERR_LIMIT) before any launch; ws_bytes = 0, so that a
    # regressed limit check stops at the workspace check (MEGA_ERR_WS) instead of launching
    import ctypes
    arr = (ctypes.c_int * 17)(*([10] * 17))
    rc = lib.mega_bbox_aug_merge(cb.data_ptr(), cs.data_ptr(), 1, 17, 500, 3, ctypes.cast(arr, ctypes.c_void_p),
                                 ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(arr, ctypes.c_void_p), 0.001, 0.5, 1, 300,
                                 cb.data_ptr(), cs.data_ptr(), cb.data_ptr(), cs.data_ptr(), cb.data_ptr(), 0, None)
    assert rc == 4


def test_batched_merge_equals_per_frame_merges(dev):
    sizes, flips = [(160, 96), (160, 96), (96, 58)], [False, True, False]
    frames = [tw.random_views(40 + f, 3, 300, C1=30, sizes=sizes, grid=30)[0] for f in range(5)]
    K = 3
    cb = torch.from_numpy(np.stack([np.stack([fr[k][0] for fr in frames]) for k in range(K)])).to(dev).contiguous()
    cs = torch.from_numpy(np.stack([np.stack([fr[k][1] for fr in frames]) for k in range(K)])).to(dev).contiguous()
    ob, os_, ol, oc = ops.bbox_aug_merge(cb, cs, sizes, flips, 0.001, 0.5, 300)
    for f in range(5):
        b1, s1, l1, c1 = ops.bbox_aug_merge(cb[:, f:f + 1].contiguous(), cs[:, f:f + 1].contiguous(), sizes, flips, 0.001,
                                            0.5, 300)
        n = int(c1.item())
        assert int(oc[f].item()) == n
        assert torch.equal(ob[f, :n], b1[0, :n]) and torch.equal(os_[f, :n], s1[0, :n]) and torch.equal(ol[f, :n], l1[0, :n])


# ------------------------------------------------------------------------------------------------ inference() end to end
L, H0, W0 = 12, 90, 160


def _video(tmp_path):
    from PIL import Image
    clip0 = synth.make_clip(L, H0, W0, seed=9).numpy()
    os.makedirs(str(tmp_path / "Data" / "v"), exist_ok=True)
    lines = []
    for t in range(L):
        Image.fromarray(clip0[t]).save(str(tmp_path / "Data" / "v" / ("%06d.JPEG" % t)), format="PNG")
        lines.append("v %d %d %d" % (t + 1, t, L))
    (tmp_path / "index.txt").write_text("\n".join(lines) + "\n")
    return str(tmp_path / "Data"), str(tmp_path / "index.txt")


def _model(dev, method):
    import mega.pytorch_amd.fgfa  # noqa: F401
    cfg = config.get_cfg("R-50", method)
    cfg.DTYPE = "bfloat16"
    cfg.MODEL.DEVICE = str(dev)
    cfg.NMS_STRICT_GT = True
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 180, 320
    if method == "mega":
        sd = synth.make_state_dict(blocks=(3, 4, 6), reduce_channel=True, global_res_stage=0, seed=1)
    elif method == "rdn":
        import mega.pytorch_amd.rdn  # noqa: F401
        sd = synth.make_rdn_state_dict(advanced_stage=1, seed=2)
    elif method == "fgfa":
        sd = synth.make_fgfa_state_dict(seed=3)
    elif method == "dff":
        sd = synth.make_dff_state_dict(seed=3)
    else:
        sd = {k: v for k, v in synth.make_fgfa_state_dict(seed=3).items() if not k.startswith(("flownet.", "embednet."))}
    model = modeling.build_detection_model(cfg)
    model.load_state_dict(sd)
    model.to(dev)
    return cfg, model


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.size == y.size and len(x) == len(y)
        assert torch.equal(x.bbox, y.bbox) and torch.equal(x.get_field("scores"), y.get_field("scores"))
        assert torch.equal(x.get_field("labels"), y.get_field("labels"))


@pytest.mark.parametrize("method", ["mega", "rdn", "fgfa", "dff", "base"])
def test_inference_bbox_aug(dev, tmp_path, method, monkeypatch):
    """ENABLED with the identity view alone == ENABLED=False (predictions.pth tensors); with H_FLIP + one scale the result
    is the twin merge of the candidates the engines produced for the views."""
    img_dir, idx = _video(tmp_path)
    cfg, model = _model(dev, method)
    plain = inference.inference(cfg, model, img_dir, idx, output_folder=str(tmp_path / "plain"))
    cfg.TEST.BBOX_AUG.ENABLED = True
    ident = inference.inference(cfg, model, img_dir, idx, output_folder=str(tmp_path / "ident"))
    assert not model.roi_heads.box.post_processor.candidates          # candidate mode only inside the run
    _same(plain, ident)
    _same(inference.load_predictions(str(tmp_path / "plain" / "predictions.pth")),
          inference.load_predictions(str(tmp_path / "ident" / "predictions.pth")))
    assert plain[0].size == (320, 180)
    cfg.TEST.BBOX_AUG.H_FLIP = True
    cfg.TEST.BBOX_AUG.SCALES = (130,)
    cfg.TEST.BBOX_AUG.MAX_SIZE = 250
    seen = {}
    real = bbox_aug.merge

    def spy(per_view, views, pp, chunk=16):
        seen["per_view"] = [(b.cpu().numpy(), s.cpu().numpy()) for b, s in per_view]
        seen["views"] = views
        return real(per_view, views, pp, chunk=5)          # (chunks of 5 frames: 12 = 5 + 5 + 2)
    monkeypatch.setattr(bbox_aug, "merge", spy)
    aug = inference.inference(cfg, model, img_dir, idx, output_folder=str(tmp_path / "aug"))
    views = seen["views"]
    assert [(v.hflip, v.size) for v in views] == [(False, (320, 180)), (True, (320, 180)), (False, (231, 130))]
    sizes, flips = [v.size for v in views], [v.hflip for v in views]
    assert len(aug) == L
    for f in range(L):
        wb, ws, wl = tw.merge([(b[f], s[f]) for b, s in seen["per_view"]], sizes, flips)
        a = aug[f]
        assert a.size == (320, 180) and len(a) == len(ws)
        np.testing.assert_array_equal(a.get_field("labels").numpy(), wl)
        np.testing.assert_array_equal(_bits(a.get_field("scores").numpy()), _bits(ws))
        np.testing.assert_array_equal(_bits(a.bbox.numpy()), _bits(wb))
    assert sum(len(a) for a in aug) > 0


def test_inference_bbox_aug_with_seq_nms_and_eval(dev, tmp_path):
    """inference(..., seq_nms=True, anno_path=...) with TEST.BBOX_AUG writes every output"""
    from test_vid_eval_gpu import _xml
    from mega.pytorch_amd import vid_eval
    img_dir, idx = _video(tmp_path)
    ann = tmp_path / "Annotations" / "v"
    os.makedirs(str(ann))
    for t in range(L):
        (ann / ("%06d.xml" % t)).write_text(_xml(H0, W0, [(vid_eval.CLASSES_MAP[1 + t % 30], (10, 10, 60, 50))]))
    cfg, model = _model(dev, "base")
    cfg.TEST.BBOX_AUG.ENABLED = True
    cfg.TEST.BBOX_AUG.H_FLIP = True
    out = tmp_path / "out"
    inference.inference(cfg, model, img_dir, idx, output_folder=str(out), seq_nms=True,
                        anno_path=str(tmp_path / "Annotations"))
    for name in ("predictions.pth", "predictions_seq_nms.pth", "result.txt", "result_seq_nms.txt"):
        assert (out / name).exists(), name


@pytest.mark.parametrize("engine_kwargs", [None, {"per_frame": True}])
def test_base_detector_with_tta_vs_reference_fixture(dev, tmp_path, engine_kwargs):
    """tests/golden/ref_bbox_aug.npz (the reference's unmodified im_detect_bbox_aug on the base R-50 detector, CPU): the
    same frames through inference() with the same TEST.BBOX_AUG views (identity, flip, 145x97 and its flip), f32,
    NMS_STRICT_GT False (the CPU rule), under the tolerances of
    test_e2e_gpu.py::test_base_single_frame_detector_vs_reference_fixture"""
    from PIL import Image
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_bbox_aug.npz"))
    H, W = int(d["cfg_H"]), int(d["cfg_W"])
    clip0 = synth.make_clip(2, H, W, seed=int(d["cfg_seed_clip"])).numpy()
    os.makedirs(str(tmp_path / "Data" / "v"))
    for t in range(2):
        Image.fromarray(clip0[t]).save(str(tmp_path / "Data" / "v" / ("%06d.JPEG" % t)), format="PNG")
    (tmp_path / "index.txt").write_text("v 1 0 2\nv 2 1 2\n")
    import mega.pytorch_amd.fgfa  # noqa: F401
    cfg = config.get_cfg("R-50", "base")
    cfg.MODEL.DEVICE = str(dev)
    cfg.NMS_STRICT_GT = False
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = int(d["cfg_min_size"]), int(d["cfg_max_size"])
    cfg.merge_from_list(["TEST.BBOX_AUG.ENABLED", True, "TEST.BBOX_AUG.H_FLIP", True,
                         "TEST.BBOX_AUG.SCALES", (int(d["cfg_scale"]),), "TEST.BBOX_AUG.MAX_SIZE", int(d["cfg_aug_max_size"]),
                         "TEST.BBOX_AUG.SCALE_H_FLIP", True])
    sd = {k: v for k, v in synth.make_fgfa_state_dict(seed=int(d["cfg_seed_w"])).items()
          if not k.startswith(("flownet.", "embednet."))}
    model = modeling.build_detection_model(cfg)
    model.load_state_dict(sd)
    model.to(dev)
    preds = inference.inference(cfg, model, str(tmp_path / "Data"), str(tmp_path / "index.txt"),
                                engine_kwargs=engine_kwargs)
    assert len(preds) == 2
    for idx, det in enumerate(preds):
        rb, rs, rl = d["boxes%d" % idx], d["scores%d" % idx], d["labels%d" % idx]
        gb, gs, gl = det.bbox.numpy(), det.get_field("scores").numpy(), det.get_field("labels").numpy()
        assert det.size == tuple(int(x) for x in d["size%d" % idx])
        assert len(det) == rb.shape[0] > 0
        unmatched = 0
        for k in range(len(rl)):
            m = (gl == rl[k]) & (np.abs(gs - rs[k]) < 1e-4) & (np.abs(gb - rb[k]).max(axis=1) < 2e-2)
            unmatched += 0 if m.any() else 1
        assert unmatched == 0, "frame %d: %d reference detections have no match" % (idx, unmatched)
