"""GPU: the device half of the JPEG decode.  ops.jpeg_reconstruct on the twin's coefficients equals the twin's RGB byte for
byte and, on the stream cases, Pillow's -- at N = 1 and N = 3, with output and workspace poisoned beforehand; a
feed.FrameSource(decode="device") hands out the same frames as the host path through every way of asking for them; frames the
decoder refuses fall back to the host one by one; and the detections of a video do not depend on the mode."""
import io
import os

import numpy as np
import pytest
import torch

import jpeg_cases
import jpeg_twin
import poison
from mega.pytorch_amd import feed, jpeg, ops

pytestmark = pytest.mark.gpu

STREAMS = jpeg_cases.stream_cases()
COEFS = jpeg_cases.coef_cases()
_REF = {}


def _stream_ref(name, data):
    """(info, coefficients by the C decoder, Pillow's RGB), once per case"""
    if name not in _REF:
        info = jpeg.probe(data)
        _REF[name] = (info, ops.jpeg_entropy_decode(data, info), jpeg_cases.pillow_rgb(data))
    return _REF[name]


def _reconstruct(dev, info, bufs, mode):
    """bufs: one coefficient buffer per frame -> uint8 [N, H, W, 3] on the host, run under poison `mode`"""
    host = np.zeros((len(bufs), info.stride), dtype=np.int16)
    for i, b in enumerate(bufs):
        host[i, :info.coef_elems] = b
    coef = torch.from_numpy(host).to(dev)
    with poison.poisoned(mode, (ops,)) as p:
        out = ops.jpeg_reconstruct(coef, info)
        assert p.count == 2      # the output and the workspace of the component planes, both filled beforehand
    return out.cpu().numpy()


@pytest.mark.parametrize("name, data", STREAMS, ids=[n for n, _ in STREAMS])
def test_reconstruct_equals_pillow_on_stream_cases(dev, name, data):
    info, buf, want = _stream_ref(name, data)
    assert np.array_equal(jpeg_twin.reconstruct(buf, info.width, info.height, info.sampling), want)
    for mode in ("zeros", "ones"):
        got = _reconstruct(dev, info, [buf], mode)
        assert got.shape == (1,) + want.shape and np.array_equal(got[0], want), mode
    # N = 3: the frame between two copies of another case of the same geometry (its own coefficients shifted), each in its slot
    other = np.roll(buf[jpeg.QT_ELEMS:], 64)
    b2 = np.concatenate([buf[:jpeg.QT_ELEMS], other])
    want2 = jpeg_twin.reconstruct(b2, info.width, info.height, info.sampling)
    got = _reconstruct(dev, info, [b2, buf, b2], "ones")
    assert np.array_equal(got[1], want) and np.array_equal(got[0], want2) and np.array_equal(got[2], want2)


@pytest.mark.parametrize("case", COEFS, ids=[c[0] for c in COEFS])
def test_reconstruct_equals_twin_on_coefficient_cases(dev, case):
    name, w, h, s, buf = case
    info = jpeg.make_info(w, h, s)
    want = jpeg_twin.reconstruct(buf, w, h, s)
    for mode in ("zeros", "ones"):
        assert np.array_equal(_reconstruct(dev, info, [buf], mode)[0], want), mode
    neg = buf.copy()
    neg[jpeg.QT_ELEMS:] = -np.maximum(neg[jpeg.QT_ELEMS:], -32767)
    got = _reconstruct(dev, info, [buf, neg, buf], "ones")
    assert np.array_equal(got[0], want) and np.array_equal(got[2], want)
    assert np.array_equal(got[1], jpeg_twin.reconstruct(neg, w, h, s))


def test_reconstruct_batch_of_three_images(dev):
    datas = jpeg_cases.batch_case()
    info = jpeg.probe(datas[0])
    bufs = [ops.jpeg_entropy_decode(d, info) for d in datas]
    got = _reconstruct(dev, info, bufs, "ones")
    for i, d in enumerate(datas):
        assert np.array_equal(got[i], jpeg_cases.pillow_rgb(d)), i
    # a stride beyond the frame's element count, and an output tensor of the caller's
    host = np.full((3, info.stride + 64), 0x5A5A, dtype=np.int16)
    for i, b in enumerate(bufs):
        host[i, :info.coef_elems] = b
    out = torch.full((3, info.height, info.width, 3), 7, dtype=torch.uint8, device=dev)
    assert ops.jpeg_reconstruct(torch.from_numpy(host).to(dev), info, out=out) is out
    assert np.array_equal(out.cpu().numpy(), got)
    # a slice of a batch: frames of 33 x 50 x 3 bytes are odd-sized, so frame 1 starts off a dword (stored byte by byte)
    big = torch.full((3, info.height, info.width, 3), 7, dtype=torch.uint8, device=dev)
    ops.jpeg_reconstruct(torch.from_numpy(host).to(dev)[1:], info, out=big[1:])
    assert big[1:].data_ptr() % 4 != 0 and np.array_equal(big[1:].cpu().numpy(), got[1:]) and bool((big[0] == 7).all())


def test_reconstruct_at_a_dword_aligned_width_and_video_size(dev):
    """W % 4 == 0 takes the dword stores; 96 x 128 has several thread blocks per launch in 4:2:0 and 4:4:4"""
    for s, code in ((2, jpeg.S420), (1, jpeg.S422), (0, jpeg.S444), (None, jpeg.GRAY)):
        d = jpeg_cases.encode(jpeg_cases.picture(128, 96, 31, noise=(s == 0)), s, 92)
        info = jpeg.probe(d)
        assert info.sampling == code and info.width % 4 == 0
        got = _reconstruct(dev, info, [ops.jpeg_entropy_decode(d, info)] * 2, "ones")
        want = jpeg_cases.pillow_rgb(d)
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want), s


# ------------------------------------------------------------------------------------------------ the feed
def _jpeg_folder(tmp_path, n=6, w=45, h=67, sampling=2, special=None, suffix="JPEG"):
    """n frames `%06d.<suffix>` of w x h; special: {frame: (sampling, keyword arguments of the encoder)}"""
    os.makedirs(str(tmp_path), exist_ok=True)
    for t in range(n):
        s, kw = (special or {}).get(t, (sampling, {}))
        rgb = jpeg_cases.picture(w, h, 300 + t, noise=(t == 1))
        if suffix == "png":
            from PIL import Image
            Image.fromarray(rgb).save(str(tmp_path / ("%06d.png" % t)))
        else:
            (tmp_path / ("%06d.%s" % (t, suffix))).write_bytes(jpeg_cases.encode(rgb, s, 90, **kw))
    return str(tmp_path / ("%s." + suffix))


def _compare_sources(dev, pattern, n, **size):
    """every way of asking a decode="device" source for frames gives what the decode="host" source gives; returns it"""
    srcs = {}
    for mode in ("host", "device"):
        srcs[mode] = feed.FrameSource(pattern, "%06d", n, dev, workers=3, decode=mode, **size)
    host, devs = srcs["host"], srcs["device"]
    assert host.decode_mode == "host" and host.host_fallbacks == 0
    assert devs.in_hw == host.in_hw and devs.out_hw == host.out_hw and devs.shape == host.shape
    ids = list(range(n))
    for ask in (ids, [4, 1], [2], [5, 0, 3, 3]):
        assert torch.equal(devs.fetch_original(ask), host.fetch_original(ask)), ask
        assert torch.equal(devs.fetch(ask), host.fetch(ask)), ask
    # through the read-ahead: staged on the copy stream by a background thread, fetched with the same ids
    for s in (host, devs):
        s.stage_ahead([1, 2, 3])
    a, b = devs.fetch([1, 2, 3]), host.fetch([1, 2, 3])
    assert devs.ahead_hits == 1 and host.ahead_hits == 1 and torch.equal(a, b)
    devs.stage_ahead([0, 1])
    assert torch.equal(devs.fetch([4, 5]), host.fetch([4, 5]))      # a fetch of anything else drops the staged batch
    # a batch of 8 or more goes up in chunks, each reconstructed behind its copy
    long = [i % n for i in range(11)]
    assert torch.equal(devs.fetch_original(long), host.fetch_original(long))
    # mirrored views
    flip = {m: feed.FrameSource(pattern, "%06d", n, dev, workers=2, decode=m, hflip=True, **size) for m in ("host", "device")}
    assert torch.equal(flip["device"].fetch(ids), flip["host"].fetch(ids))
    assert torch.equal(flip["device"].fetch(ids), torch.flip(devs.fetch(ids), dims=[2]))
    for s in list(srcs.values()) + list(flip.values()):
        s.close()
    return devs


def test_frame_source_device_decode_equals_host_decode(dev, tmp_path):
    pattern = _jpeg_folder(tmp_path, 6)
    devs = _compare_sources(dev, pattern, 6, min_size=90, max_size=160)
    assert devs.decode_mode == "device" and devs.host_fallbacks == 0 and devs.jpeg_info.sampling == jpeg.S420
    assert devs.in_hw == (67, 45) and devs.out_hw != devs.in_hw
    same = _compare_sources(dev, pattern, 6, min_size=45, max_size=67)      # no resize: the decoded frames themselves
    assert same.out_hw == same.in_hw == (67, 45)


def test_refused_frames_fall_back_to_the_host_one_by_one(dev, tmp_path):
    pattern = _jpeg_folder(tmp_path, 6, special={3: (2, {"progressive": True}), 4: (0, {})})
    devs = _compare_sources(dev, pattern, 6, min_size=90, max_size=160)
    assert devs.decode_mode == "device" and devs.host_fallbacks == 2 and sorted(devs._fallback_ids) == [3, 4]


def test_a_frame_of_another_size_raises_as_on_the_host_path(dev, tmp_path):
    pattern = _jpeg_folder(tmp_path, 3)
    (tmp_path / "000002.JPEG").write_bytes(jpeg_cases.encode(jpeg_cases.picture(33, 50, 1), 2, 90))
    for mode in ("host", "device"):
        src = feed.FrameSource(pattern, "%06d", 3, dev, workers=2, decode=mode)
        assert src.decode_mode == mode
        with pytest.raises(ValueError, match="the video started as"):
            src.fetch([0, 1, 2])
        src.close()


def test_a_png_folder_becomes_a_host_source(dev, tmp_path):
    pattern = _jpeg_folder(tmp_path, 3, suffix="png")
    src = feed.FrameSource(pattern, "%06d", 3, dev, workers=2, decode="device")
    ref = feed.FrameSource(pattern, "%06d", 3, dev, workers=2)
    assert src.decode_mode == "host" and src.jpeg_info is None and src.host_fallbacks == 0
    assert torch.equal(src.fetch([0, 1, 2]), ref.fetch([0, 1, 2]))
    src.close()
    ref.close()


def test_detections_do_not_depend_on_the_decode_mode(dev, tmp_path):
    """compute_on_dataset on a 6-frame JPEG video with the single-frame R-50 detector at a small MIN_SIZE_TEST"""
    from mega.pytorch_amd import config, inference, modeling, synth
    import mega.pytorch_amd.fgfa  # noqa: F401
    L, H0, W0 = 6, 90, 160
    clip = synth.make_clip(L, H0, W0, seed=9).numpy()
    os.makedirs(str(tmp_path / "Data" / "v"))
    for t in range(L):
        (tmp_path / "Data" / "v" / ("%06d.JPEG" % t)).write_bytes(jpeg_cases.encode(clip[t], 2, 92))
    (tmp_path / "index.txt").write_text("".join("v %d %d %d\n" % (t + 1, t, L) for t in range(L)))
    cfg = config.get_cfg("R-50", "base")
    cfg.MODEL.DEVICE = str(dev)
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 180, 320
    sd = {k: v for k, v in synth.make_fgfa_state_dict(seed=3).items() if not k.startswith(("flownet.", "embednet."))}
    model = modeling.build_detection_model(cfg)
    model.load_state_dict(sd)
    model.to(dev)
    index = inference.VIDTestIndex(str(tmp_path / "index.txt"))
    res = {m: inference.compute_on_dataset(model, index, str(tmp_path / "Data"), dev, steps_per_batch=4, decode=m)
           for m in ("host", "device")}
    assert sorted(res["host"]) == sorted(res["device"]) == list(range(L)) and sum(len(p) for p in res["host"].values()) > 0
    for i in range(L):
        a, b = res["host"][i], res["device"][i]
        assert a.size == b.size and torch.equal(a.bbox, b.bbox)
        assert torch.equal(a.get_field("scores"), b.get_field("scores")) and torch.equal(a.get_field("labels"), b.get_field("labels"))
    with pytest.raises(ValueError, match="decode"):
        inference.compute_on_dataset(model, index, str(tmp_path / "Data"), dev, decode="gpu")
