"""Times the two JPEG decode modes of the frame feed (mega.pytorch_amd.feed.FrameSource, decode="host" | "device") on 64
synthetic 720 x 1280 frames (synth.make_clip), encoded in memory at quality 90, 4:2:0.

  python tools/bench_feed.py [--frames 64] [--workers 16] [--repeats 3] [--batch 16] [--out profiles/jpeg_feed.json]

One JSON line (also written to --out):
  host, one thread    ms per frame of a full Pillow decode (Image.open(...).convert("RGB") to a numpy array) and of the entropy
                      decode alone (mega_jpeg_entropy_decode into a re-used int16 buffer): best of the repeats
  host, --workers     frames/s of each on a thread pool (both release the GIL)
  device              time per frame of mega_jpeg_reconstruct's two launches on the whole batch, HIP events around the entry
                      point, and beside it the device time of a plain device-to-device copy of the same coefficient bytes
                      and of their pinned host-to-device copy
  feed                frames/s of FrameSource.fetch over the whole folder in batches of --batch, resize included, in both
                      modes (a fresh source per repeat, so every frame is decoded every time), and whether both gave the same
                      bytes
No ratio is fixed in advance: the comparison is the Pillow path in the same run.  Real ImageNet VID JPEGs are not available
where this runs; the frames are synthetic, and camera footage has other coefficient statistics and file sizes.
"""
import argparse
import io
import json
import os
import platform
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _best(fn, repeats):
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args(argv)
    import PIL
    import torch
    from PIL import Image
    from mega.pytorch_amd import _lib, feed, jpeg, ops, synth
    _lib.load()
    dev = torch.device("cuda:0")
    T, H, W = a.frames, a.height, a.width
    clip = synth.make_clip(T, H, W, seed=5).numpy()
    datas = []
    for t in range(T):
        b = io.BytesIO()
        Image.fromarray(clip[t]).save(b, "JPEG", quality=a.quality, subsampling=2)
        datas.append(b.getvalue())
    info = jpeg.probe(datas[0])
    assert info.sampling == jpeg.S420 and info.hw == (H, W)

    def pillow(i):
        return np.asarray(Image.open(io.BytesIO(datas[i])).convert("RGB"))

    bufs = [np.empty(info.stride, dtype=np.int16) for _ in range(T)]

    def entropy(i):
        return ops.jpeg_entropy_decode(datas[i], info, bufs[i])

    res = {"metric": "jpeg_feed", "command": " ".join(["python", "tools/bench_feed.py"] + list(sys.argv[1:] if argv is None else argv)),
           "frames": T, "height": H, "width": W, "quality": a.quality, "sampling": "4:2:0",
           "mean_jpeg_bytes": int(np.mean([len(d) for d in datas])), "coefficient_bytes_per_frame": info.stride * 2,
           "rgb_bytes_per_frame": H * W * 3, "workers": a.workers, "batch": a.batch, "repeats": a.repeats,
           "pillow": PIL.__version__, "host": platform.node(), "cpus_usable": len(os.sched_getaffinity(0)),
           "device": torch.cuda.get_device_name(0)}
    # ---- host, one thread
    res["pillow_decode_ms_per_frame_1_thread"] = round(_best(lambda: [pillow(i) for i in range(T)], a.repeats) / T * 1e3, 3)
    res["entropy_decode_ms_per_frame_1_thread"] = round(_best(lambda: [entropy(i) for i in range(T)], a.repeats) / T * 1e3, 3)
    # ---- host, thread pool
    with ThreadPoolExecutor(max_workers=a.workers) as pool:
        rounds = 4
        ids = list(range(T)) * rounds
        res["pillow_decode_fps_%d_workers" % a.workers] = round(len(ids) / _best(lambda: list(pool.map(pillow, ids)), a.repeats), 1)
        res["entropy_decode_fps_%d_workers" % a.workers] = round(len(ids) / _best(lambda: list(pool.map(entropy, ids)), a.repeats), 1)
    # ---- device
    stage = torch.empty((T, info.stride), dtype=torch.int16).pin_memory()
    for i in range(T):
        stage[i].numpy()[:] = bufs[i]
    coef = stage.to(dev)
    out = torch.empty((T, H, W, 3), dtype=torch.uint8, device=dev)
    other = torch.empty_like(coef)

    def device_ms(fn):
        fn()
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(max(a.repeats, 5)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1))
        return best
    nb = _lib.load().mega_jpeg_reconstruct_workspace_bytes(T, H, W, info.sampling)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)

    def reconstruct():      # the entry point itself: workspace and output allocated once, outside the events
        ops._call("mega_jpeg_reconstruct", coef, info.stride, T, H, W, info.sampling, out, ws, nb)
    res["reconstruct_device_ms_per_frame"] = round(device_ms(reconstruct) / T, 4)
    res["d2d_copy_of_coefficients_device_ms_per_frame"] = round(device_ms(lambda: other.copy_(coef)) / T, 4)
    res["h2d_copy_of_coefficients_ms_per_frame"] = round(device_ms(lambda: other.copy_(stage, non_blocking=True)) / T, 4)
    same = all(np.array_equal(out[i].cpu().numpy(), pillow(i)) for i in (0, T // 2, T - 1))
    res["reconstruct_equals_pillow"] = bool(same)
    # ---- the feed
    with tempfile.TemporaryDirectory() as td:
        for t in range(T):
            with open(os.path.join(td, "%06d.JPEG" % t), "wb") as f:
                f.write(datas[t])
        pattern = os.path.join(td, "%s.JPEG")
        batches = [list(range(o, min(o + a.batch, T))) for o in range(0, T, a.batch)]
        sums = {}
        for mode in ("host", "device"):
            def run():
                src = feed.FrameSource(pattern, "%06d", T, dev, workers=a.workers, cache_frames=T, decode=mode)
                src.prefetch(range(T))
                acc = 0
                for ids in batches:
                    acc += int(src.fetch(ids).sum(dtype=torch.int64))      # (the sum also waits for the batch)
                torch.cuda.synchronize()
                sums[mode] = (acc, src.decode_mode, src.host_fallbacks)
                src.close()
            run()      # warm-up: page-locks nothing that survives, but loads the kernels and the resize tables' code
            res["fetch_fps_%s" % mode] = round(T / _best(run, a.repeats), 1)
        res["fetch_modes_agree"] = bool(sums["host"][0] == sums["device"][0])
        res["fetch_device_mode"], res["fetch_host_fallbacks"] = sums["device"][1], sums["device"][2]
    res["entropy_decode_faster_than_pillow_per_frame"] = bool(
        res["entropy_decode_ms_per_frame_1_thread"] < res["pillow_decode_ms_per_frame_1_thread"])
    res["not_measured"] = ("real ImageNet VID JPEGs: they are not available where this ran; the frames are synthetic "
                           "(synth.make_clip), and camera footage has other coefficient statistics and file sizes; the "
                           "spread between machines; a run with the engines consuming the frames")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
