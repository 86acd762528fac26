"""Times the demo (mega.pytorch_amd.demo) on synthetic frames with a fixed seeded detection set.  One JSON line:

  render_ms_per_frame      ops.overlay_detections (selection + drawing) on 720 x 1280 frames resized from 562 x 1000, 300
                           detection rows per frame of which 0, 8 and 300 are kept (device events around --repeats calls
                           on --frames frames, after a warm-up), and select_ms_per_frame: the selection pass alone
  twin_ms_per_frame        the numpy twin (tests/overlay_twin.py) on the same inputs, on the host
  demo / detector wall     VIDDemo.run_on_image_folder (detect, render, JPEG encode and write) against plain
                           inference.compute_on_dataset on the same synthetic folder (--video-frames frames of
                           --video-hw), wall time per frame, R-50 seeded weights, bfloat16
  python tools/bench_demo.py [--method mega] [--frames 16] [--repeats 20] [--video-frames 120] [--skip-video]
Kernel times by name: run it under  rocprofv3 --kernel-trace --stats -- python tools/bench_demo.py --skip-video
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HW, RHW, ROWS = (720, 1280), (562, 1000), 300


def detection_set(seed, F, kept, thr=0.7):
    """[F,300,...] detections in the 562 x 1000 frame: `kept` rows per frame score above thr, the rest below"""
    rng = np.random.default_rng(seed)
    ctr = rng.uniform([0, 0], [RHW[1], RHW[0]], (F, ROWS, 2))
    wh = rng.uniform(20, [0.5 * RHW[1], 0.5 * RHW[0]], (F, ROWS, 2))
    box = np.concatenate([ctr - wh / 2, ctr + wh / 2], 2).clip(0, [RHW[1] - 1, RHW[0] - 1] * 2).astype(np.float32)
    score = rng.uniform(0.001, thr - 0.01, (F, ROWS)).astype(np.float32)
    score[:, :kept] = rng.uniform(thr + 0.01, 1.0, (F, kept)).astype(np.float32)
    label = rng.integers(1, 31, (F, ROWS)).astype(np.int64)
    return box, score, label, np.full(F, ROWS, np.int32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--method", default="mega", choices=["mega", "base"])
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--video-frames", type=int, default=120)
    ap.add_argument("--video-hw", type=int, nargs=2, default=[360, 640])
    ap.add_argument("--skip-video", action="store_true")
    a = ap.parse_args(argv)
    import torch
    import overlay_twin as tw
    from mega.pytorch_amd import config, demo, inference, modeling, ops, synth
    if not torch.cuda.is_available():
        sys.exit("bench_demo.py needs a HIP device")
    dev = torch.device("cuda:0")
    atlas = demo.LabelAtlas(*demo.glyph_atlas(16))
    pal = demo.class_palette(31)
    d_atlas, d_pal = atlas.to(dev), torch.from_numpy(pal).to(dev)
    F = a.frames
    frames = np.random.default_rng(0).integers(0, 256, (F,) + HW + (3,)).astype(np.uint8)
    res = {"metric": "demo_overlay", "frame_hw": list(HW), "resized_hw": list(RHW), "rows_per_frame": ROWS, "frames": F,
           "repeats": a.repeats, "render_ms_per_frame": {}, "select_ms_per_frame": {}, "twin_ms_per_frame": {}}
    for kept in (0, 8, 300):
        box, score, label, counts = detection_set(kept, F, kept)
        t = [torch.from_numpy(x).to(dev) for x in (box, score, label, counts)]
        d_frames = torch.from_numpy(frames).to(dev)
        for select_only in (False, True):
            for _ in range(3):
                ops.overlay_detections(d_frames, *t, RHW, 0.7, 1, d_pal, d_atlas, select_only=select_only)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.repeats):
                ops.overlay_detections(d_frames, *t, RHW, 0.7, 1, d_pal, d_atlas, select_only=select_only)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.repeats / F
            res["select_ms_per_frame" if select_only else "render_ms_per_frame"][str(kept)] = round(ms, 5)
        n = min(F, 2)
        t0 = time.perf_counter()
        want = tw.draw_batch(frames[:n], box[:n], score[:n], label[:n], counts[:n], RHW, 0.7, 1, pal, atlas, demo.CATEGORIES)
        res["twin_ms_per_frame"][str(kept)] = round((time.perf_counter() - t0) * 1e3 / n, 3)
        assert np.array_equal(d_frames[:n].cpu().numpy(), want), "kernel and twin differ"
    if not a.skip_video:
        from PIL import Image
        L, (H0, W0) = a.video_frames, a.video_hw
        cfg = config.get_cfg("R-50", a.method)
        cfg.DTYPE = "bfloat16"
        cfg.MODEL.DEVICE = "cuda:0"
        if a.method == "mega":
            sd = synth.make_state_dict(blocks=(3, 4, 6), reduce_channel=True, global_res_stage=0, seed=1)
        else:
            sd = {k: v for k, v in synth.make_fgfa_state_dict(seed=3).items() if not k.startswith(("flownet.", "embednet."))}
        model = modeling.build_detection_model(cfg)
        model.load_state_dict(sd)
        model.to(dev)
        with tempfile.TemporaryDirectory() as td:
            os.makedirs(os.path.join(td, "Data", "v"))
            clip = synth.make_clip(L, H0, W0, seed=2).numpy()
            lines = []
            for i in range(L):
                Image.fromarray(clip[i]).save(os.path.join(td, "Data", "v", "%06d.JPEG" % i), format="JPEG", quality=92)
                lines.append("v %d %d %d" % (i + 1, i, L))
            with open(os.path.join(td, "index.txt"), "w") as f:
                f.write("\n".join(lines) + "\n")
            index = inference.VIDTestIndex(os.path.join(td, "index.txt"))
            preds = inference.compute_on_dataset(model, index, os.path.join(td, "Data"), dev)      # warm-up: graphs, plans
            best = sorted(float(p.get_field("scores").max()) for p in preds.values() if len(p))
            thr = best[len(best) // 4] if best else 0.7       # three quarters of the frames draw something
            vd = demo.VIDDemo(cfg, model, confidence_threshold=thr, output_folder=os.path.join(td, "out"))
            vd.run_on_image_folder(os.path.join(td, "Data", "v"))                                   # warm-up
            wall = {"detector": [], "demo": [], "demo_no_files": []}
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                inference.compute_on_dataset(model, index, os.path.join(td, "Data"), dev)
                wall["detector"].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                vd.run_on_image_folder(os.path.join(td, "Data", "v"))
                wall["demo"].append(time.perf_counter() - t0)
                vd.output_folder = None
                t0 = time.perf_counter()
                vd.run_on_image_folder(os.path.join(td, "Data", "v"))
                wall["demo_no_files"].append(time.perf_counter() - t0)
                vd.output_folder = os.path.join(td, "out")
            res.update({"video": {"method": a.method, "frames": L, "hw": [H0, W0], "dtype": "bfloat16",
                                  "threshold": round(thr, 6),
                                  "detector_wall_ms_per_frame": round(float(np.median(wall["detector"])) * 1e3 / L, 3),
                                  "demo_wall_ms_per_frame": round(float(np.median(wall["demo"])) * 1e3 / L, 3),
                                  "demo_without_jpeg_ms_per_frame": round(float(np.median(wall["demo_no_files"])) * 1e3 / L, 3)}})
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
