"""Calibrate the FP8 activation scales of a detector built with cfg.FP8_CONV "layer3" (mega/pytorch_amd/f8.py) on a folder of
frames and write them as a JSON file of numbers keyed by module name -- what `tools/demo.py --f8-scales FILE` and
inference(..., f8_scales=FILE) read.

  python tools/calibrate_f8.py mega --arch R-101 --weights MEGA_R_101.pth --image-folder <frames> --out scales.json
      the sorted "*<suffix>" files of the folder (at most --max-frames, evenly spaced), resized as at test time, through the
      bf16 backbone; every FP8 block's scale = absmax / 448 of its input and of its conv1 output over those frames.
  python tools/calibrate_f8.py mega --dry-run
      parses the arguments and prints the resolved settings as one JSON line; no device code is imported.
Percentile and other clipping policies are out of scope.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("method", nargs="?", default="mega", choices=["base", "dff", "fgfa", "rdn", "mega"])
    ap.add_argument("--arch", choices=["R-50", "R-101"], default="R-101")
    ap.add_argument("--weights", default=None, help="checkpoint of the detector (torch .pth or Caffe2 .pkl)")
    ap.add_argument("--image-folder", default="datasets/ILSVRC2015/Data/VID/val/ILSVRC2015_val_00003001")
    ap.add_argument("--suffix", default=".JPEG")
    ap.add_argument("--max-frames", type=int, default=32, help="frames used, evenly spaced over the folder")
    ap.add_argument("--batch", type=int, default=8, help="frames per backbone pass")
    ap.add_argument("--out", default="scales.json")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--decode", choices=["host", "device"], default="host", help="device: the JPEG pixel stages run in HIP")
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args(argv)
    if a.max_frames < 1 or a.batch < 1:
        ap.error("--max-frames and --batch must be positive")
    return a


def main(argv=None):
    a = parse(argv)
    settings = {"method": a.method, "arch": a.arch, "weights": a.weights, "image_folder": a.image_folder, "suffix": a.suffix,
                "max_frames": a.max_frames, "batch": a.batch, "out": a.out, "device": a.device,
                "decode": a.decode}
    if a.dry_run:
        print(json.dumps(dict(settings, dry_run=True)))
        return 0
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from PIL import Image
    from mega.pytorch_amd import checkpoint, config, demo, f8, feed, modeling
    if not torch.cuda.is_available():
        sys.exit("tools/calibrate_f8.py needs a HIP device (the backbone has no CPU fallback)")
    cfg = config.get_cfg(a.arch, a.method)
    cfg.DTYPE, cfg.FP8_CONV = "bfloat16", "layer3"
    cfg.MODEL.DEVICE = a.device
    model = modeling.build_detection_model(cfg)
    if a.weights:
        checkpoint.load_checkpoint(cfg, model, a.weights)
    dev = torch.device(a.device)
    model.to(dev)
    files = demo.VIDDemo.list_frames(a.image_folder, a.suffix)
    n = min(a.max_frames, len(files))
    ids = sorted({int(round(i * (len(files) - 1) / max(n - 1, 1))) for i in range(n)})
    def reader(i):
        with open(files[i], "rb") as f:
            return f.read()
    how = (dict(decode="device", reader=reader) if a.decode == "device"
           else dict(opener=lambda i: np.asarray(Image.open(files[i]).convert("RGB"))))
    src = feed.FrameSource(os.path.join(a.image_folder, "%s"), "%s", len(files), dev, min_size=cfg.INPUT.MIN_SIZE_TEST,
                           max_size=cfg.INPUT.MAX_SIZE_TEST, **how)
    try:
        batches = [src.fetch(ids[o:o + a.batch]).clone() for o in range(0, len(ids), a.batch)]
    finally:
        src.close()
    scales = f8.calibrate(model, batches)
    with open(a.out, "w") as f:
        json.dump(scales, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(dict(settings, frames=len(ids), blocks=len(scales),
                          in_scale_max=max(v["in"] for v in scales.values()), mid_scale_max=max(v["mid"] for v in scales.values()))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
