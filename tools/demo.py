"""Run a detector on a folder of frames and write the annotated frames (mega.pytorch_amd.demo.VIDDemo; the reference's
demo/demo.py).

  python tools/demo.py mega --arch R-101 --weights MEGA_R_101.pth --image-folder <frames> --output-folder <out>
      the sorted "*<suffix>" files of the folder as one video -> <out>/000000.jpg ...; one JSON line with the timings.
  python tools/demo.py mega --dtype bfloat16 --f8-scales scales.json ...
      the same with layer3's identity blocks in FP8 (cfg.FP8_CONV), the scales from tools/calibrate_f8.py.
  python tools/demo.py mega --dry-run
      parses the arguments and prints the resolved settings as one JSON line; no device code is imported.
Video files (the reference's --video / --output-video) are out of scope: no codec library is a dependency.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("method", choices=["base", "dff", "fgfa", "rdn", "mega"], help="which method to use")
    ap.add_argument("--arch", choices=["R-50", "R-101"], default="R-101")
    ap.add_argument("--weights", default=None, help="checkpoint of the detector (torch .pth or Caffe2 .pkl)")
    ap.add_argument("--flownet-weights", default=None, help="fgfa / dff: the FlowNet checkpoint loaded after --weights")
    ap.add_argument("--image-folder", default="datasets/ILSVRC2015/Data/VID/val/ILSVRC2015_val_00003001")
    ap.add_argument("--suffix", default=".JPEG", help="the suffix of the images in the image folder")
    ap.add_argument("--output-folder", default=None, help="default: demo/visualization/<method>")
    ap.add_argument("--threshold", type=float, default=0.7, help="draw detections with score > threshold")
    ap.add_argument("--thickness", type=int, default=1, help="outline thickness in pixels (odd)")
    ap.add_argument("--dtype", choices=["float32", "bfloat16", "float16"], default="float32")
    ap.add_argument("--f8-scales", default=None, metavar="FILE", help="run layer3's identity blocks in FP8 (cfg.FP8_CONV "
                    "'layer3'; --dtype bfloat16) with the calibrated scales of this JSON file (tools/calibrate_f8.py)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--decode", choices=["host", "device"], default="host", help="device: entropy-decode the JPEGs on the "
                    "host threads and run the pixel stages (IDCT, upsampling, colour) in HIP; same frames bit for bit")
    ap.add_argument("--dry-run", action="store_true", help="print the resolved settings as one JSON line and stop")
    a = ap.parse_args(argv)
    if a.thickness < 1 or a.thickness % 2 == 0:
        ap.error("--thickness must be odd")
    if a.output_folder is None:
        a.output_folder = os.path.join("demo", "visualization", a.method)
    return a


def main(argv=None):
    a = parse(argv)
    settings = {"method": a.method, "arch": a.arch, "weights": a.weights, "flownet_weights": a.flownet_weights,
                "image_folder": a.image_folder, "suffix": a.suffix, "output_folder": a.output_folder,
                "threshold": a.threshold, "thickness": a.thickness, "dtype": a.dtype, "device": a.device,
                "f8_scales": a.f8_scales, "decode": a.decode}
    if a.dry_run:
        print(json.dumps(dict(settings, dry_run=True)))
        return 0
    sys.path.insert(0, ROOT)
    import torch
    from mega.pytorch_amd import checkpoint, config, demo, f8, modeling
    if not torch.cuda.is_available():
        sys.exit("tools/demo.py needs a HIP device (the detector has no CPU fallback)")
    cfg = config.get_cfg(a.arch, a.method)
    cfg.DTYPE = a.dtype
    cfg.MODEL.DEVICE = a.device
    if a.f8_scales:
        cfg.FP8_CONV = "layer3"
    model = modeling.build_detection_model(cfg)
    if a.f8_scales:
        f8.load_scales(model, a.f8_scales)
    if a.weights:
        checkpoint.load_checkpoint(cfg, model, a.weights)
    if a.flownet_weights:
        checkpoint.load_checkpoint(cfg, model, a.flownet_weights, flownet=True)
    model.to(torch.device(a.device))
    d = demo.VIDDemo(cfg, model, confidence_threshold=a.threshold, thickness=a.thickness, output_folder=a.output_folder,
                      decode=a.decode)
    frames = d.run_on_image_folder(a.image_folder, suffix=a.suffix)
    print(json.dumps(dict(settings, frames=len(frames), detections=sum(len(p) for p in d.predictions),
                          detect_s=round(d.timer["detect_s"], 3), total_s=round(d.timer["total_s"], 3))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
