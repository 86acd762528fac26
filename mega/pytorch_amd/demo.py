"""The demo: run a detector on a folder of frames and draw what it finds.

Mirror of  demo/predictor.py:300-640  VIDDemo  (run_on_image_folder, select_top_predictions, overlay_boxes,
                                               overlay_class_names, generate_images)
re-designed for a GPU whose detector needs ~1 ms per key frame: the detections never leave the device before the picture
is finished.  The video goes through the engine of the test loop (inference._video_runner); the ORIGINAL-size uint8
frames are uploaded again chunk by chunk (feed.FrameSource.fetch_original), one kernel pair draws a chunk's detections
in place (ops.overlay_detections, csrc/overlay.hip), and one D2H copy per chunk brings the finished pictures back.

What is kept of the reference's picture: score > threshold (0.7, strict), drawn in descending score order, boxes rescaled
to the original frame as BoxList.resize does (one f32 multiply) and truncated to integers, one colour per class, a
"<name>: 0.93" label at the box's top-left corner, `%06d.jpg` outputs.  What differs: the rasterisation.  cv2 is not a
dependency, so there is no Hershey font; the picture is DEFINED here and implemented twice (the kernel and the numpy twin
tests/overlay_twin.py, bit for bit):

  draw list  rows with score > thr, score descending, equal scores by ascending row; box = trunc(x * f32(W / Wr)),
             trunc(y * f32(H / Hr)) (clamped to +-2^30); rows whose box is degenerate (x1 < x0 or y1 < y0), lies wholly
             outside the image, or whose class is outside the palette are dropped, label included.
  outlines   all of them first, in draw order (a later one overwrites): thickness t odd, the pixels whose Chebyshev
             distance to the 1-pixel rectangle {x in {x0,x1}, y0<=y<=y1} U {y in {y0,y1}, x0<=x<=x1} is <= (t-1)/2,
             in the class colour, clipped to the image.
  labels     then all labels in draw order, on top of every outline: text "<name>: D.DD", D.DD the digits of
             "%.2f" % score (scores in [0, 1]; larger ones print as 9.99).  Glyph k of the text occupies adv[k] columns;
             the rectangle is sum(adv) wide and gh high, rows [y0 - gh, y0) (if y0 - gh < 0: rows from max(y0, 0)),
             columns from max(min(x0, W - width), 0), clipped to the image.  Every pixel of it is the class colour c
             blended with white by the glyph coverage a: (c * (255 - a) + 255 * a + 127) // 255  (a = 0 beyond the
             glyph cell).
The glyph atlas is rasterised at run time from Pillow's built-in default font (no font file is shipped); kernel and twin
take it as an input.  Colours are RGB (frames are decoded by Pillow), not cv2's BGR.  Video files are out of scope.
"""
import colorsys
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import feed, vid_eval

CATEGORIES = vid_eval.CLASSES            # index = label; 0 is the background
CHARSET = "abcdefghijklmnopqrstuvwxyz0123456789:._ "
JPEG_QUALITY = 95                        # cv2.imwrite's default
MAX_NAME = 18                            # glyphs of a class name the kernel keeps (csrc/overlay.hip OV_MAX_NAME)


def glyph_atlas(height=16, chars=CHARSET):
    """Rasterise `chars` with Pillow's built-in default font at pixel size `height` -> (cells u8 [G,gh,gw] coverage,
    advances i32 [G], chars).  gh is the font's line height (ascent + descent), gw the largest advance; a glyph is drawn
    at the left of its cell and shows its first adv columns."""
    from PIL import Image, ImageDraw, ImageFont
    try:
        font = ImageFont.load_default(size=height)
    except TypeError:                    # a Pillow whose default font is the fixed bitmap font
        font = ImageFont.load_default()
    adv = [max(1, int(np.ceil(font.getlength(c)))) for c in chars]
    if hasattr(font, "getmetrics"):
        gh = int(sum(font.getmetrics()))
    else:
        gh = int(font.getbbox(chars)[3])
    gh, gw = max(gh, 1), max(adv)
    cells = np.zeros((len(chars), gh, gw), np.uint8)
    for i, c in enumerate(chars):
        im = Image.new("L", (gw, gh), 0)
        ImageDraw.Draw(im).text((0, 0), c, font=font, fill=255)
        cells[i] = np.asarray(im)
    return cells, np.asarray(adv, np.int32), chars


def class_palette(num_classes):
    """u8 [num_classes,3] RGB: fixed, visibly distinct colours (golden-ratio hue steps, two brightness levels); entry 0,
    the background, is never drawn."""
    pal = np.zeros((num_classes, 3), np.uint8)
    for i in range(1, num_classes):
        r, g, b = colorsys.hsv_to_rgb((i * 0.6180339887498949) % 1.0, 0.85, 0.95 if i % 2 else 0.70)
        pal[i] = (int(round(r * 255)), int(round(g * 255)), int(round(b * 255)))
    return pal


class LabelAtlas(object):
    """What the overlay needs to write labels: cells [G,gh,gw] u8, advances [G] i32, class_glyphs [NC,ML] i32 (the glyphs
    of each class name, -1 after its end), fmt_glyphs [13] i32 (the glyphs of '0'..'9', ':', ' ', '.').  Built from
    numpy arrays; to(device) gives the same object over torch tensors."""

    def __init__(self, cells, advances, chars, categories=CATEGORIES):
        index = {c: i for i, c in enumerate(chars)}
        for name in list(categories) + ["0123456789: ."]:
            for c in name:
                if c not in index:
                    raise ValueError("glyph atlas has no cell for %r (needed by %r)" % (c, name))
        if max(len(n) for n in categories) > MAX_NAME:
            raise ValueError("a class name is longer than %d characters" % MAX_NAME)
        ml = max(1, max(len(n) for n in categories))
        table = np.full((len(categories), ml), -1, np.int32)
        for k, name in enumerate(categories):
            table[k, :len(name)] = [index[c] for c in name]
        self.cells = np.ascontiguousarray(cells, np.uint8)
        self.advances = np.ascontiguousarray(advances, np.int32)
        self.class_glyphs = table
        self.fmt_glyphs = np.asarray([index[c] for c in "0123456789: ."], np.int32)
        self.chars = chars
        if self.cells.ndim != 3 or self.advances.shape != (self.cells.shape[0],) or len(chars) != self.cells.shape[0]:
            raise ValueError("glyph atlas: cells [G,gh,gw], advances [G] and chars must agree")
        if (self.advances < 1).any() or (self.advances > self.cells.shape[2]).any():
            raise ValueError("glyph atlas: advances must lie in [1, cell width]")

    def to(self, device):
        out = object.__new__(LabelAtlas)
        out.chars = self.chars
        for k in ("cells", "advances", "class_glyphs", "fmt_glyphs"):
            v = getattr(self, k)
            setattr(out, k, (torch.from_numpy(v) if isinstance(v, np.ndarray) else v).to(device))
        return out


def encode_jpeg(path, frame):
    from PIL import Image
    Image.fromarray(frame).save(path, format="JPEG", quality=JPEG_QUALITY)


class VIDDemo(object):
    """predictor.py:300-640.  cfg.MODEL.VID.METHOD selects the detector (mega, rdn, fgfa, dff, base), each through the
    engine compute_on_dataset uses.  model: a built detector with its weights loaded (None: build_detection_model(cfg),
    weights as initialised).  runner / overlay replace the engine and ops.overlay_detections (tests without a device).
    With cfg.TEST.SOFT_NMS or cfg.TEST.BBOX_VOTE on, the folder runs as compute_on_dataset runs a video with them: the
    box head in candidate mode, the identity view (or the TEST.BBOX_AUG views, if enabled too) through the runner, then
    soft_nms.py's filter; this needs the model (its post-processor holds the thresholds), also beside a runner."""

    CATEGORIES = CATEGORIES

    def __init__(self, cfg, model=None, confidence_threshold=0.7, thickness=1, output_folder=None, steps_per_batch=10,
                 engine_kwargs=None, source_kwargs=None, seed=0, render_chunk=16, glyph_height=16, runner=None,
                 overlay=None, decode="host"):
        if int(thickness) < 1 or int(thickness) % 2 == 0:
            raise ValueError("thickness must be odd, got %r" % (thickness,))
        self.cfg = cfg
        self.method = cfg.MODEL.VID.METHOD
        self.device = torch.device(cfg.MODEL.DEVICE)
        self.confidence_threshold = float(confidence_threshold)
        self.thickness = int(thickness)
        self.output_folder = output_folder
        self.render_chunk = int(render_chunk)
        self.source_kwargs = dict(source_kwargs or {})
        if decode not in ("host", "device"):
            raise ValueError('decode must be "host" or "device", got %r' % (decode,))
        self.decode = decode      # "device": the frames' JPEG pixel stages run in HIP (feed.FrameSource, jpeg.py)
        from .soft_nms import enabled_filter
        self.final = enabled_filter(cfg)        # (ValueError for a bad value, before any device work)
        if self.final is not None and model is None and runner is not None:
            raise ValueError("TEST.SOFT_NMS / TEST.BBOX_VOTE need the model beside a runner (candidate mode)")
        if runner is None:
            from . import inference
            if model is None:
                from .modeling import build_detection_model
                model = build_detection_model(cfg)
                model.to(self.device)
            model.eval()
            runner = inference._video_runner(model, steps_per_batch, seed, engine_kwargs)
        self.model = model
        self.runner = runner
        if overlay is None:
            from . import ops
            overlay = ops.overlay_detections
        self.overlay = overlay
        self.atlas = LabelAtlas(*glyph_atlas(glyph_height), categories=self.CATEGORIES)
        self.palette = class_palette(len(self.CATEGORIES))
        self._dev_atlas = self._dev_palette = None
        self.predictions = None
        self.timer = {}

    # ------------------------------------------------------------------------------------------ input
    @staticmethod
    def list_frames(folder, suffix=".JPEG"):
        if not os.path.isdir(folder):
            raise FileNotFoundError('folder "%s" does not exist' % folder)
        files = sorted(f for f in os.listdir(folder) if f.endswith(suffix))
        if not files:
            raise FileNotFoundError('no "*%s" files in "%s"' % (suffix, folder))
        return [os.path.join(folder, f) for f in files]

    def _source(self, files, min_size=None, max_size=None, hflip=False):
        from PIL import Image

        def opener(i):
            return np.asarray(Image.open(files[i]).convert("RGB"))

        def reader(i):
            with open(files[i], "rb") as f:
                return f.read()
        how = dict(decode="device", reader=reader) if self.decode == "device" else dict(opener=opener)
        how.update(self.source_kwargs)
        return feed.FrameSource(os.path.join(os.path.dirname(files[0]), "%s"), "%s", len(files), self.device,
                                min_size=self.cfg.INPUT.MIN_SIZE_TEST if min_size is None else min_size,
                                max_size=self.cfg.INPUT.MAX_SIZE_TEST if max_size is None else max_size,
                                hflip=hflip, **how)

    def _detect(self, src, files):
        v = {"start": 0, "pattern": "%s", "seg_len": len(files)}
        if self.final is None:
            return self.runner(src, v)
        from . import bbox_aug
        aug = getattr(getattr(self.cfg, "TEST", None), "BBOX_AUG", None)
        aug_cfg = self.cfg if aug is not None and aug.ENABLED else None
        return bbox_aug.run_video(self.model, self.runner, v, src, lambda mn, mx, hf: self._source(files, mn, mx, hf),
                                  aug_cfg=aug_cfg, final=self.final)

    # ------------------------------------------------------------------------------------------ render
    def _render_chunk(self, src, dets, ids):
        """the annotated original frames `ids` on the device; everything here is enqueued, nothing synchronises"""
        frames = src.fetch_original(ids)
        chunk = [dets[i] for i in ids]
        R = max(len(d) for d in chunk)
        if R == 0:
            return frames
        if self._dev_atlas is None:
            self._dev_atlas = self.atlas.to(self.device)
            self._dev_palette = torch.from_numpy(self.palette).to(self.device)
        pad = torch.nn.utils.rnn.pad_sequence
        boxes = pad([d.bbox.reshape(-1, 4) for d in chunk], batch_first=True).contiguous()
        scores = pad([d.get_field("scores").reshape(-1).to(torch.float32) for d in chunk], batch_first=True).contiguous()
        labels = pad([d.get_field("labels").reshape(-1) for d in chunk], batch_first=True).contiguous()
        counts = torch.tensor([len(d) for d in chunk], dtype=torch.int32).to(self.device, non_blocking=True)
        w, h = chunk[0].size
        return self.overlay(frames.contiguous(), boxes, scores, labels, counts, (h, w), self.confidence_threshold,
                            self.thickness, self._dev_palette, self._dev_atlas)

    def iter_image_folder(self, folder, suffix=".JPEG"):
        """Generator form of run_on_image_folder: yields the annotated frames (uint8 RGB [H,W,3] numpy arrays) in order.
        With an output_folder every frame is also written as it is finished (generate_images on the source's thread
        pool: the encode of one chunk runs beside the render of the next)."""
        import time
        files = self.list_frames(folder, suffix)
        L = len(files)
        src = self._source(files)
        pending = []
        try:
            t0 = time.perf_counter()
            with torch.no_grad():
                dets = self._detect(src, files)
            if len(dets) != L:
                raise RuntimeError("the detector returned %d frames for a folder of %d" % (len(dets), L))
            self.predictions = dets
            src._drop_ahead()      # a read-ahead batch the engine left staged shares the pinned rings fetch_original uses
            cuda = self.device.type == "cuda"
            if cuda:
                torch.cuda.synchronize(self.device)
            self.timer["detect_s"] = time.perf_counter() - t0
            chunks = [list(range(o, min(L, o + self.render_chunk))) for o in range(0, L, self.render_chunk)]
            stage = None
            for c, ids in enumerate(chunks):
                if c + 1 < len(chunks):
                    src.prefetch(chunks[c + 1])
                dev = self._render_chunk(src, dets, ids)
                if cuda:      # one D2H copy per chunk into pinned memory
                    if stage is None or stage.shape[0] < len(ids):
                        stage = torch.empty((len(ids),) + tuple(dev.shape[1:]), dtype=torch.uint8).pin_memory()
                    stage[:len(ids)].copy_(dev, non_blocking=True)
                    torch.cuda.current_stream(self.device).synchronize()
                    out = [stage[i].numpy().copy() for i in range(len(ids))]
                else:
                    out = [dev[i].numpy().copy() for i in range(len(ids))]
                if self.output_folder:
                    pending.append(self._write(out, ids[0], src.pool))
                for a in out:
                    yield a
            for futs in pending:
                for f in futs:
                    f.result()
            pending = []
            self.predictions = [d.to("cpu") for d in dets]      # as compute_on_dataset returns them
            self.timer["total_s"] = time.perf_counter() - t0
        finally:
            for futs in pending:
                for f in futs:
                    f.cancel()
            src.close()

    def run_on_image_folder(self, folder, suffix=".JPEG"):
        """predictor.py:398-489: the sorted "*<suffix>" files of `folder` as one video -> the annotated frames, a list
        of uint8 RGB arrays of the original size.  self.predictions holds the raw detections afterwards: list[BoxList] on
        the host, in the resized frame's coordinates, as inference.compute_on_dataset returns them."""
        return list(self.iter_image_folder(folder, suffix))

    # ------------------------------------------------------------------------------------------ output
    def _write(self, frames, first_id, pool):
        os.makedirs(self.output_folder, exist_ok=True)
        return [pool.submit(encode_jpeg, os.path.join(self.output_folder, "%06d.jpg" % (first_id + i)), a)
                for i, a in enumerate(frames)]

    def generate_images(self, frames, first_id=0):
        """predictor.py:616-618: <output_folder>/%06d.jpg (JPEG quality 95, cv2.imwrite's default), encoded in parallel"""
        if not self.output_folder:
            raise ValueError("generate_images needs an output_folder")
        with ThreadPoolExecutor(max_workers=8) as pool:
            for f in self._write(frames, first_id, pool):
                f.result()
