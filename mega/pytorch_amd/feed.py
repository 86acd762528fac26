"""Test-time frame feed: the step BEFORE the hot path.

Mirror of the reference's test-time input pipeline
  mega_core/data/datasets/vid_mega.py:95-142      VIDMEGADataset._get_test  (which frames a key frame consumes)
  mega_core/data/transforms/transforms.py:27-66   Resize.get_size / F.resize (PIL BILINEAR)
  mega_core/data/transforms/transforms.py:107-129 ToTensor + Normalize(to_bgr255)
  mega_core/data/transforms/build.py:26-45        the test-time Compose
re-designed for a GPU whose per-key-frame step is ~2 ms: JPEG decode stays on host worker threads (PIL releases the
GIL while decoding), decoded uint8 frames land in pinned staging buffers, ONE async H2D copy per batch, and
Resize + BGR/mean run on the device (mega_resize_bilinear_u8, bit-identical to Pillow's resampler, then
mega_preprocess_frames).  The in-forward `PIL.Image.open` of the reference's cold start
(generalized_rcnn_mega.py:185-191) disappears: every frame goes through the same source.

`FrameSource` is the object ClipEngine.run() accepts in place of a resident clip tensor.

decode="device" (opt-in; jpeg.py defines it) moves the per-pixel half of the JPEG decode to the device as well: the worker
threads only read the file and entropy-decode it (C++, csrc/jpeg_entropy.h) into int16 DCT coefficients, the pinned staging
buffers hold coefficients instead of pixels (3 bytes per pixel for 4:2:0, as before), and two HIP launches per batch --
dequantise + IDCT, then chroma upsampling + YCbCr -> RGB -- produce the same [n,H,W,3] uint8 tensor, bit for bit.
"""
import io
import math
import os
import threading
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import jpeg
from . import ops

PRECISION_BITS = 32 - 8 - 2


def get_size(image_size, min_size=600, max_size=1000):
    """transforms.py:35-55 Resize.get_size for one min_size: (w, h) -> (oh, ow)."""
    w, h = image_size
    size = min_size
    if max_size is not None:
        min_original_size = float(min((w, h)))
        max_original_size = float(max((w, h)))
        if max_original_size / min_original_size * size > max_size:
            size = int(round(max_size * min_original_size / max_original_size))
    if (w <= h and w == size) or (h <= w and h == size):
        return (h, w)
    if w < h:
        ow = size
        oh = int(size * h / w)
    else:
        oh = size
        ow = int(size * w / h)
    return (oh, ow)


def pil_bilinear_coeffs(in_size, out_size):
    """Pillow libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc for the BILINEAR (triangle, support 1)
    filter over the full box [0, in_size): returns (bounds int32 [out,2] = first tap / tap count,
    coeffs int32 [out,ksize] fixed-point << 22, ksize).  Double-precision host arithmetic, as in Pillow."""
    scale = float(np.float32(in_size) - np.float32(0.0)) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.float64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        x = np.arange(xmax, dtype=np.float64)
        a = np.abs((x + xmin - center + 0.5) * ss)
        w = np.where(a < 1.0, 1.0 - a, 0.0)
        ww = 0.0
        for v in w:                      # sequential double sum, same order as the C loop
            ww += float(v)
        if ww != 0.0:
            w = w / ww
        kk[xx, :xmax] = w
        bounds[xx] = (xmin, xmax)
    ki = np.where(kk < 0, -0.5 + kk * (1 << PRECISION_BITS), 0.5 + kk * (1 << PRECISION_BITS)).astype(np.int64)
    return bounds, ki.astype(np.int32), ksize


class ResizeTables(object):
    """Device-resident coefficient tables of one (input size -> output size) resize."""

    def __init__(self, in_hw, out_hw, device):
        self.in_hw, self.out_hw = tuple(in_hw), tuple(out_hw)
        bh, ch, self.ksize_h = pil_bilinear_coeffs(in_hw[1], out_hw[1])
        bv, cv, self.ksize_v = pil_bilinear_coeffs(in_hw[0], out_hw[0])
        self.bounds_h = torch.from_numpy(bh).to(device)
        self.coef_h = torch.from_numpy(ch).to(device)
        self.bounds_v = torch.from_numpy(bv).to(device)
        self.coef_v = torch.from_numpy(cv).to(device)


def frame_ids_for_key(idx, seg_len, max_offset, global_size, shuffled, global_enable=True):
    """vid_mega.py:95-120 for a single video starting at dataset index 0: (ref_l frame id, [ref_g frame ids])."""
    ref_l = min(seg_len - 1, idx + max_offset)
    ref_g = []
    if global_enable:
        size = global_size if idx == 0 else 1
        ref_g = [int(shuffled[(idx + global_size - i - 1) % seg_len]) for i in range(size)]
    return ref_l, ref_g


class FrameSource(object):
    """A video as a directory of image files, presented to ClipEngine like a resident uint8 clip.

    img_dir / pattern follow the reference's conventions (`img_dir % (pattern % frame_id)`,
    vid_mega.py:108-109, vid.py `_img_dir`/`pattern`).  fetch(ids) returns the RESIZED uint8 frames [n,H,W,3] on
    the device, fetch_original(ids) the decoded frames before the resize; prefetch(ids) starts the host decodes early.

    decode: "host" (default) decodes every frame with Pillow on the worker threads.  "device" (a HIP device, no `opener`):
    frame 0 is probed instead of decoded; if it is a JPEG the device decoder accepts (jpeg.py), the workers entropy-decode
    and the pixels are made on the device -- `decode_mode` is then "device" -- else the source silently becomes a host
    source (`decode_mode` "host": a folder of PNGs, say).  A later frame that the decoder refuses, or whose sampling differs
    from frame 0's, is decoded by Pillow and copied into its slot after the kernels; `host_fallbacks` counts such frames.
    reader: frame id -> the file's bytes, in place of img_dir / pattern (a caller that holds a list of files)."""

    def __init__(self, img_dir, pattern, seg_len, device, min_size=600, max_size=1000, workers=8, cache_frames=64,
                 opener=None, hflip=False, decode="host", reader=None):
        # hflip: every fetched frame is mirrored left-right after the resize (a TEST.BBOX_AUG flip view, bbox_aug.py)
        self.hflip = bool(hflip)
        self.img_dir, self.pattern, self.seg_len = img_dir, pattern, int(seg_len)
        self.device = torch.device(device)
        if decode not in ("host", "device"):
            raise ValueError('decode must be "host" or "device", got %r' % (decode,))
        if decode == "device" and opener is not None:
            raise ValueError('decode="device" reads the files itself: it cannot be combined with an opener')
        if decode == "device" and self.device.type != "cuda":
            raise ValueError('decode="device" needs a HIP device, got %s' % self.device)
        self.reader = reader
        self.opener = opener or self._open
        self.decode_mode = "host"
        self.jpeg_info = None
        self._fallback_ids = set()
        self._lock = threading.Lock()
        if decode == "device":
            try:
                self.jpeg_info = jpeg.probe(self._read(0))
                self.decode_mode = "device"
            except jpeg.Unsupported:
                pass
        if self.decode_mode == "device":
            self.in_hw = self.jpeg_info.hw
        else:
            first = self.opener(0)
            self.in_hw = (first.shape[0], first.shape[1])
        self.out_hw = get_size((self.in_hw[1], self.in_hw[0]), min_size, max_size)
        self.pool = ThreadPoolExecutor(max_workers=workers)
        self.cache = OrderedDict()
        self.cache_frames = cache_frames
        self.tables = None
        self._stage = {}      # batch size -> ring of [pinned staging buffer, event of the last H2D copy that read it]
        self.dtype = torch.uint8
        self.is_cuda = self.device.type == "cuda"
        self.shape = (self.seg_len, self.out_hw[0], self.out_hw[1], 3)
        self.decoded = 0
        # read-ahead (stage_ahead): ONE batch staged beyond what has been fetched -- key, device tensor, the event of its last
        # H2D copy, the thread that fills the pinned buffer and issues the copies on the copy stream
        self._ahead = None
        self._copy_stream = None
        self.ahead_hits = 0

    @property
    def host_fallbacks(self):
        """frames of a decode="device" source that Pillow had to decode"""
        return len(self._fallback_ids)

    def _read(self, frame_id):
        """the bytes of frame `frame_id`'s file"""
        if self.reader is not None:
            return self.reader(frame_id)
        path = self.img_dir % (self.pattern % frame_id)
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        with open(path, "rb") as f:
            return f.read()

    def _open(self, frame_id):
        from PIL import Image
        if self.reader is not None:
            return np.asarray(Image.open(io.BytesIO(self.reader(frame_id))).convert("RGB"))
        path = self.img_dir % (self.pattern % frame_id)
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        return np.asarray(Image.open(path).convert("RGB"))

    def _decode(self, frame_id):
        if self.decode_mode == "device":
            return self._entropy_decode(frame_id)
        a = self.opener(frame_id)
        if a.shape[:2] != self.in_hw:
            raise ValueError("frame %d is %s, the video started as %s" % (frame_id, a.shape[:2], self.in_hw))
        self.decoded += 1
        return a

    def _entropy_decode(self, frame_id):
        """decode="device", on a worker thread: the frame's int16 coefficient slot [stride] (ctypes releases the GIL around
        the C++ decoder) -- or, for a frame the decoder refuses, its uint8 RGB [Hi,Wi,3] from Pillow"""
        data = self._read(frame_id)
        try:
            out = ops.jpeg_entropy_decode(data, self.jpeg_info, np.empty(self.jpeg_info.stride, dtype=np.int16))
        except (jpeg.Unsupported, jpeg.Corrupt):
            from PIL import Image
            out = np.array(Image.open(io.BytesIO(data)).convert("RGB"))      # (a corrupt file raises here, as on the host path)
            if out.shape[:2] != self.in_hw:
                raise ValueError("frame %d is %s, the video started as %s" % (frame_id, out.shape[:2], self.in_hw))
            with self._lock:
                self._fallback_ids.add(frame_id)
        self.decoded += 1
        return out

    def prefetch(self, ids):
        for f in ids:
            f = int(f)
            if f not in self.cache:
                self.cache[f] = self.pool.submit(self._decode, f)
        while len(self.cache) > self.cache_frames:
            self.cache.popitem(last=False)

    def stage_ahead(self, ids):
        """Start bringing a LATER batch onto the device now: a background thread fills a pinned buffer from the decode cache and
        issues the H2D copies on the source's own copy stream, so they run beside whatever the device is doing for the
        current batch; fetch(ids) with the same ids then only waits for that event.  One batch of read-ahead; a fetch of
        anything else drops it.  (ClipEngine.run() calls this with the step-batch that FOLLOWS the range it was asked for --
        a caller that walks the video block by block finds every block's frames already in HBM: the reference's loader
        overlaps its H2D the same way, one DataLoader batch ahead of the forward, engine/inference.py:24-42.)"""
        if not self.is_cuda:
            return
        key = tuple(int(f) for f in ids)
        if not key or (self._ahead is not None and self._ahead["key"] == key):
            return
        self._drop_ahead()
        self.prefetch(key)
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=self.device)
        import threading
        ent = {"key": key, "dev": None, "ev": None, "err": None}

        def work():
            try:
                with torch.cuda.stream(self._copy_stream):
                    ent["dev"] = self._to_device(key)
                    ent["ev"] = torch.cuda.Event()
                    ent["ev"].record(self._copy_stream)
            except Exception as e:  # noqa: BLE001  (surfaced by the fetch that asks for this batch)
                ent["err"] = e
        ent["thread"] = threading.Thread(target=work, daemon=True)
        ent["thread"].start()
        self._ahead = ent

    def _drop_ahead(self):
        ent, self._ahead = self._ahead, None
        if ent is not None:
            ent["thread"].join()
            if ent["ev"] is not None:
                ent["ev"].synchronize()      # its staging buffer and device tensor may be re-used after this

    def fetch(self, ids):
        ent = self._ahead
        if ent is not None and ent["key"] == tuple(int(f) for f in ids):
            self._ahead = None
            ent["thread"].join()
            if ent["err"] is not None:
                raise ent["err"]
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ent["ev"])
            ent["dev"].record_stream(cur)
            self.ahead_hits += 1
            return self._resized(ent["dev"])
        if ent is not None:
            self._drop_ahead()
        return self._resized(self._to_device(ids))

    def fetch_original(self, ids):
        """the decoded, UNRESIZED uint8 frames `ids` [n,Hi,Wi,3] on the device (what the demo draws on): the same host
        decode cache and pinned staging as fetch(); the read-ahead batch, if any, is left alone"""
        return self._to_device(ids)

    def _resized(self, dev):
        if self.out_hw == self.in_hw:
            return ops.resize_bilinear_u8_flip(dev, self.out_hw, None) if self.hflip else dev
        if self.tables is None:
            self.tables = ResizeTables(self.in_hw, self.out_hw, self.device)
        if self.hflip:
            return ops.resize_bilinear_u8_flip(dev, self.out_hw, self.tables)
        return ops.resize_bilinear_u8(dev, self.out_hw, self.tables)

    def _to_device(self, ids):
        """the decoded frames `ids` as ONE uint8 device tensor [n,Hi,Wi,3] (host copies + H2D on the CURRENT stream)"""
        self.prefetch(ids)
        n = len(ids)
        if self.decode_mode == "device":
            return self._to_device_coefficients(ids)
        # pinned staging buffers are a small ring per batch size, re-used once the H2D copy that read them has completed
        # (an event per buffer): page-locking a fresh 72 MB buffer per 40-frame batch costs more than the copy it feeds
        ev = None
        if self.is_cuda:
            ring = self._stage.setdefault(n, [])
            slot = next((x for x in ring if x[1].query()), None)
            if slot is None and len(ring) >= 3:
                slot = ring[0]
                slot[1].synchronize()
            if slot is None:
                slot = [torch.empty((n, self.in_hw[0], self.in_hw[1], 3), dtype=torch.uint8).pin_memory(), torch.cuda.Event()]
                ring.append(slot)
            else:
                ring.remove(slot)
                ring.append(slot)
            stage, ev = slot
        else:
            stage = torch.empty((n, self.in_hw[0], self.in_hw[1], 3), dtype=torch.uint8)
        view = stage.numpy()
        futs = [self.cache.get(int(f)) or self.pool.submit(self._decode, int(f)) for f in ids]
        # the copies into the staging buffer run on the worker threads too (numpy releases the GIL): 40 frames of 1.8 MB
        # are ~10 ms on one thread, which would sit serially in front of every frame-stage launch

        # (put() tasks wait on decode futures that run on the SAME pool: deadlock-free because ThreadPoolExecutor starts its
        #  tasks in submission order and every decode was submitted -- by prefetch() or the line above -- before any put())
        def put(i):
            np.copyto(view[i], futs[i].result())
        if self.is_cuda and n >= 8:
            # chunks: the H2D copy of chunk c runs while the workers fill chunk c + 1 of the staging buffer
            dev = torch.empty(stage.shape, dtype=torch.uint8, device=self.device)
            nch = 4
            for c in range(nch):
                lo, hi = c * n // nch, (c + 1) * n // nch
                list(self.pool.map(put, range(lo, hi)))
                dev[lo:hi].copy_(stage[lo:hi], non_blocking=True)
        else:
            list(self.pool.map(put, range(n)))
            dev = stage.to(self.device, non_blocking=True)
        if ev is not None:
            ev.record()
        return dev

    def _to_device_coefficients(self, ids):
        """_to_device of a decode="device" source: the pinned ring holds int16 coefficient slots [n,stride]; each chunk is
        copied and then reconstructed (mega_jpeg_reconstruct: two launches) on the CURRENT stream, behind its copy"""
        n, info = len(ids), self.jpeg_info
        ring = self._stage.setdefault(n, [])
        slot = next((x for x in ring if x[1].query()), None)
        if slot is None and len(ring) >= 3:
            slot = ring[0]
            slot[1].synchronize()
        if slot is None:
            slot = [torch.empty((n, info.stride), dtype=torch.int16).pin_memory(), torch.cuda.Event()]
            ring.append(slot)
        else:
            ring.remove(slot)
            ring.append(slot)
        stage, ev = slot
        view = stage.numpy()
        futs = [self.cache.get(int(f)) or self.pool.submit(self._decode, int(f)) for f in ids]
        late = {}      # position in the batch -> the RGB of a frame Pillow decoded

        def put(i):      # (on the workers, after the decodes: see _to_device)
            r = futs[i].result()
            if r.dtype == np.int16:
                np.copyto(view[i], r)
            else:
                view[i].fill(0)      # its slot still goes through the kernels: defined coefficients, a gray frame
                late[i] = r
        coef = torch.empty(stage.shape, dtype=torch.int16, device=self.device)
        dev = torch.empty((n, self.in_hw[0], self.in_hw[1], 3), dtype=torch.uint8, device=self.device)
        nch = 4 if n >= 8 else 1
        for c in range(nch):
            lo, hi = c * n // nch, (c + 1) * n // nch
            list(self.pool.map(put, range(lo, hi)))
            coef[lo:hi].copy_(stage[lo:hi], non_blocking=True)
            ops.jpeg_reconstruct(coef[lo:hi], info, out=dev[lo:hi])
        ev.record()
        for i, rgb in sorted(late.items()):
            dev[i].copy_(torch.from_numpy(rgb))      # (pageable memory: the copy returns when it is done)
        return dev

    def close(self):
        self._drop_ahead()
        self.pool.shutdown(wait=False)
        self._stage = {}          # (the pinned staging rings: up to 3 buffers of n x H x W x 3 per batch size seen -- ADVICE r05)
