"""The JPEG cases of tests/test_jpeg.py and tests/test_jpeg_gpu.py: every image is built in memory with Pillow, every
coefficient-level case directly, so there are no fixtures.  A stream case is (name, JPEG bytes); a coefficient case is
(name, width, height, sampling code, int16 buffer in the layout of mega/pytorch_amd/jpeg.py)."""
import io

import numpy as np
from PIL import Image

from mega.pytorch_amd import jpeg

# W x H: a single pixel, a partial MCU on each edge, odd and even chroma widths, the one-column and one-row chroma edges;
# 3x5 and 4x4 have a chroma plane of 2 columns (replicated by the library, not interpolated), 2x7 one of 1 column
SIZES = ((1, 1), (8, 9), (16, 16), (17, 31), (33, 50), (45, 67))
NARROW = ((3, 5), (4, 4), (2, 7))
SAMPLINGS = (("444", 0), ("422", 1), ("420", 2), ("gray", None))
QUALITIES = (50, 95, 100)


def picture(w, h, seed, noise=False):
    """smooth colour gradients plus texture, or white noise: uint8 [h, w, 3]"""
    rng = np.random.RandomState(seed)
    if noise:
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 255.0 / max(w - 1, 1), yy * 255.0 / max(h - 1, 1), 255.0 - (xx + yy) * 255.0 / max(w + h - 2, 1)], -1)
    return np.clip(base + rng.normal(0, 30, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(rgb, sampling, quality=90, **kw):
    """JPEG bytes of uint8 [h, w, 3]; sampling: Pillow's subsampling code 0 / 1 / 2, or None for a grayscale image"""
    im = Image.fromarray(rgb)
    b = io.BytesIO()
    if sampling is None:
        im.convert("L").save(b, "JPEG", quality=quality, **kw)
    else:
        im.save(b, "JPEG", quality=quality, subsampling=sampling, **kw)
    return b.getvalue()


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def stream_cases():
    out = []
    seed = 0
    for w, h in SIZES + NARROW:
        for sname, s in SAMPLINGS:
            for q in QUALITIES:
                seed += 1
                out.append(("%dx%d-%s-q%d" % (w, h, sname, q), encode(picture(w, h, seed), s, q)))
            out.append(("%dx%d-%s-optimised" % (w, h, sname), encode(picture(w, h, seed + 1000), s, 75, optimize=True)))
    for sname, s in SAMPLINGS:
        out.append(("45x67-%s-restart3" % sname, encode(picture(45, 67, 77), s, 90, restart_marker_blocks=3)))
        out.append(("45x67-%s-noise-q100" % sname, encode(picture(45, 67, 78, noise=True), s, 100)))
    return out


def batch_case():
    """three different images of one size and sampling, as a batch"""
    return [encode(picture(33, 50, 200 + i, noise=(i == 2)), 2, (50, 95, 100)[i]) for i in range(3)]


def _buffer(w, h, sampling, qt_value, fill):
    info = jpeg.make_info(w, h, sampling)
    buf = np.zeros(info.coef_elems, dtype=np.int16)
    ncomp = 1 if sampling == jpeg.GRAY else 3
    buf[:64 * ncomp] = qt_value
    blocks = buf[jpeg.QT_ELEMS:].reshape(-1, 64)
    fill(blocks)
    return buf


def coef_cases():
    """coefficient-level cases, no entropy stage: a lone DC, a lone coefficient at each of the 64 positions, alternating-sign
    extremes whose dequantised values stay within int16, a lone highest frequency on a DC, dense blocks without symmetry"""
    out = []

    def lone_dc(b):
        b[:, 0] = np.arange(b.shape[0]) * 37 % 511 - 255

    def lone_each(b):
        for i in range(b.shape[0]):
            b[i, i % 64] = (200 + 13 * i) * (1 if (i // 64) % 2 == 0 else -1)

    def extremes(b):
        sign = np.where((np.arange(64) + np.arange(b.shape[0])[:, None]) % 2 == 0, 1, -1)
        b[:] = sign * 32767
        b[1::3] = -32768 * (sign[1::3] > 0) + 32767 * (sign[1::3] < 0)

    def checker(b):
        b[:, 63] = 1000
        b[:, 0] = -1024

    def dense(b):      # no symmetry between rows and columns: a transposed pass order or block shows
        b[:] = np.random.RandomState(b.shape[0]).randint(-60, 61, b.shape) * (np.arange(64) % 8 < 5)
        b[:, 0] = np.random.RandomState(1).randint(-900, 900, b.shape[0])

    for sname, s in (("gray", jpeg.GRAY), ("444", jpeg.S444), ("422", jpeg.S422), ("420", jpeg.S420)):
        out.append(("dense-%s" % sname, 45, 67, s, _buffer(45, 67, s, 5, dense)))
        out.append(("dc-%s" % sname, 33, 50, s, _buffer(33, 50, s, 8, lone_dc)))
        out.append(("each-%s" % sname, 64, 64, s, _buffer(64, 64, s, 3, lone_each)))      # 64 luma blocks: every position
        out.append(("extremes-%s" % sname, 17, 31, s, _buffer(17, 31, s, 1, extremes)))
        out.append(("checker-%s" % sname, 45, 67, s, _buffer(45, 67, s, 16, checker)))
    return out


def progressive():
    return encode(picture(33, 50, 5), 2, 90, progressive=True)


def truncations(data, count=24):
    """the stream cut at `count` byte positions spread over the whole file, the first few bytes and the last included"""
    n = len(data)
    cuts = sorted(set([1, 2, 3, 4, n - 1, n - 2] + [int(x) for x in np.linspace(5, n - 3, count)]))
    return [(c, data[:c]) for c in cuts if 0 < c < n]


def flips(data, count=24, seed=0):
    """the stream with a few bytes of its entropy-coded data replaced, `count` seeded variants"""
    import jpeg_twin
    start = jpeg_twin.parse(data).scan
    rng = np.random.RandomState(seed)
    out = []
    for i in range(count):
        d = bytearray(data)
        for _ in range(1 + i % 4):
            d[rng.randint(start, len(d) - 2)] = rng.randint(0, 256)
        out.append((i, bytes(d)))
    return out


def handmade(scan, ac_symbol=0xF1):
    """a one-block 8x8 gray JPEG written by hand: both Huffman tables hold ONE code, the single bit 0 -- DC category 0 and the
    AC symbol `ac_symbol` -- so the entropy data `scan` decides exactly which syntax rule breaks"""
    def seg(marker, body):
        return bytes([0xFF, marker, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + bytes(body)
    one_code = [1] + [0] * 15
    return (b"\xff\xd8" + seg(0xDB, [0] + [1] * 64) + seg(0xC0, [8, 0, 8, 0, 8, 1, 1, 0x11, 0])
            + seg(0xC4, [0x00] + one_code + [0]) + seg(0xC4, [0x10] + one_code + [ac_symbol])
            + seg(0xDA, [1, 1, 0x00, 0, 63, 0]) + bytes(scan) + b"\xff\xd9")


def replace_segment(data, marker, new_body=None, new_marker=None):
    """the stream with the body of its first `marker` segment replaced (None: the segment removed)"""
    p = 2
    while data[p + 1] != marker:
        p += 2 + ((data[p + 2] << 8) | data[p + 3])
    ln = (data[p + 2] << 8) | data[p + 3]
    if new_body is None:
        return data[:p] + data[p + 2 + ln:]
    body = bytes(new_body)
    return data[:p] + bytes([0xFF, new_marker or marker, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + body + data[p + 2 + ln:]


def segment(data, marker):
    p = 2
    while data[p + 1] != marker:
        p += 2 + ((data[p + 2] << 8) | data[p + 3])
    return data[p + 4:p + 2 + ((data[p + 2] << 8) | data[p + 3])]


def refused_cases():
    """(name, bytes) of streams outside the accepted set"""
    good = encode(picture(17, 31, 9), 2, 90)
    sof, sos = bytearray(segment(good, 0xC0)), bytearray(segment(good, 0xDA))
    out = [("progressive", progressive()),
           ("arithmetic", replace_segment(good, 0xC0, sof, new_marker=0xC9)),
           ("several-scans", replace_segment(good, 0xDA, [1, 1, 0x00, 0, 63, 0])),
           ("12-bit", replace_segment(good, 0xC0, bytes([12]) + bytes(sof[1:]))),
           ("dqt-16-bit", replace_segment(good, 0xDB, bytes([0x10]) + bytes(segment(good, 0xDB)[1:]))),
           ("sampling-4x1", replace_segment(good, 0xC0, bytes(sof[:7]) + bytes([0x41]) + bytes(sof[8:]))),
           ("sampling-1x2", replace_segment(good, 0xC0, bytes(sof[:7]) + bytes([0x12]) + bytes(sof[8:]))),
           ("chroma-2x1", replace_segment(good, 0xC0, bytes(sof[:10]) + bytes([0x21]) + bytes(sof[11:]))),
           ("adobe-transform-0", good[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + good[2:]),
           ("png", b"\x89PNG\r\n\x1a\n" + b"\0" * 32)]
    b = io.BytesIO()
    Image.fromarray(picture(17, 31, 9)).convert("CMYK").save(b, "JPEG", quality=90)
    out.append(("four-components", b.getvalue()))
    for i, c in enumerate(b"RGB"):
        sof[6 + 3 * i] = c
        sos[1 + 2 * i] = c
    rgb = replace_segment(replace_segment(replace_segment(good, 0xC0, sof), 0xDA, sos), 0xE0)
    out.append(("rgb-ids-without-jfif", rgb))
    return out


def corrupt_cases():
    """(name, bytes) of accepted streams that break a syntax rule"""
    rst = encode(picture(45, 67, 77), 2, 90, restart_marker_blocks=3)
    p = rst.index(b"\xff\xd0")
    good = encode(picture(33, 50, 3), 2, 90)
    import jpeg_twin
    scan = jpeg_twin.parse(good).scan
    return [("bad-huffman-code", handmade(b"\xff\x00\xff\x00\xff\x00")),            # sixteen 1 bits: no such code
            ("index-past-63", handmade(b"\x2a\xaa\xaa")),                            # DC, then run 15 + a coefficient, five times
            ("zero-run-past-63", handmade(b"\x00\x00", ac_symbol=0xF0)),             # ZRL four times
            ("wrong-rst-number", rst[:p + 1] + b"\xd1" + rst[p + 2:]),
            ("missing-rst", rst[:p] + rst[p + 2:]),
            ("ends-before-last-mcu", good[:scan + (len(good) - scan) // 2]),
            ("marker-before-last-mcu", good[:scan + (len(good) - scan) // 2] + b"\xff\xd9"),
            ("undefined-table", replace_segment(good, 0xC4))]
