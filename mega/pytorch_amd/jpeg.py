"""JPEG decode split between the host and the device: entropy decoding in C++ on the feed's worker threads, every pixel
stage in HIP.  This docstring is the definition; tests/jpeg_twin.py restates it in numpy, csrc/jpeg_entropy.h and csrc/jpeg.hip
implement it.  The contract is equality, byte for byte, with Pillow's `Image.open(path).convert("RGB")` (libjpeg /
libjpeg-turbo with its defaults: the accurate integer IDCT, "fancy" upsampling), so that a `feed.FrameSource(decode="device")`
hands the engines the same frames as the host path.

Accepted streams
  SOF0 or SOF1 (sequential Huffman), 8-bit samples; ONE interleaved scan over all components (Ss = 0, Se = 63, Ah = Al = 0,
  components in the frame's order); 1 component, or 3 components with Y sampled 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0) and
  Cb = Cr = 1x1; 8-bit DQT entries; DRI / RSTn allowed.  A one-component scan is never interleaved, so its sampling factors
  do not matter.
Refused with `Unsupported`
  progressive, arithmetic, lossless or differential frames; a scan over fewer components than the frame has (several scans);
  16-bit quantisation tables; 4 components; an Adobe APP14 segment whose transform is not 1 on a 3-component image (RGB
  stored as such); no JFIF and no Adobe segment together with the component ids 'R', 'G', 'B' (the library then takes the
  data for RGB); any other sampling; anything that is not a JPEG.
Truncated and corrupt streams
  end with `Corrupt`: a Huffman code that no symbol has, a DC category above 11, a coefficient index past 63 (a zero run
  counts), a missing RSTn or one with the wrong number, entropy data that ends (or meets a marker) before the last MCU, a
  table that is used but not defined.  The decoder never reads outside its input and never writes outside its output.

Stage 1, host (csrc/jpeg_entropy.h): markers, then the MCUs in order -- per component its v x h blocks, row by row; per block
  the DC difference added to the component's predictor (reset at every RSTn), then run / size pairs.  Output, int16:
    qt[3][64]    the quantisation table of component 0, 1, 2 in natural (row-major) order; zeros for a missing component
    coef planes  Y, then Cb, then Cr: [block row][block col][64], natural order, NOT dequantised, over the MCU-padded block
                 grid: with (hs, vs) the sampling of Y, mcus = ceil(W / 8hs) x ceil(H / 8vs), Y has (mcus_x hs) x (mcus_y vs)
                 blocks, Cb and Cr mcus_x x mcus_y.
  Every element is written, zeros included.  For 4:2:0 this is 3 bytes per pixel, what the RGB frame it replaces takes.

Stage 2, device: dequantise (coefficient times table entry, int32) and libjpeg's accurate integer inverse DCT, jidctint.c at
  8x8: CONST_BITS = 13, PASS1_BITS = 2; constants FIX(0.298631336) = 2446, FIX(0.390180644) = 3196, FIX(0.541196100) = 4433,
  FIX(0.765366865) = 6270, FIX(0.899976223) = 7373, FIX(1.175875602) = 9633, FIX(1.501321110) = 12299, FIX(1.847759065) =
  15137, FIX(1.961570560) = 16069, FIX(2.053119869) = 16819, FIX(2.562915447) = 20995, FIX(3.072711026) = 25172.  One pass:
    even  z1 = (x2 + x6) 4433; t2 = z1 - x6 15137; t3 = z1 + x2 6270; t0 = (x0 + x4) << 13; t1 = (x0 - x4) << 13;
          t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2
    odd   a0 = x7, a1 = x5, a2 = x3, a3 = x1; z1 = a0 + a3, z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3; z5 = (z3 + z4) 9633;
          a0 *= 2446, a1 *= 16819, a2 *= 25172, a3 *= 12299; z1 *= -7373, z2 *= -20995, z3 = z3 (-16069) + z5,
          z4 = z4 (-3196) + z5; a0 += z1 + z3, a1 += z2 + z4, a2 += z2 + z3, a3 += z1 + z4
    out   y0, y7 = t10 +- a3; y1, y6 = t11 +- a2; y2, y5 = t12 +- a1; y3, y4 = t13 +- a0
  The column pass descales by 11, the row pass by 18, both round half up: (x + (1 << (n - 1))) >> n, arithmetic shift.  Then
  + 128 and a clamp to [0, 255].  int32 arithmetic throughout, wrapping.  Equality with the library is claimed for streams
  whose dequantised coefficients fit int16 (the library's own vector paths assume the same; every encoder's output does):
  nothing wraps then.  Outside that range the kernel clamps where the library's range table would wrap.

Stage 3, device: "fancy" upsampling of Cb and Cr.  The component's size is cw x ch = ceil(W hs' / hs) x ceil(H vs' / vs) (its
  own factors over the maxima); rows and columns of MCU padding are never read as neighbours.
    h2v1 (4:2:2)  sample s of column c gives outputs 2c and 2c + 1: (3 s + left + 1) >> 2 and (3 s + right + 2) >> 2; output 0
                  and output 2 cw - 1 are copies of the first / last sample.
    h2v2 (4:2:0)  output row 2r takes near = chroma row r and far = row r - 1, output row 2r + 1 far = row r + 1; the row above
                  the first chroma row is the first row itself, the row below the last the last.  With c = 3 near + far per
                  column: (3 c + c_left + 8) >> 4 and (3 c + c_right + 7) >> 4; at the ends (4 c + 8) >> 4 and
                  (4 c + 7) >> 4.
    cw <= 2       the library does not interpolate a plane that narrow: samples are replicated (2x1 or 2x2 boxes).
Stage 4, device: with Cb and Cr centred on 128,
    R = Y + ((91881 Cr + 32768) >> 16);  G = Y + ((-22554 Cb - 46802 Cr + 32768) >> 16);  B = Y + ((116130 Cb + 32768) >> 16)
  arithmetic shifts, results clamped to [0, 255].  A one-component image replicates Y into R, G, B.
"""
import numpy as np

from . import ops

INFO_INTS = 12
QT_ELEMS = 192
GRAY, S444, S422, S420 = 0, 1, 2, 3


class Unsupported(ValueError):
    """The stream is outside the accepted set (or is not a JPEG): decode it on the host."""


class Corrupt(ValueError):
    """The stream is inside the accepted set and breaks off or breaks the syntax."""


class Info(object):
    """What the probe learned: width, height, components, sampling code, per-component block grids, restart interval,
    int16 elements of the entropy decode's output.  `array` is the int32 array the C ABI reads."""

    def __init__(self, array):
        a = np.ascontiguousarray(array, dtype=np.int32)
        assert a.shape == (INFO_INTS,)
        self.array = a
        self.width, self.height, self.ncomp, self.sampling = (int(v) for v in a[:4])
        self.blocks = tuple((int(a[4 + 2 * c]), int(a[5 + 2 * c])) for c in range(3))      # (per row, per column)
        self.restart, self.coef_elems = int(a[10]), int(a[11])

    @property
    def hw(self):
        return (self.height, self.width)

    @property
    def stride(self):
        """elements between the frames of a batch: coef_elems rounded up to 8 (frames start on 16-byte boundaries)"""
        return (self.coef_elems + 7) // 8 * 8

    def same_frames(self, other):
        return (self.width, self.height, self.ncomp, self.sampling) == (other.width, other.height, other.ncomp, other.sampling)


def geometry(width, height, sampling):
    """the MCU-padded block grid ((per row, per column) of Y, Cb, Cr) of a frame size and sampling code"""
    hs, vs = (2 if sampling >= S422 else 1), (2 if sampling == S420 else 1)
    mx, my = -(-width // (8 * hs)), -(-height // (8 * vs))
    c = (0, 0) if sampling == GRAY else (mx, my)
    return ((mx * hs, my * vs), c, c)


def make_info(width, height, sampling, restart=0):
    """an Info from the frame size and sampling code alone (coefficient-level tests and tools have no stream to probe)"""
    g = geometry(width, height, sampling)
    a = [width, height, 1 if sampling == GRAY else 3, sampling]
    for bw, bh in g:
        a += [bw, bh]
    a += [restart, QT_ELEMS + 64 * sum(bw * bh for bw, bh in g)]
    return Info(np.array(a, dtype=np.int32))


def probe(data):
    """Info of the JPEG held in `data` (bytes); raises Unsupported"""
    return Info(ops.jpeg_probe(data))
