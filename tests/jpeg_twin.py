"""numpy twin of mega/pytorch_amd/jpeg.py (the module docstring there is the definition): a marker parser, a plain bit-by-bit
Huffman decoder and the three pixel stages -- dequantise + integer IDCT, fancy upsampling, YCbCr -> RGB.  Slow and obvious on
purpose.  `faults` plants a wrong detail in one stage (tests/test_jpeg.py checks that the cases notice each):
  "round78"    the h2v2 rounding constants 8 and 7 swapped
  "edge"       the last chroma column and row take the plane's MCU padding for their right / lower neighbour
  "transpose"  the IDCT passes transposed: rows first (descaled by 11), then columns (by 18) -- only roundings differ
"""
import numpy as np

from mega.pytorch_amd.jpeg import Corrupt, Unsupported, GRAY, S420, S422, S444, QT_ELEMS, geometry

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])      # zigzag position -> natural (row-major) index


# ---------------------------------------------------------------------------------------------------- stage 0: markers
class Header(object):
    pass


def parse(data):
    d = bytes(data)
    if len(d) < 4 or d[0:2] != b"\xff\xd8":
        raise Unsupported("no SOI")
    h = Header()
    h.qt, h.dc, h.ac, h.restart = {}, {}, {}, 0
    sof = jfif = adobe = False
    transform = -1
    p = 2
    while True:
        if p + 2 > len(d) or d[p] != 0xFF:
            raise Corrupt("marker expected at %d" % p)
        while p < len(d) and d[p] == 0xFF:
            p += 1
        if p >= len(d):
            raise Corrupt("ends in fill bytes")
        m = d[p]
        p += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m in (0xD8, 0xD9, 0x00):
            raise Corrupt("marker %02x before SOS" % m)
        if p + 2 > len(d):
            raise Corrupt("segment length")
        ln = (d[p] << 8) | d[p + 1]
        if ln < 2 or p + ln > len(d):
            raise Corrupt("segment beyond the data")
        s = d[p + 2:p + ln]
        p += ln
        if m in (0xC0, 0xC1):
            if sof or len(s) < 6:
                raise Corrupt("SOF")
            if s[0] != 8:
                raise Unsupported("%d-bit samples" % s[0])
            h.height, h.width, h.ncomp = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            if h.ncomp not in (1, 3):
                raise Unsupported("%d components" % h.ncomp)
            if h.width == 0 or h.height == 0:
                raise Unsupported("empty frame")
            if len(s) != 6 + 3 * h.ncomp:
                raise Corrupt("SOF length")
            h.comp = [dict(id=s[6 + 3 * c], h=s[7 + 3 * c] >> 4, v=s[7 + 3 * c] & 15, tq=s[8 + 3 * c]) for c in range(h.ncomp)]
            for k in h.comp:
                if not (1 <= k["h"] <= 4 and 1 <= k["v"] <= 4 and k["tq"] <= 3):
                    raise Corrupt("component")
            if h.ncomp == 1:
                h.sampling = GRAY
            else:
                if any((k["h"], k["v"]) != (1, 1) for k in h.comp[1:]):
                    raise Unsupported("chroma sampling")
                try:
                    h.sampling = {(1, 1): S444, (2, 1): S422, (2, 2): S420}[(h.comp[0]["h"], h.comp[0]["v"])]
                except KeyError:
                    raise Unsupported("luma sampling")
            sof = True
        elif 0xC2 <= m <= 0xCF and m not in (0xC4, 0xC8):
            raise Unsupported("frame type %02x" % m)
        elif m == 0xC4:
            q = 0
            while q < len(s):
                if q + 17 > len(s):
                    raise Corrupt("DHT")
                tc, th = s[q] >> 4, s[q] & 15
                bits = list(s[q + 1:q + 17])
                n = sum(bits)
                if tc > 1 or th > 3 or n > 256 or q + 17 + n > len(s):
                    raise Corrupt("DHT")
                (h.ac if tc else h.dc)[th] = (bits, list(s[q + 17:q + 17 + n]))
                q += 17 + n
        elif m == 0xDB:
            q = 0
            while q < len(s):
                pq, tq = s[q] >> 4, s[q] & 15
                if pq == 1:
                    raise Unsupported("16-bit quantisation table")
                if pq != 0 or tq > 3 or q + 65 > len(s):
                    raise Corrupt("DQT")
                h.qt[tq] = np.array(list(s[q + 1:q + 65]), dtype=np.int16)
                q += 65
        elif m == 0xDD:
            if len(s) != 2:
                raise Corrupt("DRI")
            h.restart = (s[0] << 8) | s[1]
        elif m == 0xE0:
            jfif = jfif or s[:5] == b"JFIF\0"
        elif m == 0xEE:
            if len(s) >= 12 and s[:5] == b"Adobe":
                adobe, transform = True, s[11]
        elif m == 0xDA:
            if not sof or len(s) < 1:
                raise Corrupt("SOS")
            ns = s[0]
            if not 1 <= ns <= 4 or len(s) != 4 + 2 * ns:
                raise Corrupt("SOS length")
            if ns != h.ncomp:
                raise Unsupported("several scans")
            for c in range(ns):
                if s[1 + 2 * c] != h.comp[c]["id"]:
                    raise Unsupported("scan order")
                h.comp[c]["td"], h.comp[c]["ta"] = s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15
                if h.comp[c]["td"] > 3 or h.comp[c]["ta"] > 3:
                    raise Corrupt("table ids")
            if (s[1 + 2 * ns], s[2 + 2 * ns], s[3 + 2 * ns]) != (0, 63, 0):
                raise Unsupported("spectral selection / approximation")
            h.scan = p
            break
    if h.ncomp == 3:
        if adobe and transform != 1:
            raise Unsupported("Adobe transform %d" % transform)
        if not jfif and not adobe and [k["id"] for k in h.comp] == [ord("R"), ord("G"), ord("B")]:
            raise Unsupported("RGB component ids")
    for k in h.comp:
        if k["tq"] not in h.qt or k["td"] not in h.dc or k["ta"] not in h.ac:
            raise Corrupt("undefined table")
    h.blocks = geometry(h.width, h.height, h.sampling)
    h.coef_elems = QT_ELEMS + 64 * sum(bw * bh for bw, bh in h.blocks)
    return h


# ---------------------------------------------------------------------------------------------------- stage 1: entropy
def _codes(bits, vals):
    """{(length, code): symbol} by the canonical assignment"""
    out, code, p = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            if code >= (1 << l):
                raise Corrupt("Huffman counts")
            out[(l, code)] = vals[p]
            p += 1
            code += 1
        code <<= 1
    return out


class _Bits(object):
    """the entropy-coded segment bit by bit: FF 00 is the byte FF, any other FF xx ends the data"""

    def __init__(self, d, pos):
        self.d, self.pos, self.cur, self.left = d, pos, 0, 0

    def bit(self):
        if self.left == 0:
            d, p = self.d, self.pos
            if p >= len(d):
                raise Corrupt("data ends inside an MCU")
            if d[p] == 0xFF:
                if p + 1 < len(d) and d[p + 1] == 0:
                    self.pos += 2
                else:
                    raise Corrupt("marker inside an MCU")
            else:
                self.pos += 1
            self.cur, self.left = d[p], 8
        self.left -= 1
        return (self.cur >> self.left) & 1

    def symbol(self, codes):
        code = 0
        for l in range(1, 17):
            code = (code << 1) | self.bit()
            if (l, code) in codes:
                return codes[(l, code)]
        raise Corrupt("bad Huffman code")

    def value(self, s):
        v = 0
        for _ in range(s):
            v = (v << 1) | self.bit()
        return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def entropy_decode(data):
    """(Header, int16 coefficient buffer in the layout of jpeg.py)"""
    d = bytes(data)
    h = parse(d)
    out = np.zeros(h.coef_elems, dtype=np.int16)
    for c, k in enumerate(h.comp):
        out[64 * c + ZIGZAG] = h.qt[k["tq"]]
    offs = np.cumsum([QT_ELEMS] + [64 * bw * bh for bw, bh in h.blocks])
    dc = [_codes(*h.dc[k["td"]]) for k in h.comp]
    ac = [_codes(*h.ac[k["ta"]]) for k in h.comp]
    hs, vs = (2 if h.sampling >= S422 else 1), (2 if h.sampling == S420 else 1)
    mx, my = h.blocks[0][0] // hs, h.blocks[0][1] // vs
    br = _Bits(d, h.scan)
    pred = [0] * 3
    done = rst = 0
    for yy in range(my):
        for xx in range(mx):
            if h.restart and done and done % h.restart == 0:
                if d[br.pos:br.pos + 2] != bytes([0xFF, 0xD0 + rst]):
                    raise Corrupt("RST%d expected" % rst)
                br = _Bits(d, br.pos + 2)
                rst = (rst + 1) & 7
                pred = [0] * 3
            for c in range(h.ncomp):
                ch, cv = (hs, vs) if c == 0 else (1, 1)
                for v in range(cv):
                    for hh in range(ch):
                        base = offs[c] + 64 * ((yy * cv + v) * h.blocks[c][0] + xx * ch + hh)
                        s = br.symbol(dc[c])
                        if s > 11:
                            raise Corrupt("DC category %d" % s)
                        if s:
                            pred[c] += br.value(s)
                        out[base] = np.int16(((pred[c] + 32768) & 0xFFFF) - 32768)
                        k = 1
                        while k < 64:
                            rs = br.symbol(ac[c])
                            r, s = rs >> 4, rs & 15
                            if s:
                                k += r
                                if k > 63:
                                    raise Corrupt("coefficient index past 63")
                                out[base + ZIGZAG[k]] = br.value(s)
                                k += 1
                            elif r == 15:
                                k += 16
                                if k > 63:
                                    raise Corrupt("zero run past 63")
                            elif r == 0:
                                break
                            else:
                                raise Corrupt("EOBn in a sequential scan")
            done += 1
    return h, out


# ---------------------------------------------------------------------------------------------------- stage 2: IDCT
def _i32(x):
    """int64 values wrapped into int32's range (kept as int64, so that the next product cannot overflow the holder)"""
    return (np.asarray(x, dtype=np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31


def _pass(x):
    """one 1-D pass along axis 0 of x [8, ...] (int64 holding wrapped int32 values), not descaled"""
    x0, x1, x2, x3, x4, x5, x6, x7 = (x[i] for i in range(8))
    w = _i32
    z1 = w((x2 + x6) * 4433)
    t2 = w(z1 + w(x6 * -15137))
    t3 = w(z1 + w(x2 * 6270))
    t0 = w(w(x0 + x4) << 13)
    t1 = w(w(x0 - x4) << 13)
    t10, t13, t11, t12 = w(t0 + t3), w(t0 - t3), w(t1 + t2), w(t1 - t2)
    a0, a1, a2, a3 = x7, x5, x3, x1
    z1, z2, z3, z4 = w(a0 + a3), w(a1 + a2), w(a0 + a2), w(a1 + a3)
    z5 = w(w(z3 + z4) * 9633)
    a0, a1, a2, a3 = w(a0 * 2446), w(a1 * 16819), w(a2 * 25172), w(a3 * 12299)
    z1, z2 = w(z1 * -7373), w(z2 * -20995)
    z3, z4 = w(w(z3 * -16069) + z5), w(w(z4 * -3196) + z5)
    a0, a1, a2, a3 = w(a0 + w(z1 + z3)), w(a1 + w(z2 + z4)), w(a2 + w(z2 + z3)), w(a3 + w(z1 + z4))
    return np.stack([w(t10 + a3), w(t11 + a2), w(t12 + a1), w(t13 + a0), w(t13 - a0), w(t12 - a1), w(t11 - a2), w(t10 - a3)])


def _descale(x, n):
    return _i32(x + (1 << (n - 1))) >> n


def idct_blocks(coef, qt, faults=()):
    """coef int16 [..., 64] natural order, qt int16 [64] -> uint8 [..., 8, 8]; also returns whether every dequantised
    coefficient fits int16 (the range in which equality with the library is claimed)"""
    deq = coef.astype(np.int64) * qt.astype(np.int64)
    fits = bool(np.all((deq >= -32768) & (deq <= 32767)))
    x = deq.reshape(coef.shape[:-1] + (8, 8))
    a1, a2 = (-1, -2) if "transpose" in faults else (-2, -1)
    ws = _descale(_pass(np.moveaxis(x, a1, 0)), 11)            # columns: the transform runs down the rows, axis -2
    ws = np.moveaxis(ws, 0, a1)
    y = _descale(_pass(np.moveaxis(ws, a2, 0)), 18)            # rows
    y = np.moveaxis(y, 0, a2)
    return np.clip(y + 128, 0, 255).astype(np.uint8), fits


def planes_from_coef(buf, width, height, sampling, faults=()):
    """the component planes (uint8, MCU-padded) of one frame's coefficient buffer, and the int16-range flag"""
    blocks = geometry(width, height, sampling)
    planes, off, fits = [], QT_ELEMS, True
    for c, (bw, bh) in enumerate(blocks):
        if bw * bh == 0:
            continue
        co = buf[off:off + 64 * bw * bh].reshape(bh, bw, 64)
        off += 64 * bw * bh
        px, f = idct_blocks(co, buf[64 * c:64 * c + 64], faults)
        fits = fits and f
        planes.append(px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return planes, fits


# ---------------------------------------------------------------------------------------------------- stage 3: upsampling
def _h2v1(p, faults=()):
    p = p.astype(np.int32)
    h, w = p.shape
    out = np.empty((h, 2 * w), dtype=np.int32)
    left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0] = p[:, 0]
    out[:, -1] = p[:, -1]
    return out


def _h2v2(p, faults=()):
    p = p.astype(np.int32)
    h, w = p.shape
    above = np.concatenate([p[:1], p[:-1]], axis=0)
    below = np.concatenate([p[1:], p[-1:]], axis=0)
    out = np.empty((2 * h, 2 * w), dtype=np.int32)
    ra, rb = (7, 8) if "round78" in faults else (8, 7)
    for v, far in ((0, above), (1, below)):
        c = 3 * p + far
        left = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
        right = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
        e = (3 * c + left + ra) >> 4
        o = (3 * c + right + rb) >> 4
        e[:, 0] = (4 * c[:, 0] + ra) >> 4
        o[:, -1] = (4 * c[:, -1] + rb) >> 4
        out[v::2, 0::2] = e
        out[v::2, 1::2] = o
    return out


def upsample(plane, width, height, sampling, faults=()):
    """a chroma plane (MCU-padded) -> int32 [height, width]"""
    hs, vs = (2 if sampling >= S422 else 1), (2 if sampling == S420 else 1)
    cw, ch = -(-width // hs), -(-height // vs)
    p = plane if "edge" in faults else plane[:ch, :cw]
    if hs == 1:
        out = p.astype(np.int32)
    elif cw <= 2:
        out = np.repeat(np.repeat(p.astype(np.int32), hs, axis=1), vs, axis=0)
    elif vs == 1:
        out = _h2v1(p, faults)
    else:
        out = _h2v2(p, faults)
    return out[:height, :width]


# ---------------------------------------------------------------------------------------------------- stage 4: colour
def to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def reconstruct(buf, width, height, sampling, faults=(), want_fits=False):
    """one frame's coefficient buffer -> uint8 RGB [height, width, 3]"""
    planes, fits = planes_from_coef(buf, width, height, sampling, faults)
    y = planes[0][:height, :width]
    if sampling == GRAY:
        rgb = np.repeat(y[:, :, None], 3, axis=2)
    else:
        rgb = to_rgb(y, upsample(planes[1], width, height, sampling, faults), upsample(planes[2], width, height, sampling, faults))
    return (rgb, fits) if want_fits else rgb


def decode(data, faults=()):
    """JPEG bytes -> uint8 RGB [H, W, 3]; asserts the range in which equality with the library is claimed"""
    h, buf = entropy_decode(data)
    rgb, fits = reconstruct(buf, h.width, h.height, h.sampling, faults, want_fits=True)
    assert fits, "a dequantised coefficient outside int16"
    return rgb
