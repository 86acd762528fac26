// Host half of the device JPEG decode (mega/pytorch_amd/jpeg.py defines it; tests/jpeg_twin.py is its numpy twin): marker
// parsing and sequential Huffman entropy decoding of a baseline JPEG into raw int16 DCT coefficients.  Plain C++17, no HIP
// and no allocation: jpeg.hip wraps the two functions as C-ABI entry points, tools/jpeg_entropy_check.cpp compiles this
// header alone.
//
// Accepted: SOF0 / SOF1, 8-bit samples, one interleaved scan over all components (Ss = 0, Se = 63, Ah = Al = 0), 1 component
// or 3 components with Y sampled 1x1, 2x1 or 2x2 and Cb = Cr = 1x1, 8-bit DQT entries, DRI / RSTn.  Everything else --
// progressive, arithmetic or lossless frames, a scan over fewer components than the frame has, 16-bit tables, 4 components, an
// Adobe segment whose transform is not 1 on 3 components, component ids R, G, B without a JFIF or Adobe segment, any other
// sampling -- is JPG_UNSUPPORTED; a stream that breaks the syntax (bad Huffman code, coefficient index past 63, missing or
// misnumbered RSTn, data that ends before the last MCU, a table that is used but never defined) is JPG_CORRUPT.
//
// Every read is bounds-checked against [data, data + nbytes) and every write against the caller's element count; the
// decoder writes EVERY element of [0, coef_elems) of its output (a block is zeroed before its coefficients land), so the
// result does not depend on what the buffer held.
//
// Output layout (int16): qt[3][64] -- the quantisation table of component 0, 1, 2 in natural (row-major) order, zeros for a
// component the image does not have -- then one coefficient plane per component, [block row][block col][64] over the
// MCU-padded block grid, each block in natural order, NOT dequantised.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace mega_jpeg {

enum { JPG_OK = 0, JPG_UNSUPPORTED = 1, JPG_CORRUPT = 2 };

// sampling codes: how Y is sampled relative to Cb / Cr
enum { SAMP_GRAY = 0, SAMP_444 = 1, SAMP_422 = 2, SAMP_420 = 3 };

// info[]: 0 width, 1 height, 2 components, 3 sampling code, 4 + 2c / 5 + 2c blocks per row / column of component c (0 for a
// component the image does not have), 10 restart interval in MCUs (0: none), 11 int16 elements of the decode's output
constexpr int INFO_INTS = 12;
constexpr int QT_ELEMS = 3 * 64;

// the block grid of every component from the frame size and the sampling code alone; false for values outside the set
static inline bool geometry(int W, int H, int sampling, int bw[3], int bh[3]) {
  if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || sampling < SAMP_GRAY || sampling > SAMP_420) return false;
  const int hs = sampling >= SAMP_422 ? 2 : 1, vs = sampling == SAMP_420 ? 2 : 1;
  const int mx = (W + 8 * hs - 1) / (8 * hs), my = (H + 8 * vs - 1) / (8 * vs);
  bw[0] = mx * hs;
  bh[0] = my * vs;
  bw[1] = bw[2] = sampling == SAMP_GRAY ? 0 : mx;
  bh[1] = bh[2] = sampling == SAMP_GRAY ? 0 : my;
  return true;
}

static inline long long coef_elems(const int bw[3], const int bh[3]) {
  long long n = QT_ELEMS;
  for (int c = 0; c < 3; ++c) n += 64ll * bw[c] * bh[c];
  return n;
}

static const unsigned char NATURAL_ORDER[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int LOOK_BITS = 9;

struct HuffTable {
  bool defined = false;
  unsigned char bits[17];
  unsigned char vals[256];
  // derived: codes of up to LOOK_BITS bits resolve in one table read ((length << 8) | symbol, 0 = longer code); longer ones
  // through the per-length code ranges
  uint16_t look[1 << LOOK_BITS];
  int32_t maxcode[18];      // largest code of each length, -1 if none; [17] is a sentinel that ends the search
  int32_t valoff[17];       // vals index of a code = code + valoff[length]
};

// false if the counts do not describe a prefix code
static inline bool derive(HuffTable& t) {
  int code = 0, p = 0;
  memset(t.look, 0, sizeof(t.look));
  for (int l = 1; l <= 16; ++l) {
    const int n = t.bits[l];
    if (n == 0) {
      t.maxcode[l] = -1;
      t.valoff[l] = 0;
    } else {
      if (code + n > (1 << l)) return false;
      t.valoff[l] = p - code;
      if (l <= LOOK_BITS) {
        for (int i = 0; i < n; ++i) {
          const int first = (code + i) << (LOOK_BITS - l);
          for (int f = 0; f < (1 << (LOOK_BITS - l)); ++f) t.look[first + f] = (uint16_t)((l << 8) | t.vals[p + i]);
        }
      }
      p += n;
      code += n;
      t.maxcode[l] = code - 1;
    }
    code <<= 1;
  }
  t.maxcode[17] = 0x7fffffff;
  return true;
}

struct Component {
  int id, h, v, tq, td, ta;
};

struct Header {
  int width = 0, height = 0, ncomp = 0, sampling = 0, restart = 0;
  int bw[3], bh[3];
  Component comp[3];
  bool qt_defined[4] = {false, false, false, false};
  unsigned char qt[4][64];      // zigzag order, as the stream stores them
  HuffTable dc[4], ac[4];
  size_t scan = 0;              // first byte of the entropy-coded data
};

static inline void fill_info(const Header& h, int* info) {
  info[0] = h.width;
  info[1] = h.height;
  info[2] = h.ncomp;
  info[3] = h.sampling;
  for (int c = 0; c < 3; ++c) {
    info[4 + 2 * c] = h.bw[c];
    info[5 + 2 * c] = h.bh[c];
  }
  info[10] = h.restart;
  info[11] = (int)coef_elems(h.bw, h.bh);
}

// Markers up to and including the SOS header.  The Huffman tables are not derived here (the probe does not need them).
static inline int parse_header(const unsigned char* d, size_t n, Header& hd) {
  if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return JPG_UNSUPPORTED;      // not a JPEG at all
  size_t p = 2;
  bool sof = false, jfif = false, adobe = false;
  int adobe_transform = -1;
  for (;;) {
    if (p + 2 > n) return JPG_CORRUPT;
    if (d[p] != 0xFF) return JPG_CORRUPT;
    while (p < n && d[p] == 0xFF) ++p;      // fill bytes
    if (p >= n) return JPG_CORRUPT;
    const int m = d[p++];
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;      // stand-alone
    if (m == 0xD8 || m == 0xD9 || m == 0x00) return JPG_CORRUPT;
    if (p + 2 > n) return JPG_CORRUPT;
    const size_t len = ((size_t)d[p] << 8) | d[p + 1];
    if (len < 2 || p + len > n) return JPG_CORRUPT;
    const unsigned char* s = d + p + 2;
    const size_t sl = len - 2;
    p += len;
    if (m == 0xC0 || m == 0xC1) {
      if (sof) return JPG_CORRUPT;
      if (sl < 6) return JPG_CORRUPT;
      if (s[0] != 8) return JPG_UNSUPPORTED;
      hd.height = (s[1] << 8) | s[2];
      hd.width = (s[3] << 8) | s[4];
      hd.ncomp = s[5];
      if (hd.ncomp != 1 && hd.ncomp != 3) return JPG_UNSUPPORTED;
      if (hd.width == 0 || hd.height == 0) return JPG_UNSUPPORTED;      // (a height of 0 defers to a DNL segment)
      if (sl != (size_t)6 + 3 * hd.ncomp) return JPG_CORRUPT;
      for (int c = 0; c < hd.ncomp; ++c) {
        Component& k = hd.comp[c];
        k.id = s[6 + 3 * c];
        k.h = s[7 + 3 * c] >> 4;
        k.v = s[7 + 3 * c] & 15;
        k.tq = s[8 + 3 * c];
        if (k.h < 1 || k.h > 4 || k.v < 1 || k.v > 4) return JPG_CORRUPT;
        if (k.tq > 3) return JPG_CORRUPT;
      }
      if (hd.ncomp == 1) {
        hd.sampling = SAMP_GRAY;      // a one-component scan is never interleaved: its factors do not matter (A.2.2)
      } else {
        if (hd.comp[1].h != 1 || hd.comp[1].v != 1 || hd.comp[2].h != 1 || hd.comp[2].v != 1) return JPG_UNSUPPORTED;
        const int h = hd.comp[0].h, v = hd.comp[0].v;
        if (h == 1 && v == 1) hd.sampling = SAMP_444;
        else if (h == 2 && v == 1) hd.sampling = SAMP_422;
        else if (h == 2 && v == 2) hd.sampling = SAMP_420;
        else return JPG_UNSUPPORTED;
      }
      sof = true;
    } else if ((m >= 0xC2 && m <= 0xCF) && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      return JPG_UNSUPPORTED;      // progressive, lossless, differential, arithmetic frames
    } else if (m == 0xCC) {
      return JPG_UNSUPPORTED;      // arithmetic conditioning
    } else if (m == 0xC4) {
      size_t q = 0;
      while (q < sl) {
        if (q + 17 > sl) return JPG_CORRUPT;
        const int tc = s[q] >> 4, th = s[q] & 15;
        if (tc > 1 || th > 3) return JPG_CORRUPT;
        HuffTable& t = tc ? hd.ac[th] : hd.dc[th];
        int cnt = 0;
        t.bits[0] = 0;
        for (int l = 1; l <= 16; ++l) {
          t.bits[l] = s[q + l];
          cnt += s[q + l];
        }
        if (cnt > 256 || q + 17 + cnt > sl) return JPG_CORRUPT;
        memset(t.vals, 0, sizeof(t.vals));
        memcpy(t.vals, s + q + 17, cnt);
        t.defined = true;
        q += 17 + cnt;
      }
    } else if (m == 0xDB) {
      size_t q = 0;
      while (q < sl) {
        const int pq = s[q] >> 4, tq = s[q] & 15;
        if (pq == 1) return JPG_UNSUPPORTED;      // 16-bit entries
        if (pq != 0 || tq > 3) return JPG_CORRUPT;
        if (q + 65 > sl) return JPG_CORRUPT;
        memcpy(hd.qt[tq], s + q + 1, 64);
        hd.qt_defined[tq] = true;
        q += 65;
      }
    } else if (m == 0xDD) {
      if (sl != 2) return JPG_CORRUPT;
      hd.restart = (s[0] << 8) | s[1];
    } else if (m == 0xE0) {
      if (sl >= 5 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) {
        adobe = true;
        adobe_transform = s[11];
      }
    } else if (m == 0xDA) {
      if (!sof) return JPG_CORRUPT;
      if (sl < 1) return JPG_CORRUPT;
      const int ns = s[0];
      if (ns < 1 || ns > 4 || sl != (size_t)4 + 2 * ns) return JPG_CORRUPT;
      if (ns != hd.ncomp) return JPG_UNSUPPORTED;      // one scan per component: several scans
      for (int c = 0; c < ns; ++c) {
        if (s[1 + 2 * c] != hd.comp[c].id) return JPG_UNSUPPORTED;      // another interleaving order than the frame's
        hd.comp[c].td = s[2 + 2 * c] >> 4;
        hd.comp[c].ta = s[2 + 2 * c] & 15;
        if (hd.comp[c].td > 3 || hd.comp[c].ta > 3) return JPG_CORRUPT;
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return JPG_UNSUPPORTED;
      hd.scan = p;
      break;
    }
    // every other segment (APPn, COM, DNL, ...) is skipped
  }
  if (hd.ncomp == 3) {
    if (adobe && adobe_transform != 1) return JPG_UNSUPPORTED;
    if (!jfif && !adobe && hd.comp[0].id == 'R' && hd.comp[1].id == 'G' && hd.comp[2].id == 'B') return JPG_UNSUPPORTED;
  }
  if (!geometry(hd.width, hd.height, hd.sampling, hd.bw, hd.bh)) return JPG_UNSUPPORTED;
  if (coef_elems(hd.bw, hd.bh) > 0x7fffffffll) return JPG_UNSUPPORTED;
  for (int c = 0; c < hd.ncomp; ++c) {
    if (!hd.qt_defined[hd.comp[c].tq] || !hd.dc[hd.comp[c].td].defined || !hd.ac[hd.comp[c].ta].defined) return JPG_CORRUPT;
  }
  return JPG_OK;
}

// The entropy-coded segment as a bit stream: FF 00 is a data byte FF; any other FF xx is a marker, which the reader never
// passes -- from there on it supplies zero bits and counts them, so a decode that has used padding bits can be told.
struct BitReader {
  const unsigned char* d;
  size_t pos, end;
  uint64_t buf = 0;
  int nbits = 0;      // bits in buf, real and padding
  int pad = 0;        // how many of them are padding (always the last ones)
  bool stopped = false;

  BitReader(const unsigned char* data, size_t start, size_t n) : d(data), pos(start), end(n) {}

  inline void fill() {
    while (nbits <= 56) {
      unsigned b = 0;
      if (!stopped) {
        if (pos >= end) {
          stopped = true;
        } else if (d[pos] != 0xFF) {
          b = d[pos++];
        } else if (pos + 1 < end && d[pos + 1] == 0x00) {
          b = 0xFF;
          pos += 2;
        } else {
          stopped = true;      // a marker, or a lone FF at the end of the data
        }
      }
      if (stopped) pad += 8;
      buf = (buf << 8) | b;
      nbits += 8;
    }
  }
  inline unsigned peek(int n) { return (unsigned)((buf >> (nbits - n)) & ((1u << n) - 1u)); }      // n in [1, 16], n <= nbits
  inline void drop(int n) { nbits -= n; }
  inline bool overrun() const { return nbits < pad; }
  inline void reset() {
    buf = 0;
    nbits = 0;
    pad = 0;
    stopped = false;
  }
};

// one Huffman symbol, -1 for a code of more than 16 bits
static inline int decode_symbol(BitReader& br, const HuffTable& t) {
  if (br.nbits < 16) br.fill();
  const unsigned e = t.look[br.peek(LOOK_BITS)];
  if (e) {
    br.drop(e >> 8);
    return e & 255;
  }
  const int code16 = (int)br.peek(16);
  int l = LOOK_BITS + 1;
  while (l <= 16 && (code16 >> (16 - l)) > t.maxcode[l]) ++l;
  if (l > 16) return -1;
  const int idx = (code16 >> (16 - l)) + t.valoff[l];
  if (idx < 0 || idx > 255) return -1;
  br.drop(l);
  return t.vals[idx];
}

// the next s bits (s in [1, 15]) as the signed value of category s
static inline int receive_extend(BitReader& br, int s) {
  if (br.nbits < s) br.fill();
  const int v = (int)br.peek(s);
  br.drop(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

static inline int probe(const unsigned char* data, long long nbytes, int* info) {
  if (!data || !info || nbytes <= 0) return JPG_UNSUPPORTED;
  Header hd;
  const int rc = parse_header(data, (size_t)nbytes, hd);
  if (rc != JPG_OK) return rc;
  fill_info(hd, info);
  return JPG_OK;
}

// expect: the probe's info of the stream this one must agree with in size, component count and sampling (entries 0 to 3;
// the rest follows from them).  out_elems: capacity of out in int16 elements, at least expect[11].
static inline int entropy_decode(const unsigned char* data, long long nbytes, const int* expect, int16_t* out,
                                 long long out_elems) {
  if (!data || !expect || !out || nbytes <= 0) return JPG_UNSUPPORTED;
  Header hd;
  int rc = parse_header(data, (size_t)nbytes, hd);
  if (rc != JPG_OK) return rc;
  if (hd.width != expect[0] || hd.height != expect[1] || hd.ncomp != expect[2] || hd.sampling != expect[3])
    return JPG_UNSUPPORTED;
  const long long total = coef_elems(hd.bw, hd.bh);
  if (out_elems < total) return JPG_UNSUPPORTED;
  for (int c = 0; c < hd.ncomp; ++c) {
    if (!derive(hd.dc[hd.comp[c].td]) || !derive(hd.ac[hd.comp[c].ta])) return JPG_CORRUPT;
  }
  // tables, natural order
  for (int c = 0; c < 3; ++c) {
    int16_t* q = out + 64 * c;
    if (c < hd.ncomp) {
      for (int k = 0; k < 64; ++k) q[NATURAL_ORDER[k]] = (int16_t)hd.qt[hd.comp[c].tq][k];
    } else {
      memset(q, 0, 64 * sizeof(int16_t));
    }
  }
  int16_t* plane[3];
  long long off = QT_ELEMS;
  for (int c = 0; c < 3; ++c) {
    plane[c] = out + off;
    off += 64ll * hd.bw[c] * hd.bh[c];
  }
  const int hs = hd.sampling >= SAMP_422 ? 2 : 1, vs = hd.sampling == SAMP_420 ? 2 : 1;
  const int mx = hd.bw[0] / hs, my = hd.bh[0] / vs;
  int pred[3] = {0, 0, 0};
  BitReader br(data, hd.scan, (size_t)nbytes);
  long long done = 0;
  int next_rst = 0;
  for (int yy = 0; yy < my; ++yy) {
    for (int xx = 0; xx < mx; ++xx) {
      if (hd.restart > 0 && done > 0 && done % hd.restart == 0) {
        // the interval ended on a byte boundary: at most 7 real bits are left over, and the next two bytes are RSTn
        if (br.overrun() || br.nbits - br.pad >= 8) return JPG_CORRUPT;
        if (br.pos + 2 > br.end || data[br.pos] != 0xFF || data[br.pos + 1] != 0xD0 + next_rst) return JPG_CORRUPT;
        br.pos += 2;
        br.reset();
        next_rst = (next_rst + 1) & 7;
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int c = 0; c < hd.ncomp; ++c) {
        const int ch = c == 0 ? hs : 1, cv = c == 0 ? vs : 1;
        const HuffTable& dct = hd.dc[hd.comp[c].td];
        const HuffTable& act = hd.ac[hd.comp[c].ta];
        for (int v = 0; v < cv; ++v) {
          for (int h = 0; h < ch; ++h) {
            int16_t* blk = plane[c] + 64 * ((long long)(yy * cv + v) * hd.bw[c] + (xx * ch + h));
            memset(blk, 0, 64 * sizeof(int16_t));
            int s = decode_symbol(br, dct);
            if (s < 0 || s > 11) return JPG_CORRUPT;
            if (s) pred[c] += receive_extend(br, s);
            blk[0] = (int16_t)pred[c];
            for (int k = 1; k < 64;) {
              const int rs = decode_symbol(br, act);
              if (rs < 0) return JPG_CORRUPT;
              const int r = rs >> 4;
              s = rs & 15;
              if (s) {
                k += r;
                if (k > 63) return JPG_CORRUPT;
                blk[NATURAL_ORDER[k]] = (int16_t)receive_extend(br, s);
                ++k;
              } else if (r == 15) {
                k += 16;
                if (k > 63) return JPG_CORRUPT;      // a run of zeros must be followed by a coefficient
              } else if (r == 0) {
                break;      // end of block
              } else {
                return JPG_CORRUPT;      // EOBn belongs to progressive scans
              }
            }
            if (br.overrun()) return JPG_CORRUPT;      // the data ended inside this block
          }
        }
      }
      ++done;
    }
  }
  return JPG_OK;
}

}  // namespace mega_jpeg
