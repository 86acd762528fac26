// Detection overlay of the demo (mega/pytorch_amd/demo.py defines it; tests/overlay_twin.py is its numpy twin): draws the
// detections of F frames in place on the ORIGINAL-size uint8 frames, on the device.
//
// Phase A, overlay_select_kernel, one 256-thread workgroup per frame: the frame's draw list.
//   kept rows: i < counts[f] and score > thr (strict); draw order: score descending, equal scores by ascending row;
//   box in the original frame: (int)clamp(trunc(x * sx)), one f32 multiply each (built with -ffp-contract=off), clamp to
//     +-2^30; a row is dropped when its box is degenerate (x1 < x0 or y1 < y0), lies wholly outside the image or its
//     class is outside [0, NC);
//   label text: the class's glyphs (class_glyphs row, up to the first entry outside [0, G)), then ": D.DD" where DDD =
//     min(rint(double(score) * 100), 999): the product is exact, so the digits are those of "%.2f" for scores in [0, 1];
//   label rectangle: tw = sum of the advances wide, gh high; ly = y0 - gh, or max(y0, 0) when that is < 0;
//     lx = max(min(x0, W - tw), 0).
// Phase B, overlay_draw_kernel, one workgroup per 64 x 16 pixel tile of a frame: the tile culls the draw list (an
//   entry's outline ring and its label rectangle are tested separately) into LDS in draw order; a tile nothing touches
//   returns there.  Each thread owns 4 pixels of one column (lanes run along the row).  A pixel takes the LAST label
//   that covers it, else the LAST outline: all outlines are drawn in order, then all labels.  The outline of thickness
//   t = 2h + 1 is the outer rectangle [x0-h, x1+h] x [y0-h, y1+h] minus the open interior (x0+h, x1-h) x (y0+h, y1-h).
//   A label pixel is the class colour c blended with white by the glyph coverage a: (c (255 - a) + 255 a + 127) / 255.
//   Neither case needs the old pixel: the kernel reads no pixel and writes only the covered ones (byte stores, contiguous
//   across the lanes of a row).
#include "common.h"

namespace {

constexpr int OV_THREADS = 256;
constexpr int OV_MAX_R = 512;
constexpr int OV_MAX_NAME = 18;
constexpr int OV_MAX_TEXT = OV_MAX_NAME + 6;      // ": D.DD"
constexpr int OV_TILE_W = 64;
constexpr int OV_TILE_H = 16;
constexpr int OV_ROWS = OV_TILE_H / (OV_THREADS / 64);      // pixels per thread
constexpr float OV_COORD_MAX = 1073741824.0f;

struct OvEntry {             // 112 bytes
  int x0, y0, x1, y1;        // the box in the original frame
  int lx, ly, tw;            // label rectangle: columns [lx, lx + tw), rows [ly, ly + gh)
  int cls, n;                // class, glyphs in the label
  unsigned char glyph[OV_MAX_TEXT];
  unsigned short cum[OV_MAX_TEXT];      // first column of glyph k within the rectangle
  int pad;
};
static_assert(sizeof(OvEntry) == 112, "OvEntry layout");

inline size_t ov_align(size_t x) { return (x + 255) / 256 * 256; }

__device__ __forceinline__ int ov_coord(float v, float ratio) {
  const float s = v * ratio;
  return (int)fminf(fmaxf(truncf(s), -OV_COORD_MAX), OV_COORD_MAX);
}

__global__ __launch_bounds__(OV_THREADS) void overlay_select_kernel(
    const float4* __restrict__ boxes, const float* __restrict__ scores, const void* __restrict__ labels, int labels_i64,
    const int* __restrict__ counts, int R, int H, int W, float sx, float sy, float thr, int NC,
    const int* __restrict__ class_glyphs, int ML, const int* __restrict__ fmt_glyphs, const int* __restrict__ adv, int G,
    int gh, OvEntry* __restrict__ entries, int* __restrict__ n_draw) {
  __shared__ float sh_score[OV_MAX_R];
  __shared__ unsigned char sh_draw[OV_MAX_R];
  __shared__ int sh_n;
  const int f = blockIdx.x;
  const int cnt = min(max(counts[f], 0), R);
  if (threadIdx.x == 0) sh_n = 0;
  // pass 1: which rows are drawn (own row only), the integer box
  int bx0[2], by0[2], bx1[2], by1[2], cl[2];
  for (int k = 0; k < 2; ++k) {
    const int i = threadIdx.x + k * OV_THREADS;
    bool draw = false;
    float s = 0.0f;
    if (i < cnt) {
      s = scores[(size_t)f * R + i];
      if (s > thr) {
        const float4 b = boxes[(size_t)f * R + i];
        bx0[k] = ov_coord(b.x, sx);
        by0[k] = ov_coord(b.y, sy);
        bx1[k] = ov_coord(b.z, sx);
        by1[k] = ov_coord(b.w, sy);
        const long long c = labels_i64 ? ((const long long*)labels)[(size_t)f * R + i]
                                       : (long long)((const int*)labels)[(size_t)f * R + i];
        cl[k] = (int)c;
        draw = bx1[k] >= bx0[k] && by1[k] >= by0[k] && bx1[k] >= 0 && by1[k] >= 0 && bx0[k] < W && by0[k] < H &&
               c >= 0 && c < NC;
      }
    }
    if (i < OV_MAX_R) {
      sh_score[i] = s;
      sh_draw[i] = draw ? 1 : 0;
    }
  }
  __syncthreads();
  // pass 2: position in draw order among the drawn rows, then the entry
  for (int k = 0; k < 2; ++k) {
    const int i = threadIdx.x + k * OV_THREADS;
    if (i >= cnt || !sh_draw[i]) continue;
    const float s = sh_score[i];
    int pos = 0;
    for (int j = 0; j < cnt; ++j) {
      const float sj = sh_score[j];
      pos += (sh_draw[j] && (sj > s || (sj == s && j < i))) ? 1 : 0;
    }
    atomicAdd(&sh_n, 1);
    OvEntry e;
    e.x0 = bx0[k]; e.y0 = by0[k]; e.x1 = bx1[k]; e.y1 = by1[k];
    e.cls = cl[k];
    e.pad = 0;
    int n = 0, tw = 0;
    for (int q = 0; q < OV_MAX_TEXT; ++q) { e.glyph[q] = 0; e.cum[q] = 0; }
    for (int q = 0; q < ML && q < OV_MAX_NAME; ++q) {
      const int g = class_glyphs[cl[k] * ML + q];
      if (g < 0 || g >= G) break;
      e.glyph[n] = (unsigned char)g;
      e.cum[n] = (unsigned short)min(tw, 65535);
      tw += max(adv[g], 0);
      ++n;
    }
    const double v = rint((double)s * 100.0);      // exact product, round half to even: the digits of "%.2f"
    const int iv = (int)fmin(v, 999.0);
    const int tail[6] = {fmt_glyphs[10], fmt_glyphs[11], fmt_glyphs[iv / 100], fmt_glyphs[12], fmt_glyphs[iv / 10 % 10],
                         fmt_glyphs[iv % 10]};
    for (int q = 0; q < 6; ++q) {
      const int g = min(max(tail[q], 0), G - 1);
      e.glyph[n] = (unsigned char)g;
      e.cum[n] = (unsigned short)min(tw, 65535);
      tw += max(adv[g], 0);
      ++n;
    }
    e.n = n;
    e.tw = min(tw, 65535);
    int ly = e.y0 - gh;
    if (ly < 0) ly = max(e.y0, 0);
    e.ly = ly;
    e.lx = max(min(e.x0, W - e.tw), 0);
    entries[(size_t)f * R + pos] = e;
  }
  __syncthreads();
  if (threadIdx.x == 0) n_draw[f] = sh_n;
}

__global__ __launch_bounds__(OV_THREADS) void overlay_draw_kernel(
    unsigned char* __restrict__ frames, int H, int W, int R, int half, const unsigned char* __restrict__ palette,
    const unsigned char* __restrict__ cov, int gh, int gw, const OvEntry* __restrict__ entries,
    const int* __restrict__ n_draw) {
  __shared__ unsigned char sh_flag[OV_MAX_R];
  __shared__ unsigned short sh_list[OV_MAX_R];      // the entries that touch the tile, in draw order
  __shared__ unsigned char sh_lflag[OV_MAX_R];      // bit 0: its outline does, bit 1: its label rectangle does
  __shared__ int sh_cnt;
  const int f = blockIdx.z;
  const int n = min(n_draw[f], R);
  const OvEntry* __restrict__ ent = entries + (size_t)f * R;
  const int tx0 = blockIdx.x * OV_TILE_W, ty0 = blockIdx.y * OV_TILE_H;
  const int tx1 = min(tx0 + OV_TILE_W, W) - 1, ty1 = min(ty0 + OV_TILE_H, H) - 1;      // inclusive
  int any = 0;
  for (int e = threadIdx.x; e < n; e += OV_THREADS) {
    const OvEntry& E = ent[e];
    const int x0 = E.x0, y0 = E.y0, x1 = E.x1, y1 = E.y1;
    int fl = 0;
    // outline ring: the tile meets the outer rectangle and does not lie inside the open interior
    if (tx0 <= x1 + half && tx1 >= x0 - half && ty0 <= y1 + half && ty1 >= y0 - half &&
        !(tx0 > x0 + half && tx1 < x1 - half && ty0 > y0 + half && ty1 < y1 - half))
      fl |= 1;
    if (tx0 < E.lx + E.tw && tx1 >= E.lx && ty0 < E.ly + gh && ty1 >= E.ly) fl |= 2;
    sh_flag[e] = (unsigned char)fl;
    any |= fl;
  }
  if (!__syncthreads_or(any)) return;      // nothing of this frame touches the tile
  if (threadIdx.x < 64) {                  // ordered compaction by one wave
    int c = 0;
    for (int base = 0; base < n; base += 64) {
      const int e = base + (int)threadIdx.x;
      const int fl = e < n ? sh_flag[e] : 0;
      const unsigned long long m = __ballot(fl != 0);
      if (fl) {
        const int p = c + __popcll(m & ((1ull << threadIdx.x) - 1ull));
        sh_list[p] = (unsigned short)e;
        sh_lflag[p] = (unsigned char)fl;
      }
      c += __popcll(m);
    }
    if (threadIdx.x == 0) sh_cnt = c;
  }
  __syncthreads();
  const int m = sh_cnt;
  const int px = tx0 + (int)(threadIdx.x & 63);
  const int row0 = ty0 + (int)(threadIdx.x >> 6);
  if (px >= W) return;
  int oc[OV_ROWS], le[OV_ROWS];      // class of the last outline, entry of the last label (-1: none)
  for (int r = 0; r < OV_ROWS; ++r) { oc[r] = -1; le[r] = -1; }
  for (int q = 0; q < m; ++q) {
    const int e = sh_list[q], fl = sh_lflag[q];
    const OvEntry& E = ent[e];
    if (fl & 1) {
      const int x0 = E.x0, y0 = E.y0, x1 = E.x1, y1 = E.y1, cls = E.cls;
      const bool in_x = px >= x0 - half && px <= x1 + half;
      const bool deep_x = px > x0 + half && px < x1 - half;
      for (int r = 0; r < OV_ROWS; ++r) {
        const int py = row0 + r * (OV_THREADS / 64);
        const bool hit = in_x && py >= y0 - half && py <= y1 + half && !(deep_x && py > y0 + half && py < y1 - half);
        oc[r] = hit ? cls : oc[r];
      }
    }
    if (fl & 2) {
      const int lx = E.lx, ly = E.ly, tw = E.tw;
      const bool in_x = px >= lx && px < lx + tw;
      for (int r = 0; r < OV_ROWS; ++r) {
        const int py = row0 + r * (OV_THREADS / 64);
        le[r] = (in_x && py >= ly && py < ly + gh) ? e : le[r];
      }
    }
  }
  unsigned char* __restrict__ img = frames + (size_t)f * H * W * 3;
  for (int r = 0; r < OV_ROWS; ++r) {
    const int py = row0 + r * (OV_THREADS / 64);
    if (py >= H) continue;
    int c0, c1, c2;
    if (le[r] >= 0) {
      const OvEntry& E = ent[le[r]];
      const int u = px - E.lx;
      int k = 0;
      for (int q = 1; q < E.n; ++q) k = (int)E.cum[q] <= u ? q : k;      // cum ascends: the last glyph starting at or before u
      const int col = u - (int)E.cum[k];
      const int a = col < gw ? (int)cov[((size_t)E.glyph[k] * gh + (py - E.ly)) * gw + col] : 0;
      const unsigned char* pc = palette + E.cls * 3;
      c0 = (pc[0] * (255 - a) + 255 * a + 127) / 255;
      c1 = (pc[1] * (255 - a) + 255 * a + 127) / 255;
      c2 = (pc[2] * (255 - a) + 255 * a + 127) / 255;
    } else if (oc[r] >= 0) {
      const unsigned char* pc = palette + oc[r] * 3;
      c0 = pc[0]; c1 = pc[1]; c2 = pc[2];
    } else {
      continue;
    }
    unsigned char* p = img + ((size_t)py * W + px) * 3;
    p[0] = (unsigned char)c0;
    p[1] = (unsigned char)c1;
    p[2] = (unsigned char)c2;
  }
}

}  // namespace

extern "C" size_t mega_overlay_detections_workspace_bytes(int F, int R) {
  if (F <= 0 || R <= 0) return 0;
  return ov_align((size_t)F * R * sizeof(OvEntry)) + ov_align((size_t)F * sizeof(int));
}

extern "C" int mega_overlay_detections(unsigned char* frames, int F, int H, int W, const float* boxes, const float* scores,
                                       const void* labels, int labels_i64, const int* counts, int R, float sx, float sy,
                                       float thr, int thickness, const unsigned char* palette, int NC,
                                       const int* class_glyphs, int ML, const int* fmt_glyphs, const unsigned char* cov,
                                       const int* adv, int G, int gh, int gw, int select_only, void* ws, size_t ws_bytes,
                                       void* stream) {
  mega_clear_error();
  if (F <= 0 || H <= 0 || W <= 0 || R < 0 || NC <= 0 || ML <= 0 || G <= 0 || gh <= 0 || gw <= 0) return MEGA_ERR_ARG;
  if (thickness < 1 || (thickness & 1) == 0) return MEGA_ERR_ARG;
  if (!(sx > 0.0f) || !(sy > 0.0f) || thr != thr) return MEGA_ERR_ARG;
  if (R > OV_MAX_R || ML > OV_MAX_NAME || G > 256 || F > 65535 || thickness > 255) return MEGA_ERR_LIMIT;
  if (R == 0) return MEGA_OK;
  if (!frames || !boxes || !scores || !labels || !counts || !palette || !class_glyphs || !fmt_glyphs || !cov || !adv || !ws)
    return MEGA_ERR_ARG;
  if (ws_bytes < mega_overlay_detections_workspace_bytes(F, R)) return MEGA_ERR_WS;
  OvEntry* entries = (OvEntry*)ws;
  int* n_draw = (int*)((unsigned char*)ws + ov_align((size_t)F * R * sizeof(OvEntry)));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(overlay_select_kernel, dim3(F), dim3(OV_THREADS), 0, st, (const float4*)boxes, scores, labels,
                     labels_i64, counts, R, H, W, sx, sy, thr, NC, class_glyphs, ML, fmt_glyphs, adv, G, gh, entries,
                     n_draw);
  if (!select_only)
    hipLaunchKernelGGL(overlay_draw_kernel, dim3(cdiv(W, OV_TILE_W), cdiv(H, OV_TILE_H), F), dim3(OV_THREADS), 0, st,
                       frames, H, W, R, thickness / 2, palette, cov, gh, gw, entries, n_draw);
  return mega_check_launch();
}
