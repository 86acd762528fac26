// Detection error diagnosis: every detection's kind (TP / DUPE / LOC / CLS / BOTH / BKG) with the GT box it is matched
// or attributed to, and per GT box the detections that found or nearly found it, as defined in
// mega/pytorch_amd/diagnose.py (the reference has no counterpart).  The IoU is box_math.h's vid_iou, the detection AP's:
// the prediction rescaled by the frame's ratio in f32, +1 on x2 / y2, then box_iou1.
//
// Built with -ffp-contract=off: every f32 operation of the rescale / IoU rounds on its own, as in vid_eval.hip.
//
// Mapping: one wave per frame (DG_WAVES frames per workgroup; the waves never meet at a barrier).  A frame with at most
// DG_LDS_GT boxes keeps them in the wave's slice of LDS; a larger one reads them from global memory.
//   Pass 1: mega_vid_eval_match's greedy matching for one range and no motion list, serial over the frame's run of
//   `order`; lanes hold GT boxes (chunks of 64, a taken flag per lane and chunk) and reduce the best free candidate.
//   Pass 2: lanes over the frame's detections; each that is no TP scans the frame's GT for a / ga (own label) and b / gb
//   (other labels) and applies the rules in order.
//   Pass 3: lanes over the frame's GT boxes; each scans the frame's detections, in position order, for the TP that took it
//   and the best LOC / CLS detection attributed to it.
// Pass 2 reads pass 1's det_kind and pass 3 reads pass 2's det_kind / det_gt: values the same wave stored, read back after
// a workgroup-scope fence (one CU, one vector L1).  No atomics, no workspace: the same bits on every run.
// Every index read from a device table is checked against the sizes the host passed before it addresses memory; a frame
// whose offsets do not fit is skipped, as is an `order` entry outside its frame's run.
#include "box_math.h"
#include "common.h"
#include "launch.h"

namespace {

constexpr int DG_WAVES = 4;           // frames per 256-thread workgroup
constexpr int DG_LDS_GT = 64;         // GT boxes of a frame kept in LDS: 64 x 20 B per wave
constexpr int DG_MAX_CHUNKS = 64;     // taken flags: one 64-bit word per lane -> at most 64 x 64 GT boxes per frame
constexpr unsigned char DG_TP = 0, DG_DUPE = 1, DG_LOC = 2, DG_CLS = 3, DG_BOTH = 4, DG_BKG = 5;
constexpr unsigned char DG_PENDING = 0xff;      // between pass 1 and pass 2: not a TP

__device__ __forceinline__ float dg_wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ int dg_wave_min(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// The frame's GT boxes: the wave's LDS copy, or global memory for a frame that does not fit.
struct DgGt {
  const float4* box;
  const int* label;
};

// BoxList.resize (x * ratio_w, y * ratio_h in f32), then the evaluation's +1 on x2 / y2: vid_match_kernel's pb
__device__ __forceinline__ float4 dg_pred_box(const float4 b, float rw, float rh) {
  return make_float4(b.x * rw, b.y * rh, b.z * rw + 1.0f, b.w * rh + 1.0f);
}

__global__ __launch_bounds__(64 * DG_WAVES) void diagnose_match_kernel(
    const float4* __restrict__ det_box, const int* __restrict__ det_label, const float* __restrict__ det_score,
    const long long* __restrict__ det_off, const int* __restrict__ order, const float2* __restrict__ ratio,
    const float4* __restrict__ gt_box, const int* __restrict__ gt_label, const long long* __restrict__ gt_off, int F,
    long long N, long long G, int max_gt, float tb, unsigned char* det_kind, int* det_gt, float* __restrict__ det_iou,
    int* __restrict__ gt_det) {
  __shared__ float4 s_box[DG_WAVES][DG_LDS_GT];
  __shared__ int s_label[DG_WAVES][DG_LDS_GT];
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const long long f = (long long)blockIdx.x * DG_WAVES + wave;
  if (f >= F) return;                                     // (wave-uniform, as every branch on a frame's sizes below)
  const float tf = 0.5f;
  long long g0 = gt_off[f], g1 = gt_off[f + 1];
  long long d0 = det_off[f], d1 = det_off[f + 1];
  if (g0 < 0 || g1 > G || g1 < g0 || g1 - g0 > max_gt || d0 < 0 || d1 > N || d1 < d0) return;
  const int n = (int)(g1 - g0);
  const int nch = (n + 63) >> 6;
  const float rw = ratio[f].x, rh = ratio[f].y;

  DgGt gt = {gt_box + g0, gt_label + g0};
  if (n > 0 && n <= DG_LDS_GT) {
    if (lane < n) {
      s_box[wave][lane] = gt_box[g0 + lane];
      s_label[wave][lane] = gt_label[g0 + lane];
    }
    gt.box = s_box[wave];
    gt.label = s_label[wave];
  }
  for (long long i = d0 + lane; i < d1; i += 64) det_kind[i] = DG_PENDING;
  __threadfence_block();

  // ---- pass 1: the greedy matching, in the frame's run of `order` (label, score descending, position descending)
  if (n > 0) {
    unsigned long long taken = 0;                         // bit c: GT box c * 64 + lane is taken
    for (long long i = d0; i < d1; ++i) {
      const int idx = order[i];
      if (idx < d0 || idx >= d1) continue;
      const int L = det_label[idx];
      const float4 pb = dg_pred_box(det_box[idx], rw, rh);
      const float pa = box_area1(pb);
      float bv = -1.0f;                                   // the lane's best free candidate: the lowest chunk on a tie
      int bk = 0x7fffffff;
      for (int c = 0; c < nch; ++c) {
        const int k = c * 64 + lane;
        if (k >= n || ((taken >> c) & 1) || gt.label[k] != L) continue;
        const float v = vid_iou(pb, pa, gt.box[k]);
        if (v >= tf && v > bv) {                          // (false on NaN)
          bv = v;
          bk = k;
        }
      }
      const float mx = dg_wave_max(bv);
      if (mx >= tf) {
        const int chosen = dg_wave_min(bv == mx ? bk : 0x7fffffff);     // the lowest GT index among equals
        if (lane == (chosen & 63)) taken |= 1ull << (chosen >> 6);
        if (lane == 0) {
          det_kind[idx] = DG_TP;
          det_gt[idx] = (int)(g0 + chosen);
          det_iou[idx] = mx;
        }
      }
    }
  }
  __threadfence_block();

  // ---- pass 2: the kind of every other detection
  for (long long i = d0 + lane; i < d1; i += 64) {
    if (det_kind[i] == DG_TP) continue;
    const int L = det_label[i];
    const float4 pb = dg_pred_box(det_box[i], rw, rh);
    const float pa = box_area1(pb);
    float a = -1.0f, b = -1.0f;                           // no threshold is met by "none"
    int ga = -1, gb = -1;
    for (int k = 0; k < n; ++k) {
      const float v = vid_iou(pb, pa, gt.box[k]);
      if (gt.label[k] == L) {
        if (v > a) {                                      // (strict: the lowest index on a tie; false on NaN)
          a = v;
          ga = k;
        }
      } else if (v > b) {
        b = v;
        gb = k;
      }
    }
    unsigned char kind = DG_BKG;
    int g = -1;
    float v = 0.0f;
    if (a >= tf) { kind = DG_DUPE; g = ga; v = a; }
    else if (a >= tb) { kind = DG_LOC; g = ga; v = a; }
    else if (b >= tf) { kind = DG_CLS; g = gb; v = b; }
    else if (b >= tb) { kind = DG_BOTH; g = gb; v = b; }
    det_kind[i] = kind;
    det_gt[i] = g < 0 ? -1 : (int)(g0 + g);
    det_iou[i] = v;
  }
  __threadfence_block();

  // ---- pass 3: per GT box the TP that took it, the best LOC and the best CLS detection attributed to it
  for (int k = lane; k < n; k += 64) {
    const int g = (int)(g0 + k);
    int tp = -1, loc = -1, cls = -1;
    float sl = 0.0f, sc = 0.0f;
    for (long long i = d0; i < d1; ++i) {                 // ascending position: `>=` lets the higher position win a tie
      if (det_gt[i] != g) continue;
      const unsigned char kind = det_kind[i];
      if (kind == DG_TP) {
        tp = (int)i;
      } else if (kind == DG_LOC) {
        const float s = det_score[i];
        if (loc < 0 || s >= sl) { loc = (int)i; sl = s; }
      } else if (kind == DG_CLS) {
        const float s = det_score[i];
        if (cls < 0 || s >= sc) { cls = (int)i; sc = s; }
      }
    }
    gt_det[g] = tp;
    gt_det[G + g] = loc;
    gt_det[2 * G + g] = cls;
  }
}

}  // namespace

extern "C" int mega_diagnose_match(const float* det_box, const int* det_label, const float* det_score,
                                   const long long* det_off, const int* order, const float* ratio, const float* gt_box,
                                   const int* gt_label, const long long* gt_off, int F, int C, long long N, long long G,
                                   int max_gt, float bg_thresh, unsigned char* det_kind, int* det_gt, float* det_iou,
                                   int* gt_det, void* stream) {
  mega_clear_error();
  if (F < 0 || C <= 0 || N < 0 || G < 0 || max_gt < 0 || max_gt > DG_MAX_CHUNKS * 64) return MEGA_ERR_ARG;
  if (!(bg_thresh > 0.0f && bg_thresh < 0.5f)) return MEGA_ERR_ARG;          // (NaN too)
  if (N > 0x7fffffffLL || G > 0x7fffffffLL / 3) return MEGA_ERR_ARG;         // i32 indices; gt_det holds 3 G entries
  if (F > 0 && (!det_off || !ratio || !gt_off)) return MEGA_ERR_ARG;
  if (N > 0 && (!det_box || !det_label || !det_score || !order || !det_kind || !det_gt || !det_iou)) return MEGA_ERR_ARG;
  if (G > 0 && (!gt_box || !gt_label || !gt_det)) return MEGA_ERR_ARG;
  if (F == 0) return (N == 0 && G == 0) ? MEGA_OK : MEGA_ERR_ARG;            // no frame: nothing to write
  // one wave per frame: F * 64 threads in workgroups of 256
  hipLaunchKernelGGL(diagnose_match_kernel, dim3(grid1d((unsigned long long)F * 64, 0x7fffffffu)), dim3(64 * DG_WAVES), 0,
                     (hipStream_t)stream, (const float4*)det_box, det_label, det_score, det_off, order,
                     (const float2*)ratio, (const float4*)gt_box, gt_label, gt_off, F, N, G, max_gt, bg_thresh, det_kind,
                     det_gt, det_iou, gt_det);
  return mega_check_launch();
}
