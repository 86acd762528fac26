// Motion IoU of every GT box, as defined in mega/pytorch_amd/motion_iou.py (the reference only reads such values from a
// file): the mean IoU of a box with the boxes of its own track in the +-W neighbouring frames of its video.
//   Box b of frame f with track id t; offsets d = -W .. -1, +1 .. +W (slot k = 0 .. 2W-1 in that order); the neighbour in
//   frame f + d (inside [video start, video end)) is the box with track id t there, if any.  Pair IoU: b with +1 on x2 / y2
//   against the neighbour through box_math.h's vid_iou -- the detection AP's IoU of a detection that coincides with b.
//   value = the found pairs' f32 IoUs added in f64 in slot order / their count in f64; 0.0 without a neighbour; the
//   canonical quiet NaN if a pair IoU is NaN.  count = the neighbours found.
//
// Mapping: one wave64 (a 64-thread workgroup) per frame.
//   Phase 1: the lanes stride over the frame's n * 2W (box, slot) pairs; each scans the neighbour frame's track ids and
//   writes the pair's IoU bits (MI_MISSING: no neighbour) to slot box * 2W + k -- in LDS while n * 2W <= MI_LDS_PAIRS, else
//   in the frame's slice of the caller's workspace (its boxes' slots: gt_off[f] * 2W).
//   Phase 2: one lane per box (striding beyond 64) adds its 2W slots in ascending k.  No atomics, no cross-lane float
//   arithmetic: the result is the same bits on every run.
// Every index read from a device table is clamped or checked against the sizes the host passed before it addresses
// memory; a frame whose table entries do not fit is skipped (its outputs keep the caller's initial values).
#include "box_math.h"
#include "common.h"
#include "workspace.h"

namespace {

constexpr int MI_THREADS = 64;
constexpr int MI_LDS_PAIRS = 2048;        // (box, slot) pairs of a frame kept in LDS (motion_iou.LDS_PAIRS): 8 KiB
constexpr int MI_MAX_W = 64;              // window: at most 128 slots per box
constexpr int MI_MAX_GT = 4096;           // vid_eval.MAX_GT_PER_FRAME
constexpr unsigned MI_MISSING = 0xffffffffu;      // no neighbour; a NaN IoU is stored as MI_NAN, never as this
constexpr unsigned MI_NAN = 0x7fc00000u;

__device__ __forceinline__ void mi_frame(unsigned* slots, const float4* __restrict__ gt_box,
                                         const long long* __restrict__ gt_track, const long long* __restrict__ gt_off,
                                         long long G, long long s, int n, int f, int v0, int v1, int W,
                                         double* __restrict__ values, int* __restrict__ counts) {
  const int lane = threadIdx.x;
  const int S = 2 * W, pairs = n * S;     // (<= 4096 * 128)
  // ---- phase 1: the IoU of every (box, slot) pair
  for (int i = lane; i < pairs; i += MI_THREADS) {
    const int j = i / S, k = i - j * S;
    const int fn = f + (k < W ? k - W : k - W + 1);
    unsigned bits = MI_MISSING;
    if (fn >= v0 && fn < v1) {
      long long ns = gt_off[fn], ne = gt_off[fn + 1];
      if (ns < 0) ns = 0;
      if (ne > G) ne = G;
      const long long t = gt_track[s + j];
      for (long long m = ns; m < ne; ++m) {
        if (gt_track[m] != t) continue;
        const float4 b = gt_box[s + j];
        const float4 pb = make_float4(b.x, b.y, b.z + 1.0f, b.w + 1.0f);
        const float iou = vid_iou(pb, box_area1(pb), gt_box[m]);
        bits = iou != iou ? MI_NAN : __float_as_uint(iou);
        break;                            // (a frame holds a track id once: the host checks it)
      }
    }
    slots[i] = bits;
  }
  __syncthreads();
  // ---- phase 2: one lane per box, the slots in ascending offset
  for (int j = lane; j < n; j += MI_THREADS) {
    double acc = 0.0;
    int cnt = 0;
    bool nan = false;
    for (int k = 0; k < S; ++k) {
      const unsigned bits = slots[j * S + k];
      if (bits == MI_MISSING) continue;
      const float v = __uint_as_float(bits);
      nan = nan || v != v;
      acc += (double)v;
      ++cnt;
    }
    double out = cnt ? acc / (double)cnt : 0.0;
    if (nan) out = __longlong_as_double(0x7ff8000000000000LL);
    values[s + j] = out;
    counts[s + j] = cnt;
  }
}

__global__ __launch_bounds__(MI_THREADS) void motion_iou_kernel(
    const float4* __restrict__ gt_box, const long long* __restrict__ gt_track, const long long* __restrict__ gt_off,
    const int* __restrict__ video_start, const int* __restrict__ video_end, int F, long long G, int W, int max_gt,
    double* __restrict__ values, int* __restrict__ counts, unsigned* ws) {
  __shared__ unsigned s_slots[MI_LDS_PAIRS];
  const int f = blockIdx.x;               // (workgroup-uniform: a frame is done or skipped as a whole)
  if (f >= F) return;
  const long long s = gt_off[f], e = gt_off[f + 1];
  if (s < 0 || e > G || e <= s || e - s > max_gt) return;
  const int n = (int)(e - s);
  int v0 = video_start[f], v1 = video_end[f];
  if (v0 < 0) v0 = 0;
  if (v1 > F) v1 = F;
  if (n * 2 * W <= MI_LDS_PAIRS) {
    mi_frame(s_slots, gt_box, gt_track, gt_off, G, s, n, f, v0, v1, W, values, counts);
  } else {
    if (!ws) return;                      // (the host sizes the workspace by max_gt)
    mi_frame(ws + s * 2 * W, gt_box, gt_track, gt_off, G, s, n, f, v0, v1, W, values, counts);
  }
}

}  // namespace

// The slots of all G boxes when a frame's pairs may not fit LDS; nothing otherwise.
extern "C" size_t mega_motion_iou_workspace_bytes(long long G, int W, int max_gt) {
  if (G <= 0 || W < 1 || W > MI_MAX_W || max_gt <= 0) return 0;
  if ((long long)max_gt * 2 * W <= MI_LDS_PAIRS) return 0;
  WsCarver c(nullptr);
  c.take<unsigned>((size_t)G * 2 * (size_t)W);
  return c.bytes;
}

extern "C" int mega_motion_iou(const float* gt_box, const long long* gt_track, const long long* gt_off,
                               const int* video_start, const int* video_end, int F, long long G, int W, int max_gt,
                               double* values, int* counts, void* ws, size_t ws_bytes, void* stream) {
  mega_clear_error();
  if (F < 0 || G < 0 || W < 1 || W > MI_MAX_W || max_gt < 0 || max_gt > MI_MAX_GT || G > 0x7fffffffLL) return MEGA_ERR_ARG;
  if (!gt_off || (F > 0 && (!video_start || !video_end))) return MEGA_ERR_ARG;
  if (G > 0 && (!gt_box || !gt_track || !values || !counts)) return MEGA_ERR_ARG;
  const size_t need = mega_motion_iou_workspace_bytes(G, W, max_gt);
  if (need > 0 && !ws) return MEGA_ERR_ARG;
  if (ws_bytes < need) return MEGA_ERR_WS;
  if (F == 0 || G == 0) return MEGA_OK;   // nothing to do
  hipLaunchKernelGGL(motion_iou_kernel, dim3((unsigned)F), dim3(MI_THREADS), 0, (hipStream_t)stream,
                     (const float4*)gt_box, gt_track, gt_off, video_start, video_end, F, G, W, max_gt, values, counts,
                     need > 0 ? (unsigned*)ws : nullptr);
  return mega_check_launch();
}
