// ImageNet VID proposal recall: the greedy one-to-one matching of a frame's first `limit` proposals to its GT boxes of
//   mega_core/data/datasets/evaluation/vid/vid_eval.py:72-119   eval_proposals_vid
// with the box rescale of structures/bounding_box.py:91-125 (BoxList.resize) and the IoU of
// structures/boxlist_ops.py:53-89 (boxlist_iou, TO_REMOVE = 1).
//
// Built with -ffp-contract=off: every f32 operation of the rescale / IoU rounds exactly like the reference's separate
// torch ops (no FMA contraction).
#include "box_math.h"
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int PR_WAVES = 4;         // waves per block
constexpr int PR_SLOTS = 16;        // proposals per lane -> at most 16 x 64 = 1024 proposals per (frame, limit)
constexpr int PR_MAX_CHUNKS = 64;   // removed-GT flags: one 64-bit word per lane -> at most 64 x 64 GT boxes per frame

// The best live pair so far.  Order: IoU descending, then GT index ascending, then proposal position ascending -- what
// overlaps.max(dim=0) followed by max_overlaps.max(dim=0) picks on the CPU (the first maximum of each).
struct Best {
  float iou;
  int g, p;
};

__device__ __forceinline__ bool better(float v, int g, int p, const Best& b) {
  return v > b.iou || (v == b.iou && (g < b.g || (g == b.g && p < b.p)));
}

// One wave per (frame, limit).  Lane l owns the proposals at sorted positions l, l + 64, ... (rescaled once, kept in
// registers with their areas; bit k of `prem`: position k * 64 + l has been matched) and the removed flag of the GT
// slots l, l + 64, ... (bit c of `grem`; a chunk's 64 flags are gathered with one ballot).  Each of the min(P, G)
// rounds recomputes the IoUs of the live pairs -- every lane walks the live GT boxes (wave-uniform loads) against its
// live proposals -- reduces the best pair over the wave and removes it.  Nothing is shared through memory, so there is
// no barrier; gt_overlap / gt_prop are pre-set to 0 / -1 by the caller and lane 0 writes the matched entries.
__global__ __launch_bounds__(64 * PR_WAVES) void proposal_recall_match_kernel(
    const float4* __restrict__ box, const long long* __restrict__ off, const int* __restrict__ order,
    const float2* __restrict__ ratio, const float4* __restrict__ gt_box, const long long* __restrict__ gt_off,
    const int* __restrict__ limits, int F, int nL, long long G_all, float* __restrict__ gt_overlap,
    int* __restrict__ gt_prop) {
  const int wid = blockIdx.x * PR_WAVES + (int)(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (wid >= F * nL) return;
  const int f = wid / nL, li = wid % nL;
  const long long g0 = gt_off[f];
  const int G = (int)(gt_off[f + 1] - g0);
  const long long d0 = off[f];
  const long long n = off[f + 1] - d0;
  const int lim = limits[li];
  const int P = (int)(n < (long long)lim ? n : (long long)lim);
  if (G == 0 || P == 0) return;
  const float rw = ratio[f].x, rh = ratio[f].y;

  float4 pb[PR_SLOTS];
  float pa[PR_SLOTS];
  unsigned prem = 0;     // bit k set: slot k is dead (matched, or past P)
#pragma unroll
  for (int k = 0; k < PR_SLOTS; ++k) {
    const int p = k * 64 + lane;
    if (p < P) {
      const float4 b = box[order[d0 + p]];
      // BoxList.resize: x * ratio_w, y * ratio_h in f32; BoxList.area: (x2 - x1 + 1) * (y2 - y1 + 1)
      pb[k] = make_float4(b.x * rw, b.y * rh, b.z * rw, b.w * rh);
      pa[k] = box_area1(pb[k]);
    } else {
      pb[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      pa[k] = 0.f;
      prem |= 1u << k;
    }
  }
  u64 grem = 0;
  const int nch = (G + 63) >> 6;
  const int rounds = P < G ? P : G;
  float* out_ov = gt_overlap + (long long)li * G_all + g0;
  int* out_pr = gt_prop + (long long)li * G_all + g0;

  for (int j = 0; j < rounds; ++j) {
    Best best = {-INFINITY, 0x7fffffff, 0x7fffffff};
    for (int c = 0; c < nch; ++c) {
      const int left = G - c * 64;
      u64 live = ~__ballot((grem >> c) & 1);
      if (left < 64) live &= (1ull << left) - 1;
      while (live) {
        const int t = __builtin_ctzll(live);
        live &= live - 1;
        const int g = c * 64 + t;
        const float4 gb = gt_box[g0 + g];
        const float ga = box_area1(gb);
#pragma unroll
        for (int k = 0; k < PR_SLOTS; ++k) {
          if ((prem >> k) & 1) continue;
          const float v = box_iou1(pb[k], pa[k], gb, ga);
          // g ascends, then k: a strict > keeps the lane's first maximum (a NaN never wins)
          if (v > best.iou) {
            best.iou = v;
            best.g = g;
            best.p = k * 64 + lane;
          }
        }
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const float v = __shfl_xor(best.iou, o, 64);
      const int g = __shfl_xor(best.g, o, 64);
      const int p = __shfl_xor(best.p, o, 64);
      if (better(v, g, p, best)) {
        best.iou = v;
        best.g = g;
        best.p = p;
      }
    }
    if (best.p == 0x7fffffff) break;     // only NaN / -inf IoUs are left (boxes with x2 < x1 - 1)
    if (lane == (best.p & 63)) prem |= 1u << (best.p >> 6);
    if (lane == (best.g & 63)) grem |= 1ull << (best.g >> 6);
    if (lane == 0) {
      out_ov[best.g] = best.iou;
      out_pr[best.g] = best.p;
    }
  }
}

}  // namespace

extern "C" int mega_proposal_recall_match(const float* box, const long long* off, const int* order, const float* ratio,
                                          const float* gt_box, const long long* gt_off, const int* limits, int F, int nL,
                                          long long N, long long G, int max_limit, int max_gt, float* gt_overlap,
                                          int* gt_prop, void* stream) {
  mega_clear_error();
  if (!off || !ratio || !gt_off || !limits || F <= 0 || nL <= 0 || N < 0 || G < 0 || max_limit < 0 || max_gt < 0)
    return MEGA_ERR_ARG;
  if (N > 0 && (!box || !order)) return MEGA_ERR_ARG;
  if (G > 0 && (!gt_box || !gt_overlap || !gt_prop)) return MEGA_ERR_ARG;
  if (max_limit > PR_SLOTS * 64 || max_gt > PR_MAX_CHUNKS * 64 || N > 0x7fffffffLL ||
      (long long)F * nL > 0x7fffffffLL - PR_WAVES)
    return MEGA_ERR_ARG;
  if (G == 0) return MEGA_OK;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(gt_overlap, 0, (size_t)nL * (size_t)G * sizeof(float), st) != hipSuccess) return MEGA_ERR_LAUNCH;
  if (hipMemsetAsync(gt_prop, 0xff, (size_t)nL * (size_t)G * sizeof(int), st) != hipSuccess) return MEGA_ERR_LAUNCH;
  if (N == 0) return MEGA_OK;
  hipLaunchKernelGGL(proposal_recall_match_kernel, dim3(cdiv(F * nL, PR_WAVES)), dim3(64 * PR_WAVES), 0, st,
                     (const float4*)box, off, order, (const float2*)ratio, (const float4*)gt_box, gt_off, limits, F, nL, G,
                     gt_overlap, gt_prop);
  return mega_check_launch();
}
