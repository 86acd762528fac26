// The one "+1" (legacy TO_REMOVE = 1) box area and IoU of the box kernels: nms.cu:13-21 devIoU term by term, which is
// also boxlist_iou's (structures/boxlist_ops.py:53-89) and the IoU seq_nms.py / tracks.py / soft_nms.py define.
//   area(b) = (x2 - x1 + 1) * (y2 - y1 + 1);  width = max(min(x2) - max(x1) + 1, 0), height likewise;
//   IoU = interS / (Sa + Sb - interS)
// ONLY correct in a translation unit built with -ffp-contract=off: every product, sum and difference below must round
// on its own, as the reference's separate f32 torch ops do (tests/test_box_shared.py holds build.py to that).
// A box with x2 < x1 - 1 has a negative area and can give a NaN IoU; every caller's comparison is false on NaN.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float box_area1(const float4 b) { return (b.z - b.x + 1.f) * (b.w - b.y + 1.f); }

__device__ __forceinline__ float box_inter1(const float4 a, const float4 b) {
  const float left = fmaxf(a.x, b.x), right = fminf(a.z, b.z);
  const float top = fmaxf(a.y, b.y), bottom = fminf(a.w, b.w);
  const float width = fmaxf(right - left + 1.f, 0.f), height = fmaxf(bottom - top + 1.f, 0.f);
  return width * height;
}

__device__ __forceinline__ float box_union1(float Sa, float Sb, float interS) { return Sa + Sb - interS; }

// Sa / Sb: box_area1 of a / b, for callers that keep the areas
__device__ __forceinline__ float box_iou1(const float4 a, float Sa, const float4 b, float Sb) {
  const float interS = box_inter1(a, b);
  return interS / box_union1(Sa, Sb, interS);
}

__device__ __forceinline__ float box_iou1(const float4 a, const float4 b) {
  return box_iou1(a, box_area1(a), b, box_area1(b));
}

// The VID evaluations' IoU (vid_eval.hip's detection AP, track_eval.hip's frame hits) of a detection box p that is already
// rescaled and carries vid_eval.py:209-214's +1 on x2 / y2 (pa = box_area1(p)) with a raw GT box g: g gets the same +1,
// then boxlist_iou's operation order in f32.
__device__ __forceinline__ float vid_iou(float4 p, float pa, float4 g) {
  g.z += 1.0f;
  g.w += 1.0f;
  return box_iou1(p, pa, g, box_area1(g));
}

// f32 -> u32 whose unsigned order is the floats' order (the sort keys' high word).  Floats that compare equal get equal
// keys, so that the index in the low word breaks the tie: -0.0 takes +0.0's key (on the bits, not by `f + 0.f`, which
// holds only as long as no flag lets the compiler drop the addition).  NaNs are not ordered by any caller's contract.
__device__ __forceinline__ unsigned f32_sortable(float f) {
  unsigned u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
