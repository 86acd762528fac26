// Shared by bbox_aug.hip and soft_nms.hip: the views of a test-time augmentation merge, the mapping of a view's box into
// view 0's image, and the workspace both merges and the post-processor (boxes.hip) carve up the same way.  The +1 IoU and
// the (score, row) sort key are box_math.h's.
// Every includer is compiled with -ffp-contract=off: every product and difference below rounds on its own.
#pragma once
#include "box_math.h"
#include "common.h"
#include "workspace.h"

constexpr int kAugMaxViews = 16;
constexpr int kAugMaxRows = 8192;     // K * R per (frame, class)

struct AugViews {
  float rw[kAugMaxViews], rh[kAugMaxViews];   // view 0 size / view k size (f32), per axis
  float w[kAugMaxViews];                      // view k image width (f32), for the flip
  int flip[kAugMaxViews];
};

// The workspace of mega_bbox_aug_merge (m = F * (NC-1) * K * R rows, P = F * (NC-1) problems) and the head of
// mega_soft_merge's and mega_postprocess_batched's (m = B * (NC-1) * R, P = B * (NC-1)), in this order.
struct AugWs {
  float4* mboxes;          // [m] boxes in view 0's image
  float4* sboxes;          // [m] the same, score-sorted per problem
  float* mscores;          // [m] scores, -1 = dead
  int* order;              // [m] sorted position -> row
  int* keep_pos;           // [m] kept positions per problem
  int* tmp_idx;            // [m] scratch of the finalize
  unsigned char* flags;    // [m] 1 = kept
  int* counts;             // [P] live rows
  int* keep_cnt;           // [P] kept rows
};

// Takes the nine arrays from c; an entry point with more in its workspace goes on taking from the same carver.
static inline AugWs aug_ws_carve(WsCarver& c, size_t m, size_t P) {
  return {c.take<float4>(m), c.take<float4>(m), c.take<float>(m), c.take<int>(m), c.take<int>(m), c.take<int>(m),
          c.take<unsigned char>(m), c.take<int>(P), c.take<int>(P)};     // (evaluated left to right: AugWs's order)
}

// view_w / view_h / view_flip [K] (host).  MEGA_ERR_ARG for a view without a size.
static inline int aug_views_init(AugViews& v, const int* view_w, const int* view_h, const int* view_flip, int K) {
  for (int k = 0; k < kAugMaxViews; ++k) {
    v.rw[k] = v.rh[k] = 1.f;
    v.w[k] = 0.f;
    v.flip[k] = 0;
  }
  for (int k = 0; k < K; ++k) {
    if (view_w[k] <= 0 || view_h[k] <= 0) return MEGA_ERR_ARG;
    // BoxList.resize: float(s) / float(s_orig) in double, then the f32 tensor times that Python float (an f32 multiply)
    v.rw[k] = (float)((double)view_w[0] / (double)view_w[k]);
    v.rh[k] = (float)((double)view_h[0] / (double)view_h[k]);
    v.w[k] = (float)view_w[k];
    v.flip[k] = view_flip[k] ? 1 : 0;
  }
  return MEGA_OK;
}

static __device__ __forceinline__ float4 aug_to_view0(float4 b, int k, const AugViews& v) {
  if (v.flip[k]) {
    const float x1 = v.w[k] - b.z - 1.f;
    const float x2 = v.w[k] - b.x - 1.f;
    b.x = x1;
    b.z = x2;
  }
  if (k > 0) {
    b.x = b.x * v.rw[k];
    b.y = b.y * v.rh[k];
    b.z = b.z * v.rw[k];
    b.w = b.w * v.rh[k];
  }
  return b;
}

// Library-internal (bbox_aug.hip): the first two stages of mega_bbox_aug_merge -- load + view mapping + per-class sort,
// then the greedy NMS -- into a carved workspace: w.mboxes / w.mscores / w.flags / w.order / w.keep_pos / w.keep_cnt.
int mega_bbox_aug_load_nms(const float* cboxes, const float* cscores, int F, int K, int R, int NC, const AugViews& v,
                           float score_thresh, float nms_thresh, int strict_gt, const AugWs& w, hipStream_t st);
