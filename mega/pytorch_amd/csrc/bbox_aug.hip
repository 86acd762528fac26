// Test-time box augmentation: the merge of engine/bbox_aug.py:53-66 (im_detect_bbox_aug) on device.
//
// Input: the candidates of K views of F frames, as mega_postprocess_candidates_batched writes them for every view --
// boxes [K][F][NC-1][R][4] in the view's own image (decoded, clipped), scores [K][F][NC-1][R] (-1 at or below the
// score threshold).  Per (frame, class), the K*R rows are taken in (view, proposal row) order -- the reference's
// concatenation order -- and each row's box is mapped into view 0's image as it is loaded:
//   flipped view : x' = (W_k - x_max) - 1, x'_max = (W_k - x_min) - 1     (BoxList.transpose, two f32 ops each)
//   view k > 0   : x * rw_k, y * rh_k, the f32 ratios of view 0's size to view k's (BoxList.resize: one multiply;
//                  rw_k == rh_k is the reference's single-ratio branch, the same arithmetic)
// then filter_results (box_head/inference.py:102-149) runs on the K*R rows: score > thresh, per-class sort (score desc,
// row asc), greedy NMS, class-major / row-ascending compaction and the detections-per-image k-th value cut.  With K = 1
// and view 0 this is mega_postprocess's P2-P4 on the same candidates: the same bits.
// Compiled with -ffp-contract=off: the flip / resize products and differences round like the reference's torch ops.
#include "aug_views.h"
#include "launch.h"

namespace {

typedef unsigned long long u64;

constexpr int kMaxViews = kAugMaxViews;
constexpr int kMaxRows = kAugMaxRows;     // K * R per (frame, class): 8192 u64 sort keys = 64 KiB of LDS

// One 1024-thread block per (frame, class) problem p = f * C1 + c.  Writes the merged rows (view-0 boxes, scores with
// -1 for dropped rows, zeroed kept flags) at [p][K*R], and the score-sorted boxes + order + count for the NMS.
__global__ __launch_bounds__(1024) void aug_load_sort_kernel(const float4* __restrict__ cboxes,
                                                             const float* __restrict__ cscores, int K, int F, int C1,
                                                             int R, float score_thresh, AugViews views,
                                                             float4* __restrict__ mboxes, float* __restrict__ mscores,
                                                             unsigned char* __restrict__ flags,
                                                             float4* __restrict__ sboxes, int* __restrict__ order,
                                                             int* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char aug_smem[];
  u64* s = reinterpret_cast<u64*>(aug_smem);
  __shared__ int cnt;
  const int p = blockIdx.x, f = p / C1, c = p - f * C1;
  const int KR = K * R;
  const size_t base = (size_t)p * KR;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  int ns = 64;
  while (ns < KR) ns <<= 1;
  int local = 0;
  for (int i = threadIdx.x; i < ns; i += blockDim.x) {
    u64 key = 0;
    if (i < KR) {
      const int k = i / R, r = i - k * R;
      const size_t src = (((size_t)k * F + f) * C1 + c) * R + r;
      float sc = cscores[src];
      if (!(sc >= 0.f && sc > score_thresh)) sc = -1.f;
      mboxes[base + i] = aug_to_view0(cboxes[src], k, views);
      mscores[base + i] = sc;
      flags[base + i] = 0;
      if (sc >= 0.f) {
        key = ((u64)f32_sortable(sc) << 32) | (u64)(0xFFFFFFFFu - (unsigned)i);
        ++local;
      }
    }
    s[i] = key;
  }
  if (local) atomicAdd(&cnt, local);
  __syncthreads();
  for (int k2 = 2; k2 <= ns; k2 <<= 1) {           // bitonic, descending (boxes.hip bitonic_sort_desc)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < ns; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const u64 a = s[i], b = s[ixj];
          const bool desc = (i & k2) == 0;
          if (desc ? (a < b) : (a > b)) { s[i] = b; s[ixj] = a; }
        }
      }
      __syncthreads();
    }
  }
  const int n = cnt;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int idx = (int)(0xFFFFFFFFu - (unsigned)(s[i] & 0xFFFFFFFFu));
    const int k = idx / R, r = idx - k * R;
    order[base + i] = idx;
    // (recomputed from the input rather than read back from mboxes: no cross-thread global round trip)
    sboxes[base + i] = aug_to_view0(cboxes[(((size_t)k * F + f) * C1 + c) * R + r], k, views);
  }
  if (threadIdx.x == 0) counts[p] = n;
}

}  // namespace

extern "C" size_t mega_bbox_aug_merge_workspace_bytes(int F, int K, int R, int NC) {
  WsCarver c(nullptr);
  aug_ws_carve(c, (size_t)F * (NC - 1) * K * R, (size_t)F * (NC - 1));
  return c.bytes;
}

// Library-internal (aug_views.h): load + sort + greedy NMS, shared with the soft-NMS / box-voting merge (soft_nms.hip).
int mega_bbox_aug_load_nms(const float* cboxes, const float* cscores, int F, int K, int R, int NC, const AugViews& v,
                           float score_thresh, float nms_thresh, int strict_gt, const AugWs& w, hipStream_t st) {
  const int C1 = NC - 1, P = F * C1, KR = K * R;
  int ns = 64;
  while (ns < KR) ns <<= 1;
  const int rc = launch_lds(aug_load_sort_kernel, dim3(P), dim3(1024), (size_t)ns * sizeof(u64), st, (const float4*)cboxes,
                            cscores, K, F, C1, R, score_thresh, v, w.mboxes, w.mscores, w.flags, w.sboxes, w.order, w.counts);
  if (rc != MEGA_OK) return rc;
  return mega_boxes_nms_lazy((const float*)w.sboxes, w.counts, nullptr, w.order, P, KR, nms_thresh, strict_gt, KR,
                             w.keep_pos, w.keep_cnt, w.flags, st);
}

// cboxes [K][F][NC-1][R][4], cscores [K][F][NC-1][R]; view_w / view_h [K] (host) the views' image sizes, view_flip [K]
// (host) 1 = the view's frames were mirrored.  Outputs per frame f (capacity (NC-1)*K*R rows): out_boxes [F][cap][4],
// out_scores [F][cap], out_labels [F][cap] i64, out_cnt [F] i32 (device).
extern "C" int mega_bbox_aug_merge(const float* cboxes, const float* cscores, int F, int K, int R, int NC,
                                   const int* view_w, const int* view_h, const int* view_flip, float score_thresh,
                                   float nms_thresh, int strict_gt, int max_det, float* out_boxes, float* out_scores,
                                   long long* out_labels, int* out_cnt, void* ws, size_t ws_bytes, void* stream) {
  mega_clear_error();
  if (!cboxes || !cscores || !view_w || !view_h || !view_flip || !out_boxes || !out_scores || !out_labels || !out_cnt ||
      !ws || F <= 0 || K <= 0 || R <= 0 || NC < 2)
    return MEGA_ERR_ARG;
  if (K > kMaxViews || (long long)K * R > kMaxRows) return MEGA_ERR_LIMIT;
  if ((long long)F * (NC - 1) > 0x7fffffffLL) return MEGA_ERR_ARG;
  if (ws_bytes < mega_bbox_aug_merge_workspace_bytes(F, K, R, NC)) return MEGA_ERR_WS;
  AugViews v;
  int rc = aug_views_init(v, view_w, view_h, view_flip, K);
  if (rc != MEGA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int C1 = NC - 1, KR = K * R;
  WsCarver c(ws);
  const AugWs w = aug_ws_carve(c, (size_t)F * C1 * KR, (size_t)F * C1);
  rc = mega_bbox_aug_load_nms(cboxes, cscores, F, K, R, NC, v, score_thresh, nms_thresh, strict_gt, w, st);
  if (rc != MEGA_OK) return rc;
  return mega_boxes_post_finalize(w.flags, (const float*)w.mboxes, w.mscores, F, C1, KR, max_det, out_boxes, out_scores,
                                  out_labels, out_cnt, w.tmp_idx, st);
}
