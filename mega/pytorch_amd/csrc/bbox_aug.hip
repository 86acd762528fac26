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
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int kMaxViews = 16;
constexpr int kMaxRows = 8192;     // K * R per (frame, class): 8192 u64 sort keys = 64 KiB of LDS

struct AugViews {
  float rw[kMaxViews], rh[kMaxViews];   // view 0 size / view k size (f32), per axis
  float w[kMaxViews];                   // view k image width (f32), for the flip
  int flip[kMaxViews];
};

__device__ __forceinline__ unsigned f32_sortable(float f) {
  unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float4 to_view0(float4 b, int k, const AugViews& v) {
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
      mboxes[base + i] = to_view0(cboxes[src], k, views);
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
    sboxes[base + i] = to_view0(cboxes[(((size_t)k * F + f) * C1 + c) * R + r], k, views);
  }
  if (threadIdx.x == 0) counts[p] = n;
}

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

}  // namespace

extern "C" size_t mega_bbox_aug_merge_workspace_bytes(int F, int K, int R, int NC) {
  const size_t m = (size_t)F * (NC - 1) * K * R;
  const size_t P = (size_t)F * (NC - 1);
  return 2 * align_up(m * 16, 256) + 4 * align_up(m * 4, 256) + align_up(m, 256) + 2 * align_up(P * 4, 256);
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
  for (int k = 0; k < kMaxViews; ++k) {
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
  hipStream_t st = (hipStream_t)stream;
  const int C1 = NC - 1, P = F * C1, KR = K * R;
  const size_t m = (size_t)P * KR;
  unsigned char* w = (unsigned char*)ws;
  float4* mboxes = (float4*)w; w += align_up(m * 16, 256);
  float4* sboxes = (float4*)w; w += align_up(m * 16, 256);
  float* mscores = (float*)w; w += align_up(m * 4, 256);
  int* order = (int*)w; w += align_up(m * 4, 256);
  int* keep_pos = (int*)w; w += align_up(m * 4, 256);
  int* tmp_idx = (int*)w; w += align_up(m * 4, 256);
  unsigned char* flags = w; w += align_up(m, 256);
  int* counts = (int*)w; w += align_up((size_t)P * 4, 256);
  int* keep_cnt = (int*)w;
  int ns = 64;
  while (ns < KR) ns <<= 1;
  (void)hipFuncSetAttribute((const void*)aug_load_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            kMaxRows * (int)sizeof(u64));
  hipLaunchKernelGGL(aug_load_sort_kernel, dim3(P), dim3(1024), (size_t)ns * sizeof(u64), st, (const float4*)cboxes,
                     cscores, K, F, C1, R, score_thresh, v, mboxes, mscores, flags, sboxes, order, counts);
  int rc = mega_check_launch();
  if (rc != MEGA_OK) return rc;
  rc = mega_boxes_nms_lazy((const float*)sboxes, counts, order, P, KR, nms_thresh, strict_gt, KR, keep_pos, keep_cnt,
                           flags, st);
  if (rc != MEGA_OK) return rc;
  return mega_boxes_post_finalize(flags, (const float*)mboxes, mscores, F, C1, KR, max_det, out_boxes, out_scores,
                                  out_labels, out_cnt, tmp_idx, st);
}
