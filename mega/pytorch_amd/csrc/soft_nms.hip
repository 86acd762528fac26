// Soft-NMS (TEST.SOFT_NMS) and box voting (TEST.BBOX_VOTE): the final filter of the candidate merge, as
// mega/pytorch_amd/soft_nms.py defines it (tests/soft_nms_twin.py is the numpy twin).
//
// Input: what mega_bbox_aug_merge takes -- the candidates of K views of F frames, cboxes [K][F][NC-1][R][4] and cscores
// [K][F][NC-1][R] (-1 = dead).  Per (frame, class) the K*R rows are taken in (view, row) order and mapped into view 0's
// image (aug_views.h), then
//   soft-NMS   one 64..1024-thread block per problem keeps its rows in REGISTERS (box + score, up to 8 rows a thread) for
//              the whole chain of dependent steps: per-thread max of the (score bits, inverted row) key, wave64 shuffle
//              reduce, one LDS exchange across the waves that also carries each wave's winning box, then the decay of
//              the thread's own rows against the winner.  One barrier per step (the exchange is double-buffered).
//   voting     one wave per kept row, lanes striding over the class's live rows with their ORIGINAL boxes and scores;
//              five f64 partial sums per lane, shuffle-reduced; results go to buffers of their own.
//   finalize   the post-processor's compaction and detections-per-image cut (boxes.hip) on the final scores.
// With soft-NMS off the greedy NMS is bbox_aug.hip's; with both off the call IS mega_bbox_aug_merge.
// Compiled with -ffp-contract=off: the IoU, the flip / resize and the decay round as the definition's separate f32 ops.
#include "aug_views.h"

namespace {

typedef unsigned long long u64;

// NR rows per thread: row i = j * blockDim.x + tid, j < NR; blockDim.x * NR >= K * R.
template <int NR>
__global__ __launch_bounds__(1024) void soft_nms_kernel(const float4* __restrict__ cboxes,
                                                        const float* __restrict__ cscores, int K, int F, int C1, int R,
                                                        float score_thresh, AugViews views, float nms_thresh,
                                                        int strict_gt, int method, float sigma,
                                                        float4* __restrict__ mboxes, float* __restrict__ mscores,
                                                        unsigned char* __restrict__ flags, float* __restrict__ fscores,
                                                        int* __restrict__ keep_idx, int* __restrict__ keep_cnt) {
  __shared__ u64 wkey[2][16];
  __shared__ float4 wbox[2][16];
  const int p = blockIdx.x, f = p / C1, c = p - f * C1;
  const int KR = K * R, T = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = T >> 6;
  const size_t base = (size_t)p * KR;
  float4 box[NR];
  float sc[NR];
  unsigned alive = 0, kept = 0;
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int i = j * T + tid;
    box[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    sc[j] = -1.f;
    if (i < KR) {
      const int k = i / R, r = i - k * R;
      const size_t src = (((size_t)k * F + f) * C1 + c) * R + r;
      float s = cscores[src];
      if (!(s >= 0.f && s > score_thresh)) s = -1.f;
      box[j] = aug_to_view0(cboxes[src], k, views);
      sc[j] = s;
      mboxes[base + i] = box[j];
      mscores[base + i] = s;
      if (s >= 0.f) alive |= 1u << j;
    }
  }
  int nk = 0;
  for (int step = 0; step < KR; ++step) {      // every pass removes at least the winner
    u64 best = 0;
    float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      if ((alive >> j) & 1u) {
        const u64 key = ((u64)f32_sortable(sc[j]) << 32) | (u64)(0xFFFFFFFFu - (unsigned)(j * T + tid));
        if (key > best) { best = key; bb = box[j]; }
      }
    }
    u64 wb = best;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const u64 o = __shfl_xor(wb, d);
      wb = o > wb ? o : wb;
    }
    const int buf = step & 1;
    if (wb == 0) {
      if (lane == 0) wkey[buf][wave] = 0;
    } else if (best == wb) {                   // keys are unique (they hold the row): one lane per wave
      wkey[buf][wave] = wb;
      wbox[buf][wave] = bb;
    }
    __syncthreads();
    u64 win = 0;
    int ww = 0;
    for (int w = 0; w < nw; ++w) {
      const u64 k2 = wkey[buf][w];
      if (k2 > win) { win = k2; ww = w; }
    }
    if (win == 0) break;                       // nothing alive (uniform: every thread read the same keys)
    const float4 mb = wbox[buf][ww];
    const int widx = (int)(0xFFFFFFFFu - (unsigned)(win & 0xFFFFFFFFull));
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const unsigned bit = 1u << j;
      if (!(alive & bit)) continue;
      if (j * T + tid == widx) {               // the winner is kept with its current score
        kept |= bit;
        alive &= ~bit;
        keep_idx[base + nk] = widx;
        continue;
      }
      const float o = box_iou1(mb, box[j]);
      float w = 1.f;
      if (o == o) {                            // a NaN IoU does not decay
        if (method == 2) w = expf(-(o * o) / sigma);
        else if (strict_gt ? (o > nms_thresh) : (o >= nms_thresh)) w = 1.f - o;
      }
      sc[j] = sc[j] * w;
      if (!(sc[j] > score_thresh)) alive &= ~bit;
    }
    ++nk;
  }
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int i = j * T + tid;
    if (i < KR) {
      const bool kp = (kept >> j) & 1u;
      flags[base + i] = kp ? 1 : 0;
      fscores[base + i] = kp ? sc[j] : -1.f;
    }
  }
  if (tid == 0) keep_cnt[p] = nk;
}

// One wave per kept row: slot t = blockIdx.y * 4 + wave of problem blockIdx.x.  The kept row is keep_pos[t] itself, or
// order[keep_pos[t]] when the greedy NMS produced sorted positions.  out_scores[k] = in_scores[k] ("ID") or the voters'
// mean; out_scores may be in_scores (only row k's own entry is read and written by its wave).
__global__ __launch_bounds__(256) void box_vote_kernel(const float4* __restrict__ mboxes,
                                                       const float* __restrict__ mscores, const float* in_scores,
                                                       const int* __restrict__ keep_pos,
                                                       const int* __restrict__ keep_cnt, const int* __restrict__ order,
                                                       int KR, float vote_thresh, int scoring,
                                                       float4* __restrict__ vboxes, float* out_scores) {
  const int p = blockIdx.x, lane = threadIdx.x & 63;
  const int t = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (t >= min(keep_cnt[p], KR)) return;
  const size_t base = (size_t)p * KR;
  const int pos = keep_pos[base + t];
  if (pos < 0 || pos >= KR) return;
  const int k = order ? order[base + pos] : pos;
  if (k < 0 || k >= KR) return;
  const float4 kb = mboxes[base + k];
  double sx1 = 0., sy1 = 0., sx2 = 0., sy2 = 0., ss = 0.;
  int n = 0;
  for (int j = lane; j < KR; j += 64) {
    const float s = mscores[base + j];
    if (!(s >= 0.f)) continue;
    const float4 b = mboxes[base + j];
    if (j == k || box_iou1(kb, b) >= vote_thresh) {      // (NaN >= thr is false: a NaN IoU does not vote)
      const double sd = (double)s;
      sx1 += sd * (double)b.x;
      sy1 += sd * (double)b.y;
      sx2 += sd * (double)b.z;
      sy2 += sd * (double)b.w;
      ss += sd;
      ++n;
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    sx1 += __shfl_xor(sx1, d);
    sy1 += __shfl_xor(sy1, d);
    sx2 += __shfl_xor(sx2, d);
    sy2 += __shfl_xor(sy2, d);
    ss += __shfl_xor(ss, d);
    n += __shfl_xor(n, d);
  }
  if (lane == 0) {
    vboxes[base + k] = make_float4((float)(sx1 / ss), (float)(sy1 / ss), (float)(sx2 / ss), (float)(sy2 / ss));
    out_scores[base + k] = scoring ? (float)(ss / (double)n) : in_scores[base + k];
  }
}

// The bbox_aug workspace, then the voted boxes [m][4] and the final scores [m].
struct SoftWs {
  AugWs aug; float4* vboxes; float* fscores;
  size_t bytes;
};

SoftWs soft_ws_carve(void* ws, size_t m, size_t P) {
  WsCarver c(ws);
  return {aug_ws_carve(c, m, P), c.take<float4>(m), c.take<float>(m), c.bytes};
}

}  // namespace

extern "C" size_t mega_soft_merge_workspace_bytes(int F, int K, int R, int NC) {
  return soft_ws_carve(nullptr, (size_t)F * (NC - 1) * K * R, (size_t)F * (NC - 1)).bytes;
}

extern "C" int mega_soft_merge(const float* cboxes, const float* cscores, int F, int K, int R, int NC, const int* view_w,
                               const int* view_h, const int* view_flip, float score_thresh, float nms_thresh,
                               int strict_gt, int soft_method, float sigma, int vote, float vote_thresh,
                               int vote_scoring, int max_det, float* out_boxes, float* out_scores, long long* out_labels,
                               int* out_cnt, void* ws, size_t ws_bytes, void* stream) {
  mega_clear_error();
  if (!cboxes || !cscores || !view_w || !view_h || !view_flip || !out_boxes || !out_scores || !out_labels || !out_cnt ||
      !ws || F <= 0 || K <= 0 || R <= 0 || NC < 2)
    return MEGA_ERR_ARG;
  if (soft_method < 0 || soft_method > 2 || !(sigma > 0.f) || (vote != 0 && vote != 1) ||
      !(vote_thresh > 0.f && vote_thresh <= 1.f) || (vote_scoring != 0 && vote_scoring != 1))
    return MEGA_ERR_ARG;
  if (K > kAugMaxViews || (long long)K * R > kAugMaxRows) return MEGA_ERR_LIMIT;
  if ((long long)F * (NC - 1) > 0x7fffffffLL) return MEGA_ERR_ARG;
  if (ws_bytes < mega_soft_merge_workspace_bytes(F, K, R, NC)) return MEGA_ERR_WS;
  if (!soft_method && !vote)
    return mega_bbox_aug_merge(cboxes, cscores, F, K, R, NC, view_w, view_h, view_flip, score_thresh, nms_thresh,
                               strict_gt, max_det, out_boxes, out_scores, out_labels, out_cnt, ws, ws_bytes, stream);
  AugViews v;
  int rc = aug_views_init(v, view_w, view_h, view_flip, K);
  if (rc != MEGA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int C1 = NC - 1, P = F * C1, KR = K * R;
  const SoftWs sw = soft_ws_carve(ws, (size_t)P * KR, (size_t)P);
  const AugWs& w = sw.aug;
  float4* vboxes = sw.vboxes;
  float* fscores = sw.fscores;
  if (soft_method) {
    int T = (KR + 63) / 64 * 64;
    if (T > 1024) T = 1024;
    const int nr = (KR + T - 1) / T;
    const auto kernel = nr <= 1 ? soft_nms_kernel<1> : nr <= 2 ? soft_nms_kernel<2> : nr <= 4 ? soft_nms_kernel<4> : soft_nms_kernel<8>;
    hipLaunchKernelGGL(kernel, dim3(P), dim3(T), 0, st, (const float4*)cboxes, cscores, K, F, C1, R, score_thresh, v,
                       nms_thresh, strict_gt, soft_method, sigma, w.mboxes, w.mscores, w.flags, fscores, w.keep_pos,
                       w.keep_cnt);
    rc = mega_check_launch();
  } else {
    rc = mega_bbox_aug_load_nms(cboxes, cscores, F, K, R, NC, v, score_thresh, nms_thresh, strict_gt, w, st);
  }
  if (rc != MEGA_OK) return rc;
  if (vote) {
    hipLaunchKernelGGL(box_vote_kernel, dim3(P, cdiv(KR, 4)), dim3(256), 0, st, (const float4*)w.mboxes,
                       (const float*)w.mscores, soft_method ? (const float*)fscores : (const float*)w.mscores,
                       (const int*)w.keep_pos, (const int*)w.keep_cnt, soft_method ? (const int*)nullptr : (const int*)w.order,
                       KR, vote_thresh, vote_scoring, vboxes, fscores);
    rc = mega_check_launch();
    if (rc != MEGA_OK) return rc;
  }
  return mega_boxes_post_finalize(w.flags, vote ? (const float*)vboxes : (const float*)w.mboxes,
                                  (soft_method || vote) ? fscores : w.mscores, F, C1, KR, max_det, out_boxes, out_scores,
                                  out_labels, out_cnt, w.tmp_idx, st);
}
