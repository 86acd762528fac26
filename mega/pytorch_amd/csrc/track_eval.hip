// Tubelet AP: matching linked tracks (tubelets) against ground-truth tracks by temporal IoU, as defined in
// mega/pytorch_amd/track_eval.py (the reference has no counterpart).  Per (video, label) task with P tubelets and G GT
// tracks:
//   both(p, g) = frames where tubelet p and GT track g both have a box;  hits(p, g) = those frames where the box IoU --
//   box_math.h's vid_iou, the detection AP's, on the prediction rescaled by one f32 multiply per coordinate -- is >= 0.5f
//   (a NaN IoU is no hit);  union(p, g) = len(p) + len(g) - both(p, g);  tIoU = hits / union, never formed as a float.
//   Per threshold num / den: the tubelets in rank order (descending score, equal scores by ascending track id: the host
//   ranks them) each take the untaken GT track with hits > 0 and hits * den >= num * union of the largest tIoU
//   (hits_a * union_b > hits_b * union_a), on an equal tIoU the lowest GT track number.
//
// Task mapping: one 256-thread workgroup per task, tasks in descending box count (the host orders them), a plain launch
// of independent workgroups.
//   Phase 1: the threads walk the task's tubelet boxes; each looks at the GT boxes of its frame and label and adds to the
//   pair's `both` and, on a hit, `hits` with plain atomicAdd -- on two i32 tables in LDS when P * G <= TE_LDS_PAIRS
//   (2 x 16 KiB: four workgroups of this kernel fit a CU's 160 KiB beside each other), else on the task's slice of the
//   caller's workspace, zeroed by the workgroup first.
//   Phase 2: one wave per threshold (waves beyond R idle; thresholds beyond four go round).  Lanes hold GT tracks, in
//   chunks of 64 beyond a wave: a lane keeps the best candidate of its chunks, a shuffle butterfly the wave's, compared
//   in cross-multiplied 64-bit integers.  The taken flags are one 64-bit word per lane and threshold (bit = chunk).
//   No barrier after phase 1's.
// Every index read from a device table is checked against the sizes the host passed before it addresses memory; a task
// whose table entries do not fit is skipped (its outputs keep the caller's initial values).  No status word, no read-back.
#include "box_math.h"
#include "common.h"
#include "workspace.h"

namespace {

constexpr int TE_THREADS = 256;
constexpr int TE_WAVES = TE_THREADS / 64;
constexpr int TE_LDS_PAIRS = 4096;     // pairs of a task whose tables stay in LDS (track_eval.LDS_PAIRS)
constexpr int TE_MAX_R = 8;            // thresholds per launch
constexpr int TE_MAX_CHUNKS = 64;      // taken flags: one 64-bit word per lane -> at most 64 x 64 GT tracks per task
constexpr int TE_TASK_INTS = 8;        // class, first frame, frames, p0, P, g0, G, 0

struct TeThresholds {
  int num[TE_MAX_R], den[TE_MAX_R];
};

struct TeSizes {
  int F, C, R;
  long long M, Gb, U, J, slots, n_pairs, ws_pairs;
};

// The pair tables of a task in the workspace were written by this workgroup's stores and device-scope atomics; they are
// read back past the vector L1.  LDS tables are read plainly.
template <bool BIG>
__device__ __forceinline__ int te_load(const int* p) {
  if (BIG) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return *p;
}

template <bool BIG>
__device__ __forceinline__ void te_task(int* t_hits, int* t_both, const float4* __restrict__ box,
                                        const int* __restrict__ frame, const int* __restrict__ rank,
                                        const long long* __restrict__ seg_off, const float2* __restrict__ ratio,
                                        const float4* __restrict__ gt_box, const int* __restrict__ gt_track,
                                        const long long* __restrict__ gt_seg_off, const int* __restrict__ tubelet,
                                        const int* __restrict__ tub_len, const int* __restrict__ gt_len,
                                        const TeThresholds thr, const TeSizes z, int c, int f0, int L, int p0, int P,
                                        int g0, int G, long long pair_off, unsigned char* __restrict__ match,
                                        int* __restrict__ matched_gt, int* __restrict__ hits_out,
                                        int* __restrict__ both_out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int PG = P * G;                 // (<= INT_MAX: checked by the caller)
  for (int i = tid; i < PG; i += TE_THREADS) {
    t_hits[i] = 0;
    t_both[i] = 0;
  }
  if (BIG) __threadfence();             // the zeros are in L2 before any wave's atomic on them
  __syncthreads();

  // ---- phase 1: both / hits of every pair
  const long long seg0 = (long long)c * z.F + f0;
  long long b0 = seg_off[seg0], b1 = seg_off[seg0 + L];
  if (b0 < 0) b0 = 0;
  if (b1 > z.M) b1 = z.M;
  for (long long i = b0 + tid; i < b1; i += TE_THREADS) {
    const int f = frame[i], rk = rank[i];
    if (f < f0 || f >= f0 + L || rk < 0 || rk >= P) continue;
    long long gs = gt_seg_off[(long long)c * z.F + f], ge = gt_seg_off[(long long)c * z.F + f + 1];
    if (gs < 0) gs = 0;
    if (ge > z.Gb) ge = z.Gb;
    if (gs >= ge) continue;
    const float4 b = box[i];
    const float rw = ratio[f].x, rh = ratio[f].y;
    // BoxList.resize: x * ratio_w, y * ratio_h in f32; then the +1 on x2 / y2 (vid_match_kernel's pb)
    const float4 pb = make_float4(b.x * rw, b.y * rh, b.z * rw + 1.0f, b.w * rh + 1.0f);
    const float pa = box_area1(pb);
    for (long long k = gs; k < ge; ++k) {
      const int gl = gt_track[k];
      if (gl < 0 || gl >= G) continue;
      const int idx = rk * G + gl;
      atomicAdd(&t_both[idx], 1);
      if (vid_iou(pb, pa, gt_box[k]) >= 0.5f) atomicAdd(&t_hits[idx], 1);      // (false on NaN)
    }
  }
  if (BIG) __threadfence();
  __syncthreads();

  if (hits_out && both_out && pair_off >= 0 && pair_off + PG <= z.n_pairs) {
    for (int i = tid; i < PG; i += TE_THREADS) {
      hits_out[pair_off + i] = te_load<BIG>(t_hits + i);
      both_out[pair_off + i] = te_load<BIG>(t_both + i);
    }
  }

  // ---- phase 2: the greedy matching, one wave per threshold
  const int nch = (G + 63) >> 6;
  for (int r = wave; r < z.R; r += TE_WAVES) {
    const long long num = thr.num[r], den = thr.den[r];
    unsigned long long taken = 0;       // bit ch: GT track ch * 64 + lane is taken
    for (int p = 0; p < P; ++p) {
      const int u = tubelet[p0 + p];    // wave-uniform
      if (u < 0 || u >= z.U) continue;
      const long long plen = tub_len[u];
      int bh = 0, bu = 1, bg = -1;      // the best candidate: hits, union, GT track
      for (int ch = 0; ch < nch; ++ch) {
        const int g = ch * 64 + lane;
        if (g >= G || ((taken >> ch) & 1)) continue;
        const int h = te_load<BIG>(t_hits + p * G + g);
        if (h <= 0) continue;
        const long long un = plen + gt_len[g0 + g] - te_load<BIG>(t_both + p * G + g);
        if (un <= 0 || un > 0x7fffffffLL || h * den < num * un) continue;
        if (bg < 0 || (long long)h * bu > (long long)bh * un) {     // (strict: an equal tIoU keeps the lower chunk)
          bh = h;
          bu = (int)un;
          bg = g;
        }
      }
      if (__ballot(bg >= 0) != 0) {
        for (int o = 32; o > 0; o >>= 1) {
          const int oh = __shfl_xor(bh, o, 64), ou = __shfl_xor(bu, o, 64), og = __shfl_xor(bg, o, 64);
          if (og < 0) continue;
          const long long a = (long long)oh * bu, b = (long long)bh * ou;
          if (bg < 0 || a > b || (a == b && og < bg)) {
            bh = oh;
            bu = ou;
            bg = og;
          }
        }
        if (bg >= 0 && lane == (bg & 63)) taken |= 1ull << (bg >> 6);
      }
      if (lane == 0) {
        match[(long long)r * z.U + u] = bg >= 0 ? 1 : 0;
        matched_gt[(long long)r * z.U + u] = bg >= 0 ? g0 + bg : -1;
      }
    }
  }
}

__global__ __launch_bounds__(TE_THREADS) void tubelet_match_kernel(
    const float4* __restrict__ box, const int* __restrict__ frame, const int* __restrict__ rank,
    const long long* __restrict__ seg_off, const float2* __restrict__ ratio, const float4* __restrict__ gt_box,
    const int* __restrict__ gt_track, const long long* __restrict__ gt_seg_off, const int* __restrict__ tasks,
    const long long* __restrict__ offs, const int* __restrict__ tubelet, const int* __restrict__ tub_len,
    const int* __restrict__ gt_len, const TeThresholds thr, const TeSizes z, unsigned char* __restrict__ match,
    int* __restrict__ matched_gt, int* __restrict__ hits_out, int* __restrict__ both_out, int* ws_hits, int* ws_both) {
  __shared__ int s_hits[TE_LDS_PAIRS], s_both[TE_LDS_PAIRS];
  const int* tk = tasks + (long long)blockIdx.x * TE_TASK_INTS;
  const int c = tk[0], f0 = tk[1], L = tk[2], p0 = tk[3], P = tk[4], g0 = tk[5], G = tk[6];
  // (block-uniform: a task that does not fit the sizes is skipped as a whole)
  if (c < 0 || c >= z.C || f0 < 0 || L <= 0 || L > z.F - f0 || p0 < 0 || P <= 0 || P > z.slots - p0 || g0 < 0 || G <= 0 ||
      G > z.J - g0 || G > TE_MAX_CHUNKS * 64 || (long long)P * G > 0x7fffffffLL)
    return;
  const long long PG = (long long)P * G;
  const long long pair_off = offs[(long long)blockIdx.x * 2], ws_off = offs[(long long)blockIdx.x * 2 + 1];
  if (PG > TE_LDS_PAIRS) {
    if (ws_off < 0 || ws_off > z.ws_pairs - PG) return;
    te_task<true>(ws_hits + ws_off, ws_both + ws_off, box, frame, rank, seg_off, ratio, gt_box, gt_track, gt_seg_off,
                  tubelet, tub_len, gt_len, thr, z, c, f0, L, p0, P, g0, G, pair_off, match, matched_gt, hits_out,
                  both_out);
  } else {
    te_task<false>(s_hits, s_both, box, frame, rank, seg_off, ratio, gt_box, gt_track, gt_seg_off, tubelet, tub_len,
                   gt_len, thr, z, c, f0, L, p0, P, g0, G, pair_off, match, matched_gt, hits_out, both_out);
  }
}

// One thread per tubelet: its members' f32 scores (sorted by tubelet, then frame) added in f64 in that order, / count;
// or the largest of them.
__global__ __launch_bounds__(TE_THREADS) void tubelet_score_kernel(const float* __restrict__ score,
                                                                    const long long* __restrict__ off, long long U,
                                                                    long long M, int use_max,
                                                                    double* __restrict__ out) {
  const long long u = (long long)blockIdx.x * TE_THREADS + threadIdx.x;
  if (u >= U) return;
  long long s = off[u], e = off[u + 1];
  if (s < 0) s = 0;
  if (e > M) e = M;
  if (s >= e) {
    out[u] = 0.0;
    return;
  }
  if (use_max) {
    float m = score[s];
    for (long long i = s + 1; i < e; ++i) m = fmaxf(m, score[i]);
    out[u] = (double)m;
  } else {
    double acc = 0.0;
    for (long long i = s; i < e; ++i) acc += (double)score[i];
    out[u] = acc / (double)(e - s);
  }
}

// The pair tables of the tasks that do not fit LDS: ws_pairs entries each.
struct TeWorkspace {
  int* hits; int* both;
  size_t bytes;
};

TeWorkspace te_carve(void* ws, long long ws_pairs) {
  WsCarver c(ws);
  const size_t n = ws_pairs > 0 ? (size_t)ws_pairs : 0;
  return {c.take<int>(n), c.take<int>(n), c.bytes};
}

}  // namespace

extern "C" size_t mega_tubelet_match_workspace_bytes(long long ws_pairs) {
  if (ws_pairs <= 0) return 0;
  return te_carve(nullptr, ws_pairs).bytes;
}

extern "C" int mega_tubelet_match(const float* box, const int* frame, const int* rank, const long long* seg_off,
                                  const float* ratio, const float* gt_box, const int* gt_track,
                                  const long long* gt_seg_off, const int* tasks, const long long* offs,
                                  const int* tubelet, const int* tub_len, const int* gt_len, const int* thresholds, int T,
                                  int F, int C, int R, long long M, long long Gb, long long U, long long J,
                                  long long slots, long long n_pairs, long long ws_pairs, unsigned char* match,
                                  int* matched_gt, int* hits, int* both, void* ws, size_t ws_bytes, void* stream) {
  mega_clear_error();
  if (T < 0 || F < 0 || C < 0 || R <= 0 || R > TE_MAX_R || M < 0 || Gb < 0 || U < 0 || J < 0 || slots < 0 || n_pairs < 0 ||
      ws_pairs < 0 || !thresholds)
    return MEGA_ERR_ARG;
  TeThresholds thr;
  for (int r = 0; r < TE_MAX_R; ++r) {
    thr.num[r] = r < R ? thresholds[2 * r] : 1;
    thr.den[r] = r < R ? thresholds[2 * r + 1] : 1;
    if (!(0 < thr.num[r] && thr.num[r] <= thr.den[r] && thr.den[r] <= 1024)) return MEGA_ERR_ARG;
  }
  if (F > 0x3fffffff || M > 0x7fffffffLL || Gb > 0x7fffffffLL || U > 0x7fffffffLL || J > 0x7fffffffLL ||
      slots > 0x7fffffffLL || T > 0x7fffffff / TE_TASK_INTS || (long long)C * F >= 0x7fffffffLL)
    return MEGA_ERR_ARG;
  if ((hits == nullptr) != (both == nullptr)) return MEGA_ERR_ARG;
  if (T == 0) return MEGA_OK;                            // nothing to match
  if (!box || !frame || !rank || !seg_off || !ratio || !gt_box || !gt_track || !gt_seg_off || !tasks || !offs ||
      !tubelet || !tub_len || !gt_len || !match || !matched_gt || F == 0 || C == 0 || M == 0 || Gb == 0 || U == 0 ||
      J == 0 || slots == 0)
    return MEGA_ERR_ARG;
  if (ws_pairs > 0 && !ws) return MEGA_ERR_ARG;
  if (ws_bytes < mega_tubelet_match_workspace_bytes(ws_pairs)) return MEGA_ERR_WS;
  const TeWorkspace w = te_carve(ws, ws_pairs);
  const TeSizes z = {F, C, R, M, Gb, U, J, slots, n_pairs, ws_pairs};
  hipLaunchKernelGGL(tubelet_match_kernel, dim3(T), dim3(TE_THREADS), 0, (hipStream_t)stream, (const float4*)box, frame,
                     rank, seg_off, (const float2*)ratio, (const float4*)gt_box, gt_track, gt_seg_off, tasks, offs, tubelet,
                     tub_len, gt_len, thr, z, match, matched_gt, hits, both, w.hits, w.both);
  return mega_check_launch();
}

extern "C" int mega_tubelet_scores(const float* score, const long long* off, long long U, long long M, int use_max,
                                   double* out, void* stream) {
  mega_clear_error();
  if (U < 0 || M < 0 || U > 0x7fffffffLL || M > 0x7fffffffLL || (use_max != 0 && use_max != 1)) return MEGA_ERR_ARG;
  if (U == 0) return MEGA_OK;
  if (!score || !off || !out || M == 0) return MEGA_ERR_ARG;
  hipLaunchKernelGGL(tubelet_score_kernel, dim3((unsigned)((U + TE_THREADS - 1) / TE_THREADS)), dim3(TE_THREADS), 0,
                     (hipStream_t)stream, score, off, U, M, use_max, out);
  return mega_check_launch();
}
