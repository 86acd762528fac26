// Seq-NMS (Han et al., 2016) video-level rescoring of per-frame detections, as defined in mega/pytorch_amd/seq_nms.py
// (the reference has no counterpart).  Per (video, class) task, until no box of the task is alive:
//   1. forward DP in f64: S(t,i) = s(t,i) + max{ S(t-1,j) : j alive in t-1, iou(j,i) > link_iou }  (S = s without such
//      a j); P(t,i) = the arg-max j, the smallest position on equal S, -1 without a j;
//   2. the alive box with the largest S, on equal S the earliest frame, then the smallest position; backtrack through P;
//   3. rescore the path: avg -> f32(S* / path length) (f64 division), max -> the largest original score on the path;
//   4. in every path frame remove the path box and every alive box k with iou(k, path box) > nms_iou (suppressed).
// IoU: box_math.h's box_iou1 -- the legacy +1 convention in f32 (built with -ffp-contract=off: no FMA contraction):
//   area(b) = (x2 - x1 + 1) * (y2 - y1 + 1);  w = max(min(x2) - max(x1) + 1, 0), h likewise;  inter / ((aa + ab) - inter)
// A NaN IoU neither links nor suppresses.
//
// Task mapping: one 256-thread workgroup per task, tasks in descending box count (the host orders them), a plain
// launch of independent workgroups.  A task's boxes are contiguous in the class-major / frame-minor order the host sorts
// them into; seg_off[c * F + f] is where (class c, frame f) starts.  Per-box state lives in global memory (S f64, P i32,
// a state byte); links are recomputed on the fly inside every DP step (no link storage).
// Incremental DP: after a removal in frames [t0, t*] the DP restarts at t0, always recomputes up to t*, and after t*
// stops at the first frame whose alive boxes' S did not change (the next frame's inputs are then unchanged).  A
// per-frame best (S, position) is kept for step 2; its reduction over frames takes the earliest frame on equal S.
#include <climits>

#include "box_math.h"
#include "common.h"
#include "workspace.h"

namespace {

constexpr int SN_THREADS = 256;
constexpr int SN_WAVES = SN_THREADS / 64;
constexpr unsigned char SN_ALIVE = 1;
constexpr unsigned char SN_PATH = 2;

// (s, p) beats (bs, bp): larger S, on equal S the smaller index.  The "none" value is (-inf, INT_MAX).
__device__ __forceinline__ bool sn_better(double s, int p, double bs, int bp) { return s > bs || (s == bs && p < bp); }

__device__ __forceinline__ void sn_wave_best(double& s, int& p) {
  for (int o = 32; o > 0; o >>= 1) {
    const double os = __shfl_xor(s, o, 64);
    const int op = __shfl_xor(p, o, 64);
    if (sn_better(os, op, s, p)) { s = os; p = op; }
  }
}

// Block-wide best (s, p); every thread gets the result.  lds_s / lds_p: SN_WAVES entries of a buffer the caller
// alternates between consecutive calls (no trailing barrier).
__device__ __forceinline__ void sn_block_best(double& s, int& p, double* lds_s, int* lds_p) {
  sn_wave_best(s, p);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { lds_s[w] = s; lds_p[w] = p; }
  __syncthreads();
  s = lds_s[0];
  p = lds_p[0];
  for (int k = 1; k < SN_WAVES; ++k)
    if (sn_better(lds_s[k], lds_p[k], s, p)) { s = lds_s[k]; p = lds_p[k]; }
}

// One DP frame step: S / P of the alive boxes of frame t (nt boxes from a0) from frame t-1 (np boxes from p0), the
// frame's best (S, position) into fbS / fbP.  The (i, j) pairs: g consecutive lanes share a box i and stride over j,
// then reduce in a butterfly (g a power of two <= 64, as many as frame t leaves room for in 256 threads); frames with
// more boxes loop over chunks of 256 / g boxes.  Returns (block-uniform) whether an alive box's S changed.
__device__ bool sn_frame_step(const float4* __restrict__ box, const float* __restrict__ score, double* S, int* P,
                              const unsigned char* state, long long a0, int nt,
                              long long p0, int np, float link, double* fbS, int* fbP, double* lds_s, int* lds_p) {
  int g = 1;
  while (g < 64 && g < np && nt * (g * 2) <= SN_THREADS) g <<= 1;
  const int per = SN_THREADS / g;
  const int r = threadIdx.x & (g - 1);
  double fs = -INFINITY;     // this thread's best (S, i) over its chunks (i ascending: strict > keeps the smallest)
  int fp = INT_MAX;
  int changed = 0;
  for (int base = 0; base < nt; base += per) {
    const int i = base + (int)threadIdx.x / g;
    const bool valid = i < nt && (state[a0 + i] & SN_ALIVE);
    double bs = -INFINITY;
    int bj = INT_MAX;
    if (valid) {
      const float4 bi = box[a0 + i];
      for (int j = r; j < np; j += g) {
        if (!(state[p0 + j] & SN_ALIVE)) continue;
        if (box_iou1(box[p0 + j], bi) > link) {
          const double sj = S[p0 + j];
          if (sj > bs) { bs = sj; bj = j; }
        }
      }
    }
    for (int o = g >> 1; o > 0; o >>= 1) {
      const double os = __shfl_xor(bs, o, 64);
      const int oj = __shfl_xor(bj, o, 64);
      if (sn_better(os, oj, bs, bj)) { bs = os; bj = oj; }
    }
    if (valid && r == 0) {
      const double s0 = (double)score[a0 + i];
      const double s = bj != INT_MAX ? s0 + bs : s0;
      changed |= S[a0 + i] != s;
      S[a0 + i] = s;
      P[a0 + i] = bj != INT_MAX ? bj : -1;
      if (s > fs) { fs = s; fp = i; }
    }
  }
  sn_block_best(fs, fp, lds_s, lds_p);
  changed = __syncthreads_or(changed);
  if (threadIdx.x == 0) { *fbS = fs; *fbP = fp; }
  return changed != 0;
}

__global__ __launch_bounds__(SN_THREADS) void seq_nms_kernel(
    const float4* __restrict__ box, const float* __restrict__ score, const long long* __restrict__ seg_off,
    const int* __restrict__ tasks, int F, float link, float nms, int rescore_max, unsigned char* state, float* new_score,
    long long* stats, double* S, int* P, double* fbS, int* fbP, int* path_pos, int* status) {
  // (the per-box / per-frame state is written and re-read across barriers: no __restrict__ on those pointers)
  __shared__ double lds_s[2][SN_WAVES];
  __shared__ int lds_p[2][SN_WAVES];
  __shared__ double sh_val;
  __shared__ int sh_t0, sh_t1, sh_len;
  const int c = tasks[blockIdx.x * 3], f0 = tasks[blockIdx.x * 3 + 1], L = tasks[blockIdx.x * 3 + 2];
  const long long seg0 = (long long)c * F + f0;         // segment of the task's frame t: seg0 + t
  const long long b0 = seg_off[seg0], b1 = seg_off[seg0 + L];
  const long long n = b1 - b0;
  for (long long k = b0 + threadIdx.x; k < b1; k += SN_THREADS) state[k] = SN_ALIVE;
  __syncthreads();

  int buf = 0;
  int lo = 0, hi = L - 1;          // frames to recompute; after hi, stop at the first frame without an S change
  long long iters = 0, steps = 0;
  for (;;) {
    // 1. forward DP from frame lo
    for (int t = lo; t < L; ++t) {
      const long long a0 = seg_off[seg0 + t];
      const int nt = (int)(seg_off[seg0 + t + 1] - a0);
      const long long p0 = t > 0 ? seg_off[seg0 + t - 1] : a0;
      const int np = t > 0 ? (int)(a0 - p0) : 0;
      const bool ch = sn_frame_step(box, score, S, P, state, a0, nt, p0, np, link, fbS + seg0 + t, fbP + seg0 + t,
                                    lds_s[buf], lds_p[buf]);
      buf ^= 1;
      ++steps;
      if (t > hi && !ch) break;
    }
    __syncthreads();     // thread 0's per-frame bests

    // 2. the best end box: largest S, then the earliest frame (strict > over ascending t), then the smallest position
    double bs = -INFINITY;
    int bt = INT_MAX;
    for (int t = threadIdx.x; t < L; t += SN_THREADS) {
      const double s = fbS[seg0 + t];
      if (s > bs) { bs = s; bt = t; }
    }
    sn_block_best(bs, bt, lds_s[buf], lds_p[buf]);
    buf ^= 1;
    if (bs == -INFINITY) break;      // no box of the task is alive (block-uniform)
    if (++iters > n) {               // each iteration removes at least one box: never taken
      if (threadIdx.x == 0) atomicOr(status, 1);
      break;
    }

    // backtrack (one thread), then 3. rescore value
    if (threadIdx.x == 0) {
      int t = bt, i = fbP[seg0 + bt], len = 0;
      float mx = -INFINITY;
      for (;;) {
        const long long a = seg_off[seg0 + t];
        path_pos[seg0 + t] = i;
        ++len;
        mx = fmaxf(mx, score[a + i]);
        const int j = P[a + i];
        if (j < 0 || t == 0) break;
        --t;
        i = j;
      }
      sh_t0 = t;
      sh_t1 = bt;
      sh_len = len;
      sh_val = rescore_max ? (double)mx : (double)(float)(bs / (double)len);
    }
    __syncthreads();
    const int t0 = sh_t0, t1 = sh_t1, len = sh_len;
    const float val = (float)sh_val;

    // 4. suppress: long paths one thread per frame, short ones all threads over each frame's boxes
    if (len > 16) {
      for (int t = t0 + (int)threadIdx.x; t <= t1; t += SN_THREADS) {
        const long long a = seg_off[seg0 + t];
        const int nb = (int)(seg_off[seg0 + t + 1] - a);
        const int p = path_pos[seg0 + t];
        const float4 pb = box[a + p];
        for (int k = 0; k < nb; ++k)
          if (k != p && (state[a + k] & SN_ALIVE) && box_iou1(box[a + k], pb) > nms) state[a + k] = 0;
        state[a + p] = SN_PATH;
        new_score[a + p] = val;
      }
    } else {
      for (int t = t0; t <= t1; ++t) {
        const long long a = seg_off[seg0 + t];
        const int nb = (int)(seg_off[seg0 + t + 1] - a);
        const int p = path_pos[seg0 + t];
        const float4 pb = box[a + p];
        for (int k = threadIdx.x; k < nb; k += SN_THREADS) {
          if (k == p) {
            state[a + p] = SN_PATH;
            new_score[a + p] = val;
          } else if ((state[a + k] & SN_ALIVE) && box_iou1(box[a + k], pb) > nms) {
            state[a + k] = 0;
          }
        }
      }
    }
    __syncthreads();
    lo = t0;
    hi = t1;
  }
  __syncthreads();
  for (long long k = b0 + threadIdx.x; k < b1; k += SN_THREADS) state[k] = state[k] == SN_PATH ? 1 : 0;
  if (threadIdx.x == 0 && stats) {
    stats[blockIdx.x * 2] = iters;
    stats[blockIdx.x * 2 + 1] = steps;
  }
}

struct SnWorkspace {     // in this order (a braced list is evaluated left to right)
  double* S; int* P; double* fbS; int* fbP; int* path_pos; int* status;
  size_t bytes;
};

SnWorkspace sn_carve(void* ws, size_t N, size_t segs) {
  WsCarver c(ws);
  return {c.take<double>(N), c.take<int>(N), c.take<double>(segs), c.take<int>(segs), c.take<int>(segs), c.take<int>(1),
          c.bytes};
}

}  // namespace

extern "C" size_t mega_seq_nms_workspace_bytes(long long N, long long segs) {
  if (N <= 0 || segs <= 0) return 0;
  return sn_carve(nullptr, N, segs).bytes;
}

extern "C" int mega_seq_nms(const float* box, const float* score, const long long* seg_off, const int* tasks, int T,
                            int F, int C, long long N, float link_iou, float nms_iou, int rescore_max,
                            unsigned char* keep, float* new_score, long long* stats, void* ws, size_t ws_bytes,
                            void* stream) {
  mega_clear_error();
  if (!box || !score || !seg_off || !tasks || !keep || !new_score || !ws || T <= 0 || F <= 0 || C <= 0 || N <= 0)
    return MEGA_ERR_ARG;
  if (!(link_iou >= 0.0f && link_iou <= 1.0f) || !(nms_iou >= 0.0f && nms_iou <= 1.0f)) return MEGA_ERR_ARG;
  if (N > 0x7fffffffLL || T > 0x7fffffff / 3) return MEGA_ERR_ARG;
  const long long segs = (long long)C * F;
  if (ws_bytes < mega_seq_nms_workspace_bytes(N, segs)) return MEGA_ERR_WS;
  const SnWorkspace w = sn_carve(ws, N, segs);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(w.status, 0, sizeof(int), st) != hipSuccess) return MEGA_ERR_LAUNCH;
  hipLaunchKernelGGL(seq_nms_kernel, dim3(T), dim3(SN_THREADS), 0, st, (const float4*)box, score, seg_off, tasks, F,
                     link_iou, nms_iou, rescore_max, keep, new_score, stats, w.S, w.P, w.fbS, w.fbP, w.path_pos, w.status);
  return mega_check_status(w.status, st);
}
