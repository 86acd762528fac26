// ImageNet VID detection evaluation (AP50, motion-specific AP): the per-detection greedy GT matching and the
// per-class precision / recall / AP reduction of
//   mega_core/data/datasets/evaluation/vid/vid_eval.py:156-285   calc_detection_vid_prec_rec
//   mega_core/data/datasets/evaluation/vid/vid_eval.py:288-343   calc_detection_vid_ap (use_07_metric=False)
// with the box rescale of structures/bounding_box.py:91-125 (BoxList.resize) and the IoU of
// structures/boxlist_ops.py:53-89 (boxlist_iou, TO_REMOVE = 1) after vid_eval.py:209-214's +1 on x2 / y2.
//
// Built with -ffp-contract=off: every f32 operation of the rescale / IoU rounds exactly like the reference's separate
// torch ops (no FMA contraction).
#include "box_math.h"
#include "common.h"
#include "workspace.h"

namespace {

typedef unsigned long long u64;

constexpr int VE_WAVES = 4;         // waves per block of the matching kernel
constexpr int VE_MAX_CHUNKS = 64;   // selected flags: one 64-bit word per lane -> at most 64 x 64 GT boxes per frame
constexpr int AP_THREADS = 256;
constexpr int AP_PER_THREAD = 4;
constexpr int AP_CHUNK = AP_THREADS * AP_PER_THREAD;

__device__ __forceinline__ float wave_max_f(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// One GT slot's IoU with the (rescaled, +1) detection box: box_math.h's vid_iou, shared with track_eval.hip.

// torch.max / torch.min / clamp(min=0) propagate NaN; fmaxf / fminf do not.  The reference's elementwise ops are
// reproduced for NaN-free inputs by fmaxf / fminf; a NaN coordinate gives a NaN IoU either way through the
// subtraction that follows, except when the NaN is dropped by fmaxf.  Inputs are checked for NaN on the host.

struct GtSlot {
  float4 box;
  int label;
  bool ign;
  bool valid;
};

__device__ __forceinline__ GtSlot load_gt(const float4* gt_box, const int* gt_label, const double* gt_motion, long long g0,
                                          int G, int c, double lo, double hi) {
  GtSlot s;
  const int k = c * 64 + (int)(threadIdx.x & 63);
  s.valid = k < G;
  s.box = s.valid ? gt_box[g0 + k] : make_float4(0.f, 0.f, 0.f, 0.f);
  s.label = s.valid ? gt_label[g0 + k] : -1;
  const double m = (s.valid && gt_motion) ? gt_motion[g0 + k] : __builtin_nan("");
  s.ign = (m < lo) || (m > hi);     // NaN (no motion list for the frame): ignore nothing
  return s;
}

// One wave per (frame, motion range).  Lanes hold GT slots (chunks of 64 for larger frames); the wave walks the frame's
// detections in the order order[det_off[f] .. det_off[f+1]) -- label, then score descending, then position descending --
// and applies the reference's greedy rule (vid_eval.py:221-253) to each one.
__global__ __launch_bounds__(64 * VE_WAVES) void vid_match_kernel(
    const float4* __restrict__ det_box, const int* __restrict__ det_label, const long long* __restrict__ det_off,
    const int* __restrict__ order, const float2* __restrict__ ratio, const float4* __restrict__ gt_box,
    const int* __restrict__ gt_label, const double* __restrict__ gt_motion, const long long* __restrict__ gt_off,
    const double* __restrict__ ranges, int F, int R, int C, long long N, unsigned char* __restrict__ match,
    double* __restrict__ pred_ignore, int* __restrict__ n_pos) {
  const int wid = blockIdx.x * VE_WAVES + (int)(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (wid >= F * R) return;
  const int f = wid / R, r = wid % R;
  const double lo = ranges[r * 3], hi = ranges[r * 3 + 1], empty_w = ranges[r * 3 + 2];
  const long long g0 = gt_off[f];
  const int G = (int)(gt_off[f + 1] - g0);
  const int nch = (G + 63) >> 6;

  // n_pos: the non-ignored GT boxes of each class (vid_eval.py:203)
  for (int c = 0; c < nch; ++c) {
    const GtSlot s = load_gt(gt_box, gt_label, gt_motion, g0, G, c, lo, hi);
    if (s.valid && !s.ign) atomicAdd(&n_pos[r * C + s.label], 1);
  }

  const long long d0 = det_off[f], d1 = det_off[f + 1];
  if (d0 == d1) return;
  const float rw = ratio[f].x, rh = ratio[f].y;
  const GtSlot s0 = load_gt(gt_box, gt_label, gt_motion, g0, G, 0, lo, hi);   // the common case: one chunk, kept resident
  u64 selected = 0;                                                             // bit c: slot c * 64 + lane is taken

  for (long long i = d0; i < d1; ++i) {
    const int idx = order[i];
    const float4 b = det_box[idx];
    const int L = det_label[idx];
    // BoxList.resize: x * ratio_w, y * ratio_h in f32; then vid_eval.py:209-214: x2 + 1, y2 + 1
    const float4 pb = make_float4(b.x * rw, b.y * rh, b.z * rw + 1.0f, b.w * rh + 1.0f);
    const float pa = box_area1(pb);

    // pass 1: per-class maxima over ignored / non-ignored GT (selected ones included), the best candidate, NaN candidates
    float mx_ig = -1.0f, mx_nig = -1.0f, mx_cand = -INFINITY;
    int n_same = 0, n_ign = 0;
    bool nan_cand = false;
    for (int c = 0; c < nch; ++c) {
      const GtSlot s = c == 0 ? s0 : load_gt(gt_box, gt_label, gt_motion, g0, G, c, lo, hi);
      const bool same = s.valid && s.label == L;
      const float v = same ? vid_iou(pb, pa, s.box) : -1.0f;
      const bool nn = same && !__builtin_isnan(v);
      mx_ig = fmaxf(mx_ig, wave_max_f(nn && s.ign ? v : -1.0f));
      mx_nig = fmaxf(mx_nig, wave_max_f(nn && !s.ign ? v : -1.0f));
      const bool free_ = same && !((selected >> c) & 1);
      mx_cand = fmaxf(mx_cand, wave_max_f(free_ && nn && v >= 0.5f ? v : -INFINITY));
      nan_cand |= __ballot(free_ && !nn) != 0;
      n_same += __popcll(__ballot(same));
      n_ign += __popcll(__ballot(same && s.ign));
    }

    int chosen = -1;     // GT slot in the frame
    if (nan_cand) {
      // A NaN IoU (only from boxes with x2 < x1 - 1) is never skipped by vid_eval.py:232 and resets the running match
      // value: run the reference's loop itself, in slot order, on values broadcast from their lanes.
      float cur = 0.5f;
      bool cur_ig = false;
      for (int c = 0; c < nch; ++c) {
        const GtSlot s = c == 0 ? s0 : load_gt(gt_box, gt_label, gt_motion, g0, G, c, lo, hi);
        const bool same = s.valid && s.label == L;
        const float v = same ? vid_iou(pb, pa, s.box) : 0.0f;
        const u64 elig = __ballot(same && !((selected >> c) & 1));
        const u64 ign = __ballot(s.ign);
        for (int t = 0; t < 64; ++t) {
          const float vt = __shfl(v, t, 64);
          if (!((elig >> t) & 1)) continue;
          if (vt < cur) continue;
          const bool ig_t = (ign >> t) & 1;
          if (vt == cur) {
            if (chosen < 0 || cur_ig) { chosen = c * 64 + t; cur_ig = ig_t; }
          } else {
            chosen = c * 64 + t;
            cur_ig = ig_t;
          }
          cur = vt;
        }
      }
    } else if (mx_cand >= 0.5f) {
      // the maximum IoU among free candidates >= 0.5; on a tie the first non-ignored slot, else the last tied slot
      int last = -1;
      for (int c = 0; c < nch && chosen < 0; ++c) {
        const GtSlot s = c == 0 ? s0 : load_gt(gt_box, gt_label, gt_motion, g0, G, c, lo, hi);
        const bool same = s.valid && s.label == L;
        const float v = same ? vid_iou(pb, pa, s.box) : -1.0f;
        const u64 tie = __ballot(same && !((selected >> c) & 1) && v == mx_cand);
        const u64 tie_nig = tie & __ballot(!s.ign);
        if (tie_nig) chosen = c * 64 + __builtin_ctzll(tie_nig);
        else if (tie) last = c * 64 + 63 - __builtin_clzll(tie);
      }
      if (chosen < 0) chosen = last;
    }

    unsigned char m;
    double pi;
    if (chosen >= 0) {
      const int cc = chosen >> 6, cl = chosen & 63;
      const GtSlot s = cc == 0 ? s0 : load_gt(gt_box, gt_label, gt_motion, g0, G, cc, lo, hi);
      const bool ig = (__ballot(s.ign) >> cl) & 1;
      if (lane == cl) selected |= 1ull << cc;
      m = 1;
      pi = ig ? 1.0 : 0.0;
    } else if (n_same == 0) {
      m = 0;
      pi = empty_w;
    } else {
      m = 0;
      pi = mx_nig > mx_ig ? 0.0 : mx_ig > mx_nig ? 1.0 : (double)n_ign / (double)n_same;
    }
    if (lane == 0) {
      match[(long long)r * N + idx] = m;
      pred_ignore[(long long)r * N + idx] = pi;
    }
  }
}

// ---------------------------------------------------------------------------------------------- precision / recall / AP
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

__device__ __forceinline__ double wave_suffix_max(double v, int lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_down(v, o, 64);
    if (lane + o < 64) v = fmax(v, u);
  }
  return v;
}

// vid_eval.py:265-268: tp weight = match & !(ignore == 1); fp weight = (!match & !(ignore == 1)) * (ignore == 0 ? 1 : ignore)
__device__ __forceinline__ void ap_weights(const unsigned char* match, const double* pign, const int* gorder, long long i,
                                           long long end, int& wt, double& wf) {
  wt = 0;
  wf = 0.0;
  if (i < end) {
    const int d = gorder[i];
    const unsigned char m = match[d];
    const double p = pign[d];
    const bool keep = !(p == 1.0);
    wt = (m == 1 && keep) ? 1 : 0;
    wf = (m == 0 && keep) ? (p == 0.0 ? 1.0 : p) : 0.0;
  }
}

// Block-wide exclusive prefix (over threads) of each thread's total; returns the block total too.
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* lds, T& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const T incl = wave_incl_scan(v, lane);
  __syncthreads();
  if (lane == 63) lds[w] = incl;
  __syncthreads();
  T off = 0, tot = 0;
  for (int k = 0; k < AP_THREADS / 64; ++k) {
    if (k < w) off += lds[k];
    tot += lds[k];
  }
  total = tot;
  return off + incl - v;
}

// One block per (class, motion range): the class's detections in global order gorder[seg_off[l] .. seg_off[l+1]).
// Pass 1 (forward over 1024-entry chunks): the running tp / fp sums before every chunk, into the workspace.
// Pass 2 (backward over the chunks): inclusive tp (integer) / fp (f64) scans -> prec = tp / (fp + tp + 2^-52),
// rec = tp / n_pos; the precision envelope as a suffix max carried from later chunks; AP = sum over the positions where
// recall changes of (rec_j - rec_j-1) * envelope_j (vid_eval.py:330-341: the sentinels contribute 0).  f64 throughout.
__global__ __launch_bounds__(AP_THREADS) void vid_ap_kernel(const unsigned char* __restrict__ match,
                                                             const double* __restrict__ pred_ignore,
                                                             const int* __restrict__ gorder,
                                                             const long long* __restrict__ seg_off,
                                                             const int* __restrict__ n_pos, int C, long long N,
                                                             long long slots, int* __restrict__ tp_carry,
                                                             double* __restrict__ fp_carry, double* __restrict__ ap) {
  __shared__ int lds_i[AP_THREADS / 64];
  __shared__ double lds_d[AP_THREADS / 64];
  const int l = blockIdx.x, r = blockIdx.y;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int np = n_pos[r * C + l];
  if (np == 0) {   // rec is None (vid_eval.py:281) -> AP NaN (classes never seen have no GT either)
    if (threadIdx.x == 0) ap[r * C + l] = __builtin_nan("");
    return;
  }
  const unsigned char* m = match + (long long)r * N;
  const double* p = pred_ignore + (long long)r * N;
  const long long s = seg_off[l], e = seg_off[l + 1];
  const long long nchunk = (e - s + AP_CHUNK - 1) / AP_CHUNK;
  const long long base = (long long)r * slots + s / AP_CHUNK + l;   // slots of class l never overlap class l + 1's
  int* tpc = tp_carry + base;
  double* fpc = fp_carry + base;

  int run_t = 0;
  double run_f = 0.0;
  for (long long c = 0; c < nchunk; ++c) {
    int st = 0;
    double sf = 0.0;
    for (int k = 0; k < AP_PER_THREAD; ++k) {
      int wt;
      double wf;
      ap_weights(m, p, gorder, s + c * AP_CHUNK + threadIdx.x * AP_PER_THREAD + k, e, wt, wf);
      st += wt;
      sf += wf;
    }
    int tt;
    double tf;
    block_excl_scan(st, lds_i, tt);
    block_excl_scan(sf, lds_d, tf);
    if (threadIdx.x == 0) {
      tpc[c] = run_t;
      fpc[c] = run_f;
    }
    run_t += tt;
    run_f += tf;
  }
  __threadfence_block();   // thread 0's carries are read by every thread of the block below
  __syncthreads();

  const double npd = (double)np;
  const double eps = 2.220446049250313e-16;   // np.spacing(1)
  double env_carry = 0.0;                     // max precision over the chunks after this one (the 0 sentinel)
  double ap_sum = 0.0;
  for (long long c = nchunk - 1; c >= 0; --c) {
    int wt[AP_PER_THREAD];
    double wf[AP_PER_THREAD];
    int st = 0;
    double sf = 0.0;
    for (int k = 0; k < AP_PER_THREAD; ++k) {
      ap_weights(m, p, gorder, s + c * AP_CHUNK + threadIdx.x * AP_PER_THREAD + k, e, wt[k], wf[k]);
      st += wt[k];
      sf += wf[k];
    }
    int tt;
    double tf;
    const int et = block_excl_scan(st, lds_i, tt) + tpc[c];
    const double ef = block_excl_scan(sf, lds_d, tf) + fpc[c];
    double prec[AP_PER_THREAD], rec[AP_PER_THREAD], recp[AP_PER_THREAD];
    int ct = et;
    double cf = ef;
    for (int k = 0; k < AP_PER_THREAD; ++k) {
      const long long i = s + c * AP_CHUNK + threadIdx.x * AP_PER_THREAD + k;
      recp[k] = (double)ct / npd;
      ct += wt[k];
      cf += wf[k];
      prec[k] = i < e ? (double)ct / ((cf + (double)ct) + eps) : 0.0;
      rec[k] = (double)ct / npd;
    }
    // suffix max of prec within the chunk, then with the later chunks'
    double sm = 0.0;
    for (int k = AP_PER_THREAD - 1; k >= 0; --k) sm = fmax(sm, prec[k]);
    double wsm = wave_suffix_max(sm, lane);
    __syncthreads();
    if (lane == 0) lds_d[w] = wsm;
    __syncthreads();
    double after = env_carry;   // max over the threads after this one
    const double wnext = __shfl_down(wsm, 1, 64);
    if (lane < 63) after = fmax(after, wnext);
    for (int k = w + 1; k < AP_THREADS / 64; ++k) after = fmax(after, lds_d[k]);
    double chunk_max = env_carry;
    for (int k = 0; k < AP_THREADS / 64; ++k) chunk_max = fmax(chunk_max, lds_d[k]);
    double term = 0.0;
    double env = after;
    for (int k = AP_PER_THREAD - 1; k >= 0; --k) {
      env = fmax(env, prec[k]);
      if (rec[k] != recp[k]) term += (rec[k] - recp[k]) * env;
    }
    // block sum of the terms in a fixed order
    double tot;
    block_excl_scan(term, lds_d, tot);
    ap_sum += tot;
    env_carry = chunk_max;
  }
  if (threadIdx.x == 0) ap[r * C + l] = ap_sum;
}

// The running tp / fp sums before every chunk: `slots` entries per motion range.
struct ApWorkspace {
  long long slots;
  int* tp_carry; double* fp_carry;
  size_t bytes;
};

ApWorkspace ap_carve(void* ws, long long N, int C, int R) {
  WsCarver c(ws);
  const long long slots = N / AP_CHUNK + C + 1;
  return {slots, c.take<int>((size_t)R * slots), c.take<double>((size_t)R * slots), c.bytes};
}

}  // namespace

extern "C" size_t mega_vid_eval_workspace_bytes(long long N, int C, int R) {
  if (N < 0 || C <= 0 || R <= 0) return 0;
  return ap_carve(nullptr, N, C, R).bytes;
}

extern "C" int mega_vid_eval_match(const float* det_box, const int* det_label, const long long* det_off, const int* order,
                                   const float* ratio, const float* gt_box, const int* gt_label, const double* gt_motion,
                                   const long long* gt_off, const double* ranges, int F, int R, int C, long long N,
                                   int max_gt, unsigned char* match, double* pred_ignore, int* n_pos, void* stream) {
  mega_clear_error();
  if (!det_off || !ratio || !gt_off || !ranges || !n_pos || F <= 0 || R <= 0 || C <= 0 || N < 0 || max_gt < 0)
    return MEGA_ERR_ARG;
  if (N > 0 && (!det_box || !det_label || !order || !match || !pred_ignore)) return MEGA_ERR_ARG;
  if (max_gt > 0 && (!gt_box || !gt_label)) return MEGA_ERR_ARG;
  if (max_gt > VE_MAX_CHUNKS * 64 || N > 0x7fffffffLL || (long long)F * R > 0x7fffffffLL - VE_WAVES) return MEGA_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(n_pos, 0, (size_t)R * C * sizeof(int), st) != hipSuccess) return MEGA_ERR_LAUNCH;
  hipLaunchKernelGGL(vid_match_kernel, dim3(cdiv(F * R, VE_WAVES)), dim3(64 * VE_WAVES), 0, st, (const float4*)det_box,
                     det_label, det_off, order, (const float2*)ratio, (const float4*)gt_box, gt_label, gt_motion, gt_off,
                     ranges, F, R, C, N, match, pred_ignore, n_pos);
  return mega_check_launch();
}

extern "C" int mega_vid_eval_ap(const unsigned char* match, const double* pred_ignore, const int* gorder,
                                const long long* seg_off, const int* n_pos, int C, int R, long long N, double* ap, void* ws,
                                size_t ws_bytes, void* stream) {
  mega_clear_error();
  if (!seg_off || !n_pos || !ap || !ws || C <= 0 || R <= 0 || N < 0) return MEGA_ERR_ARG;
  if (N > 0 && (!match || !pred_ignore || !gorder)) return MEGA_ERR_ARG;
  if (C > 65535 * 1024 || R > 65535) return MEGA_ERR_ARG;
  if (ws_bytes < mega_vid_eval_workspace_bytes(N, C, R)) return MEGA_ERR_WS;
  const ApWorkspace w = ap_carve(ws, N, C, R);
  hipLaunchKernelGGL(vid_ap_kernel, dim3(C, R), dim3(AP_THREADS), 0, (hipStream_t)stream, match, pred_ignore, gorder,
                     seg_off, n_pos, C, N, w.slots, w.tp_carry, w.fp_carry, ap);
  return mega_check_launch();
}
