// Linking per-frame detections into tracks (tubelets), as defined in mega/pytorch_amd/tracks.py (the reference has no
// counterpart).  Per (video, class) task, frames t ascending:
//   1. close every open track whose last frame is < t - max_gap - 1;
//   2. the candidates are the frame's boxes with score >= score_thresh, in descending score (equal scores: ascending
//      position) -- the order the host sorts every (class, frame) run into, so they are a prefix of the run;
//   3. each candidate joins the open track with last frame < t of the largest iou(track's last box, candidate) > link_iou
//      (strict; equal IoU: the track whose root has the smallest position in the frame-by-frame concatenation), or opens
//      a new track with itself as the root.  A track extended or born in frame t is not available in frame t.
// IoU: Seq-NMS's, box_math.h's box_iou1 (the legacy +1 convention in f32, built with -ffp-contract=off).
// A NaN IoU never links.
//
// Task mapping: one 256-thread workgroup (4 waves of 64) per task, tasks in descending box count (the host orders them),
// a plain launch of independent workgroups.  The open-track table (last box, last frame, root, root position, box count,
// f64 score sum, score max) is a structure of arrays: entries below LT_LDS_TRACKS in LDS, the rest in the task's slice of
// the caller's workspace (max_open - LT_LDS_TRACKS entries per task).  Entry j belongs to thread j % 256: only that
// thread reads it in the candidate scans and only that thread updates or creates it, so a candidate costs ONE barrier
// (the one inside the block-wide arg-max); the compaction, which moves entries between owners, ends with a barrier.
// Closing is an order-preserving in-place compaction (ballot prefix per wave, LDS across waves); the result does not
// depend on the table order at all, since the arg-max ties go by root position, which is unique per track.  Frames
// without a candidate are skipped: a track that is closable at t stays closable at every later frame.
// Every loop runs to a count known on entry (frames, boxes of a frame, open tracks <= max_open); a task that would open
// more than max_open tracks sets the status word instead (MEGA_ERR_LIMIT).
#include <climits>

#include "box_math.h"
#include "common.h"
#include "workspace.h"

namespace {

constexpr int LT_THREADS = 256;
constexpr int LT_WAVES = LT_THREADS / 64;
constexpr int LT_LDS_TRACKS = 1024;      // 44 bytes per entry: 44 KiB of LDS

struct LtEntry {
  float4 box;      // the track's last box
  int last;        // its frame (relative to the task's first frame)
  int root;        // index of the track's first box in the sorted arrays
  int pos;         // that box's position in the frame-by-frame concatenation (the tie key)
  int cnt;
  double sum;      // the members' scores, added in frame order
  float mx;
};

// (iou, pos, idx) beats (biou, bpos, .): larger IoU, on equal IoU the smaller root position.  "None" is (-inf, INT_MAX, -1).
__device__ __forceinline__ bool lt_better(float iou, int pos, float biou, int bpos) {
  return iou > biou || (iou == biou && pos < bpos);
}

__global__ __launch_bounds__(LT_THREADS) void link_tracks_kernel(
    const float4* __restrict__ box, const float* __restrict__ score, const int* __restrict__ pos,
    const long long* __restrict__ seg_off, const int* __restrict__ tasks, int F, float thresh, float link, int max_gap,
    int max_open, long long* root_out, int* cnt_out, double* sum_out, float* max_out, float4* g_box, int* g_last,
    int* g_root, int* g_pos, int* g_cnt, double* g_sum, float* g_mx, int* status) {
  __shared__ float4 s_box[LT_LDS_TRACKS];
  __shared__ double s_sum[LT_LDS_TRACKS];
  __shared__ int s_last[LT_LDS_TRACKS], s_root[LT_LDS_TRACKS], s_pos[LT_LDS_TRACKS], s_cnt[LT_LDS_TRACKS];
  __shared__ float s_mx[LT_LDS_TRACKS];
  __shared__ float r_iou[2][LT_WAVES];
  __shared__ int r_pos[2][LT_WAVES], r_idx[2][LT_WAVES], r_scan[2][LT_WAVES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = tasks[blockIdx.x * 3], f0 = tasks[blockIdx.x * 3 + 1], L = tasks[blockIdx.x * 3 + 2];
  const long long seg0 = (long long)c * F + f0;         // segment of the task's frame t: seg0 + t
  const long long b0 = seg_off[seg0], b1 = seg_off[seg0 + L];
  const long long over = max_open > LT_LDS_TRACKS ? max_open - LT_LDS_TRACKS : 0;
  const long long g0 = (long long)blockIdx.x * over;
  // The open-track table: entry j in LDS for j < LT_LDS_TRACKS, else entry j - LT_LDS_TRACKS of the task's workspace slice
  // (whole entries here; the per-candidate scan below reads each half of the table in a loop of its own).
  g_box += g0; g_last += g0; g_root += g0; g_pos += g0; g_cnt += g0; g_sum += g0; g_mx += g0;
  const auto tab_get = [=](int j) {
    LtEntry e;
    if (j < LT_LDS_TRACKS) {
      e.box = s_box[j]; e.last = s_last[j]; e.root = s_root[j]; e.pos = s_pos[j]; e.cnt = s_cnt[j]; e.sum = s_sum[j];
      e.mx = s_mx[j];
    } else {
      const int k = j - LT_LDS_TRACKS;
      e.box = g_box[k]; e.last = g_last[k]; e.root = g_root[k]; e.pos = g_pos[k]; e.cnt = g_cnt[k]; e.sum = g_sum[k];
      e.mx = g_mx[k];
    }
    return e;
  };
  const auto tab_put = [=](int j, const LtEntry& e) {
    if (j < LT_LDS_TRACKS) {
      s_box[j] = e.box; s_last[j] = e.last; s_root[j] = e.root; s_pos[j] = e.pos; s_cnt[j] = e.cnt; s_sum[j] = e.sum;
      s_mx[j] = e.mx;
    } else {
      const int k = j - LT_LDS_TRACKS;
      g_box[k] = e.box; g_last[k] = e.last; g_root[k] = e.root; g_pos[k] = e.pos; g_cnt[k] = e.cnt; g_sum[k] = e.sum;
      g_mx[k] = e.mx;
    }
  };
  for (long long k = b0 + tid; k < b1; k += LT_THREADS) root_out[k] = -1;
  __syncthreads();       // (a member's root is written later by the entry's owner, another thread)

  int n_open = 0;        // block-uniform
  int rb = 0, sb = 0;    // which of the two arg-max / scan scratch buffers the next use takes
  bool failed = false;
  for (int t = 0; t < L && !failed; ++t) {
    const long long a0 = seg_off[seg0 + t];
    const int nt = (int)(seg_off[seg0 + t + 1] - a0);
    if (nt <= 0 || !(score[a0] >= thresh)) continue;      // no candidate: nothing to link, closing can wait

    // 1. close: keep the entries with last >= t - max_gap - 1, in order, in place (destination <= source; a chunk's
    //    entries are all in registers before its barrier, and a later chunk never writes into a chunk not yet read)
    const int keep_from = t - max_gap - 1;                // >= INT_MIN: t >= 0, max_gap >= 0
    int n_new = 0;
    for (int base = 0; base < n_open; base += LT_THREADS) {
      const int j = base + tid;
      LtEntry e;
      bool keep = false;
      if (j < n_open) {
        e = tab_get(j);
        keep = e.last >= keep_from;
      }
      const unsigned long long m = __ballot(keep);
      if (lane == 0) r_scan[sb][wave] = __popcll(m);
      __syncthreads();
      int before = n_new, total = 0;
      for (int w = 0; w < LT_WAVES; ++w) {
        const int n = r_scan[sb][w];
        if (w < wave) before += n;
        total += n;
      }
      sb ^= 1;
      const int dst = before + __popcll(m & ((1ull << lane) - 1ull));
      if (keep && dst != j) tab_put(dst, e);
      n_new += total;
    }
    n_open = n_new;
    __syncthreads();       // moved entries have new owners
    const int n0 = n_open; // tracks born in this frame go behind n0 and are not scanned in this frame

    // 2. / 3. the candidates, in order
    for (int k = 0; k < nt; ++k) {
      const long long i = a0 + k;
      const float s = score[i];
      if (!(s >= thresh)) break;
      const float4 cb = box[i];
      float biou = -INFINITY;
      int bpos = INT_MAX, bidx = -1;
      const auto consider = [&](int j, int last, float4 tb, int p) {
        if (last >= t) return;                            // extended in this frame
        const float iou = box_iou1(tb, cb);
        if (iou > link && lt_better(iou, p, biou, bpos)) { biou = iou; bpos = p; bidx = j; }
      };
      // (two loops, so that each half of the table is read with its own kind of load)
      const int n_lds = n0 < LT_LDS_TRACKS ? n0 : LT_LDS_TRACKS;
      for (int j = tid; j < n_lds; j += LT_THREADS) consider(j, s_last[j], s_box[j], s_pos[j]);
      for (int j = LT_LDS_TRACKS + tid; j < n0; j += LT_THREADS)
        consider(j, g_last[j - LT_LDS_TRACKS], g_box[j - LT_LDS_TRACKS], g_pos[j - LT_LDS_TRACKS]);
      // block-wide arg-max: a shuffle butterfly per wave, then LDS across the waves
      for (int o = 32; o > 0; o >>= 1) {
        const float oi = __shfl_xor(biou, o, 64);
        const int op = __shfl_xor(bpos, o, 64);
        const int ox = __shfl_xor(bidx, o, 64);
        if (lt_better(oi, op, biou, bpos)) { biou = oi; bpos = op; bidx = ox; }
      }
      if (lane == 0) { r_iou[rb][wave] = biou; r_pos[rb][wave] = bpos; r_idx[rb][wave] = bidx; }
      __syncthreads();
      biou = r_iou[rb][0]; bpos = r_pos[rb][0]; bidx = r_idx[rb][0];
      for (int w = 1; w < LT_WAVES; ++w)
        if (lt_better(r_iou[rb][w], r_pos[rb][w], biou, bpos)) { biou = r_iou[rb][w]; bpos = r_pos[rb][w]; bidx = r_idx[rb][w]; }
      rb ^= 1;

      if (bidx >= 0) {                     // join: the entry's owner updates it
        if ((bidx & (LT_THREADS - 1)) == tid) {
          LtEntry e = tab_get(bidx);
          e.box = cb;
          e.last = t;
          e.cnt += 1;
          e.sum += (double)s;
          e.mx = fmaxf(e.mx, s);
          tab_put(bidx, e);
          root_out[i] = e.root;
          cnt_out[e.root] = e.cnt;
          sum_out[e.root] = e.sum;
          max_out[e.root] = e.mx;
        }
      } else {                             // a new track behind the table's end
        if (n_open >= max_open) {          // never taken with the bound the caller computed (block-uniform)
          if (tid == 0) atomicOr(status, 1);
          failed = true;
          break;
        }
        if ((n_open & (LT_THREADS - 1)) == tid) {
          LtEntry e;
          e.box = cb;
          e.last = t;
          e.root = (int)i;
          e.pos = pos[i];
          e.cnt = 1;
          e.sum = (double)s;
          e.mx = s;
          tab_put(n_open, e);
          root_out[i] = i;
          cnt_out[i] = 1;
          sum_out[i] = e.sum;
          max_out[i] = s;
        }
        ++n_open;
      }
    }
  }
}

struct LtWorkspace {
  float4* box; double* sum; int* last; int* root; int* pos; int* cnt; float* mx; int* status;
  size_t bytes;
};

LtWorkspace lt_carve(void* ws, int T, int max_open) {
  const size_t over = max_open > LT_LDS_TRACKS ? (size_t)(max_open - LT_LDS_TRACKS) : 0;
  const size_t n = (size_t)(T > 0 ? T : 0) * over;
  WsCarver c(ws);      // (a braced list is evaluated left to right: the struct's order)
  return {c.take<float4>(n), c.take<double>(n), c.take<int>(n), c.take<int>(n), c.take<int>(n), c.take<int>(n),
          c.take<float>(n), c.take<int>(1), c.bytes};
}

}  // namespace

extern "C" size_t mega_link_tracks_workspace_bytes(int T, int max_open) {
  if (T <= 0 || max_open <= 0) return 0;
  return lt_carve(nullptr, T, max_open).bytes;
}

extern "C" int mega_link_tracks(const float* box, const float* score, const int* pos, const long long* seg_off,
                                const int* tasks, int T, int F, int C, long long N, float score_thresh, float link_iou,
                                int max_gap, int max_open, long long* root, int* cnt, double* sum, float* mx, void* ws,
                                size_t ws_bytes, void* stream) {
  mega_clear_error();
  if (T < 0 || F < 0 || C < 0 || N < 0 || max_gap < 0 || max_open < 0) return MEGA_ERR_ARG;
  if (!(link_iou >= 0.0f && link_iou <= 1.0f) || score_thresh != score_thresh) return MEGA_ERR_ARG;
  if (N > 0x7fffffffLL || T > 0x7fffffff / 3) return MEGA_ERR_ARG;
  if (N == 0 || T == 0) return MEGA_OK;                  // nothing to link
  if (!box || !score || !pos || !seg_off || !tasks || !root || !cnt || !sum || !mx || !ws || F == 0 || C == 0 ||
      max_open == 0)
    return MEGA_ERR_ARG;
  if (ws_bytes < mega_link_tracks_workspace_bytes(T, max_open)) return MEGA_ERR_WS;
  const LtWorkspace w = lt_carve(ws, T, max_open);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(w.status, 0, sizeof(int), st) != hipSuccess) return MEGA_ERR_LAUNCH;
  hipLaunchKernelGGL(link_tracks_kernel, dim3(T), dim3(LT_THREADS), 0, st, (const float4*)box, score, pos, seg_off, tasks,
                     F, score_thresh, link_iou, max_gap, max_open, root, cnt, sum, mx, w.box, w.last, w.root, w.pos,
                     w.cnt, w.sum, w.mx, w.status);
  return mega_check_status(w.status, st);
}
