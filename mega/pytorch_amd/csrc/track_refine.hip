// Refining linked tracks, as defined in mega/pytorch_amd/tracks.py (the reference has no counterpart): the gap frames of a
// track are filled by linear interpolation between the two members that bracket them, and every box of a track is
// replaced by the mean of the track's boxes within r frames of it.
//   Members: the boxes with a track id, sorted by (video, track id, frame); track k's members are m_off[k] .. m_off[k+1].
//   Slots: the output boxes of the tracks in the same order; track k's slots are o_off[k] .. o_off[k+1]: with fill one per
//   frame from its first member's frame to its last member's, without fill one per member.
//   Filling, per coordinate in f32 (built with -ffp-contract=off): w = f32(f - fa) / f32(fb - fa), c = a.c + (b.c - a.c) * w;
//   score = min(a.score, b.score) * fill_scale.
//   Smoothing (r > 0): the unsmoothed f32 coordinates of the track's slots s' with |frame(s') - frame(s)| <= r, added in
//   f64 in ascending frame order starting from the first of them, divided by their count in f64, rounded once to f32.
//
// Mapping: a plain launch of independent 256-thread workgroups, each owning a tile of 256 consecutive slots.  For the tile
// plus a halo of r slots on each side a workgroup finds each slot's track (binary search in o_off) and its bracketing
// members (binary search over the track's member frames) and writes the slot's unsmoothed box, frame and track into LDS;
// after ONE barrier each thread forms its tile slot's window sum from LDS.  The frames of a track's slots ascend strictly,
// so a slot within r frames is within r slots: the halo holds every window.  Neighbouring tracks share tiles and halos; a
// window takes only the entries whose track is the slot's own.  Every member is read from HBM once per tile that holds it
// (plus the halos) and every output is written once.  No atomics, no status word: the same bits on every run.
// Every loop runs to a bound known on entry (the searches at most 32 halvings, the window 2 r + 1 entries).
// Every index read from a device table is checked against the sizes the host passed before it addresses memory; a slot
// whose table entries do not fit is written as belonging to no track (track -1, everything else zero).
#include "common.h"

namespace {

constexpr int RT_THREADS = 256;
constexpr int RT_MAX_R = 64;
constexpr int RT_ENTRIES = RT_THREADS + 2 * RT_MAX_R;      // tile + both halos: 32 bytes each, 12 KiB of LDS

// The largest i in [lo, hi] with key[i] <= v; key ascends and key[lo] <= v.
template <typename T> __device__ __forceinline__ long long rt_last_le(const T* __restrict__ key, long long lo, long long hi,
                                                                        long long v) {
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const long long mid = lo + (hi - lo + 1) / 2;
    if ((long long)key[mid] <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(RT_THREADS) void refine_tracks_kernel(
    const float4* __restrict__ m_box, const float* __restrict__ m_score, const int* __restrict__ m_frame,
    const long long* __restrict__ m_off, const long long* __restrict__ o_off, int K, long long M, long long S, int fill,
    int r, float fill_scale, float4* __restrict__ out_box, float* __restrict__ out_score, int* __restrict__ out_frame,
    int* __restrict__ out_track, int* __restrict__ out_src, unsigned char* __restrict__ out_filled) {
  __shared__ float4 s_box[RT_ENTRIES];
  __shared__ float s_score[RT_ENTRIES];
  __shared__ int s_frame[RT_ENTRIES], s_track[RT_ENTRIES], s_src[RT_ENTRIES];

  const int tid = threadIdx.x;
  const long long t0 = (long long)blockIdx.x * RT_THREADS;
  const int n = RT_THREADS + 2 * r;                       // entry e is slot t0 - r + e
  for (int e = tid; e < n; e += RT_THREADS) {
    const long long s = t0 - r + e;
    int k = -1, frame = 0, src = -1;
    float4 box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float score = 0.0f;
    if (s >= 0 && s < S) {
      k = (int)rt_last_le(o_off, 0, K - 1, s);
      const long long j0 = m_off[k], j1 = m_off[k + 1], d = s - o_off[k];
      if (j0 < 0 || j1 > M || j1 <= j0 || d < 0 || d > 0x7fffffffLL) {
        k = -1;
      } else if (!fill) {                                 // slot d is member d
        if (j0 + d < j1) {
          src = (int)(j0 + d);
          box = m_box[src]; score = m_score[src]; frame = m_frame[src];
        } else {
          k = -1;
        }
      } else {                                            // slot d is frame first + d
        const long long f = (long long)m_frame[j0] + d;
        const long long ja = rt_last_le(m_frame, j0, j1 - 1, f);
        const int fa = m_frame[ja];
        frame = (int)f;
        if (fa == f) {
          src = (int)ja;
          box = m_box[ja]; score = m_score[ja];
        } else if (ja + 1 < j1 && fa < f && m_frame[ja + 1] > f) {
          const float4 a = m_box[ja], b = m_box[ja + 1];
          const float w = (float)(int)(f - fa) / (float)(m_frame[ja + 1] - fa);
          box = make_float4(a.x + (b.x - a.x) * w, a.y + (b.y - a.y) * w, a.z + (b.z - a.z) * w, a.w + (b.w - a.w) * w);
          score = fminf(m_score[ja], m_score[ja + 1]) * fill_scale;
        } else {
          k = -1; frame = 0;
        }
      }
    }
    s_box[e] = box; s_score[e] = score; s_frame[e] = frame; s_track[e] = k; s_src[e] = src;
  }
  __syncthreads();

  const long long s = t0 + tid;
  if (s >= S) return;
  const int e = tid + r;
  const int k = s_track[e], frame = s_frame[e];
  float4 box = s_box[e];
  if (r > 0 && k >= 0) {
    double ax = 0.0, ay = 0.0, az = 0.0, aw = 0.0;
    int cnt = 0;
    for (int d = -r; d <= r; ++d) {                       // ascending slot = ascending frame
      const int e2 = e + d;
      const int df = s_frame[e2] - frame;
      if (s_track[e2] != k || df < -r || df > r) continue;
      const float4 b = s_box[e2];
      if (cnt == 0) {                                     // the sum starts from its first term: one box keeps a -0.0
        ax = (double)b.x; ay = (double)b.y; az = (double)b.z; aw = (double)b.w;
      } else {
        ax += (double)b.x; ay += (double)b.y; az += (double)b.z; aw += (double)b.w;
      }
      ++cnt;
    }
    const double c = (double)cnt;                         // >= 1: the slot itself
    box = make_float4((float)(ax / c), (float)(ay / c), (float)(az / c), (float)(aw / c));
  }
  out_box[s] = box;
  out_score[s] = s_score[e];
  out_frame[s] = frame;
  out_track[s] = k;
  out_src[s] = s_src[e];
  out_filled[s] = (unsigned char)(k >= 0 && s_src[e] < 0);
}

}  // namespace

// The fused form keeps the unsmoothed slots of a tile in LDS: no workspace.
extern "C" size_t mega_refine_tracks_workspace_bytes(long long S, int r) {
  (void)S; (void)r;
  return 0;
}

extern "C" int mega_refine_tracks(const float* m_box, const float* m_score, const int* m_frame, const long long* m_off,
                                  const long long* o_off, int K, long long M, long long S, int fill, int r, float fill_scale,
                                  float* out_box, float* out_score, int* out_frame, int* out_track, int* out_src,
                                  unsigned char* out_filled, void* ws, size_t ws_bytes, void* stream) {
  mega_clear_error();
  if (K < 0 || M < 0 || S < 0 || M > 0x7fffffffLL || S > 0x7fffffffLL || r < 0 || r > RT_MAX_R) return MEGA_ERR_ARG;
  if ((fill != 0 && fill != 1) || !(fill_scale > 0.0f && fill_scale <= 1.0f)) return MEGA_ERR_ARG;
  if (M > 0 && (!m_box || !m_score || !m_frame)) return MEGA_ERR_ARG;
  if (K > 0 && (!m_off || !o_off)) return MEGA_ERR_ARG;
  if (S > 0 && (!out_box || !out_score || !out_frame || !out_track || !out_src || !out_filled || K == 0 || M == 0))
    return MEGA_ERR_ARG;
  const size_t need = mega_refine_tracks_workspace_bytes(S, r);
  if (need > 0 && !ws) return MEGA_ERR_ARG;
  if (ws_bytes < need) return MEGA_ERR_WS;
  if (S == 0) return MEGA_OK;                             // no slot: nothing to launch
  hipLaunchKernelGGL(refine_tracks_kernel, dim3((unsigned)((S + RT_THREADS - 1) / RT_THREADS)), dim3(RT_THREADS), 0,
                     (hipStream_t)stream, (const float4*)m_box, m_score, m_frame, m_off, o_off, K, M, S, fill, r, fill_scale,
                     (float4*)out_box, out_score, out_frame, out_track, out_src, out_filled);
  return mega_check_launch();
}
