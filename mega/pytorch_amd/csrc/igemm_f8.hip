// Implicit-GEMM NHWC convolution on FP8 operands (OCP e4m3fn, bias 7, largest finite value 448, no infinities), f32
// accumulation: the opt-in FP8 path of layer3's conv1 (1x1, bf16 trunk in -> fp8 out) and conv2 (3x3, fp8 in -> bf16 out);
// mega/pytorch_amd/f8.py defines the quantisation.  Both operands go through the block-scaled MFMA
// v_mfma_scale_f32_32x32x64_f8f6f4 (cbsz = blgp = 0: e4m3 on both sides) with unit block scales (E8M0 code 127), which runs
// at twice the bf16 rate per clock; the non-scaled fp8 MFMAs run at the bf16 rate.
//
// Contraction, layouts and epilogue are those of igemm.hip: activations NHWC, weights OHWI, K order (r, s, c),
//   y = act(acc * scale[c] + bias[c]),   acc = the f32 sum of code products
// with the three factors s_in * sw[c] * bn_scale[c] folded into scale[c] by the host.  There is no residual operand.
//
// Input forms.   MEGA_F8: the producer's codes, copied to LDS as they are.   MEGA_BF16: converted on the load path --
//   registers, widen to f32, * in_inv_scale, clamp to +-448, v_cvt_pk_fp8_f32 (round to nearest even), into LDS as fp8: the
//   bf16 trunk is read once and no fp8 copy of it ever exists in HBM.
// Output forms.  MEGA_BF16: one rounding of y.   MEGA_F8: quantize(y, out_inv_scale) = clamp(y * out_inv_scale, +-448)
//   converted to e4m3 (the clamp comes BEFORE the conversion: nothing depends on what the instruction does above 448).
// A padding tap is the code 0x00 = +0.
//
// Geometry.  256 threads = 4 waves, block tile 128 rows x BN columns, K step 128 codes (Cin % 128 == 0, so a K step never
//   crosses a tap).  BN = 256 (Cout % 256 == 0: waves 2 x 2, each 64 rows x 128 columns = 2 x 4 fragments of 32 x 32) or
//   BN = 64 (waves 4 x 1, each 32 rows x 64 columns).  LDS holds two stages of [A: 128 rows][B: BN rows] x 128 bytes; a row's
//   eight 16-byte chunks are XOR-swizzled by the row (physical chunk = chunk ^ (row & 7)).  The next K step's global loads are
//   issued before the current step's MFMAs and written to the other stage after them: one barrier per K step.
// Fragments.  Lane l of either operand holds row (l & 31) and the 32 consecutive codes [32 (l >> 5), 32 (l >> 5) + 32) of a
//   64-deep K slice -- one block-scale group per lane, which is why the group of a lane must be contiguous.  Both operands are
//   read with the SAME map, and the weight is the first operand, so the 32 x 32 result is indexed [n][m] as in igemm8: a lane
//   owns output row m = l & 31 and, for g = 0..3, the four consecutive channels 8 g + 4 (l >> 5) + (0..3).
#include "launch.h"

namespace {

constexpr int NTF = 256;               // threads per block
constexpr int BMF = 128;               // rows per block tile
constexpr int KSTEP = 128;             // codes per K step = bytes per LDS row
constexpr int UNIT = 0x7f7f7f7f;       // E8M0 127 = 2^0 in every byte, whichever byte the op-sel picks

typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2f_t __attribute__((ext_vector_type(2)));

struct F8Params {
  const void* in; const void* w; const float* scale; const float* bias; void* out;
  float in_inv, out_inv;
  int N, H, W, Cin, Cout, R, S, pad, M, relu;
};

__device__ __forceinline__ float clamp448(float v) { return fminf(fmaxf(v, -448.f), 448.f); }

// four floats -> four e4m3 codes in one dword (element 0 in the low byte), round to nearest even
__device__ __forceinline__ unsigned pack_f8x4(float a, float b, float c, float d) {
  int r = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  r = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, r, true);
  return (unsigned)r;
}

// eight bf16 (one 16-byte vector) -> eight codes: quantize(v, inv) of f8.py
__device__ __forceinline__ u32x2f_t quant_bf16x8(const u32x4_t& v, float inv) {
  float f[8];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    f[2 * d] = clamp448(__uint_as_float(v[d] << 16) * inv);
    f[2 * d + 1] = clamp448(__uint_as_float(v[d] & 0xffff0000u) * inv);
  }
  return u32x2f_t{pack_f8x4(f[0], f[1], f[2], f[3]), pack_f8x4(f[4], f[5], f[6], f[7])};
}

// IN_BF16: the input is bf16 (else fp8 codes); OUT_F8: the output is fp8 codes (else bf16)
template <int BN, bool IN_BF16, bool OUT_F8>
__global__ __launch_bounds__(NTF) void igemm_f8_kernel(F8Params p) {
  constexpr int WC = BN == 256 ? 2 : 1;        // wave columns
  constexpr int WR = 4 / WC;                   // wave rows
  constexpr int MF = BMF / (32 * WR);          // 32-row fragments per wave
  constexpr int NF = BN / (32 * WC);           // 32-column fragments per wave
  constexpr int A_BYTES = BMF * KSTEP, B_BYTES = BN * KSTEP, STAGE = A_BYTES + B_BYTES;
  constexpr int NB = BN * 8 / NTF;             // 16-byte weight chunks per thread per K step
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave / WC, wc = wave % WC;
  const int ntn = p.Cout / BN;
  const int tile_m = blockIdx.x / ntn, tile_n = blockIdx.x - tile_m * ntn;
  const int m0 = tile_m * BMF, n0 = tile_n * BN;

  // ---- staging: thread (srow, sch) moves chunk sch of rows srow + 32 u.  One chunk is 16 codes: 16 bytes of an fp8
  //      input, two 16-byte vectors of a bf16 input.
  const int srow = tid >> 3, sch = tid & 7;
  int a_ho[4], a_wo[4];
  size_t a_pix[4];                              // pixel index of (image, ho, wo); rows past M never pass the range test
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int m = m0 + srow + 32 * u;
    const bool ok = m < p.M;
    const int mm = ok ? m : 0;
    const int img = mm / (p.H * p.W), rem = mm - img * (p.H * p.W);
    const int ho = rem / p.W;
    a_ho[u] = ok ? ho : -(1 << 20);
    a_wo[u] = rem - ho * p.W;
    a_pix[u] = (size_t)mm;
  }
  const int cin_steps = p.Cin / KSTEP;
  const int nk = p.R * p.S * cin_steps;
  const size_t K = (size_t)p.R * p.S * p.Cin;

  u32x4_t ra[4][IN_BF16 ? 2 : 1], rb[NB];
  auto gload = [&](int kt) {
    const int tap = kt / cin_steps, kc = (kt - tap * cin_steps) * KSTEP;
    const int r = tap / p.S, s = tap - r * p.S;
    const int dh = r - p.pad, dw = s - p.pad;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int hi = a_ho[u] + dh, wi = a_wo[u] + dw;
      const bool ok = ((unsigned)hi < (unsigned)p.H) & ((unsigned)wi < (unsigned)p.W);
      // (stride 1, dil 1: the tap's pixel is the row's own pixel moved by (dh, dw) inside the same image)
      const size_t e = (size_t)((long long)a_pix[u] + (long long)dh * p.W + dw) * p.Cin + kc + sch * 16;
      if (IN_BF16) {
        const u32x4_t* src = reinterpret_cast<const u32x4_t*>(static_cast<const bf16_t*>(p.in) + (ok ? e : 0));
        ra[u][0] = ok ? src[0] : u32x4_t{0, 0, 0, 0};
        ra[u][IN_BF16 ? 1 : 0] = ok ? src[1] : u32x4_t{0, 0, 0, 0};
      } else {
        const u32x4_t* src = reinterpret_cast<const u32x4_t*>(static_cast<const unsigned char*>(p.in) + (ok ? e : 0));
        ra[u][0] = ok ? src[0] : u32x4_t{0, 0, 0, 0};
      }
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int n = n0 + srow + 32 * u;            // < Cout: BN divides Cout
      rb[u] = *reinterpret_cast<const u32x4_t*>(static_cast<const unsigned char*>(p.w) + (size_t)n * K + (size_t)kt * KSTEP + sch * 16);
    }
  };
  auto lstore = [&](int buf) {
    unsigned char* sa = smem + buf * STAGE;
    unsigned char* sb = sa + A_BYTES;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = srow + 32 * u;
      u32x4_t v;
      if (IN_BF16) {
        const u32x2f_t lo = quant_bf16x8(ra[u][0], p.in_inv), hi = quant_bf16x8(ra[u][IN_BF16 ? 1 : 0], p.in_inv);
        v = u32x4_t{lo[0], lo[1], hi[0], hi[1]};
      } else {
        v = ra[u][0];
      }
      *reinterpret_cast<u32x4_t*>(sa + row * KSTEP + ((sch ^ (row & 7)) << 4)) = v;
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int row = srow + 32 * u;
      *reinterpret_cast<u32x4_t*>(sb + row * KSTEP + ((sch ^ (row & 7)) << 4)) = rb[u];
    }
  };

  f32x16_t acc[MF][NF];
#pragma unroll
  for (int i = 0; i < MF; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragment of 32 rows starting at row0 of an operand slab, K slice h (64 codes): two 16-byte chunks per lane
  const int l31 = lane & 31, lh = lane >> 5;
  auto frag = [&](const unsigned char* slab, int row0, int h) -> i32x8_t {
    const int row = row0 + l31;
    const int c0 = h * 4 + lh * 2;
    const u32x4_t q0 = *reinterpret_cast<const u32x4_t*>(slab + row * KSTEP + (((c0) ^ (row & 7)) << 4));
    const u32x4_t q1 = *reinterpret_cast<const u32x4_t*>(slab + row * KSTEP + (((c0 + 1) ^ (row & 7)) << 4));
    return i32x8_t{(int)q0[0], (int)q0[1], (int)q0[2], (int)q0[3], (int)q1[0], (int)q1[1], (int)q1[2], (int)q1[3]};
  };

  gload(0);
  lstore(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    gload(kt + 1 < nk ? kt + 1 : kt);            // (the last step loads itself again: a loop body without branches)
    const unsigned char* sa = smem + buf * STAGE;
    const unsigned char* sb = sa + A_BYTES;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      i32x8_t af[MF], bf[NF];
#pragma unroll
      for (int i = 0; i < MF; ++i) af[i] = frag(sa, (wr * MF + i) * 32, h);
#pragma unroll
      for (int j = 0; j < NF; ++j) bf[j] = frag(sb, (wc * NF + j) * 32, h);
#pragma unroll
      for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(bf[j], af[i], acc[i][j], 0, 0, 0, UNIT, 0, UNIT);
    }
    // (one basic block and this fence: otherwise hipcc sinks the MFMAs below the stage's LDS writes -- and with them below
    //  the wait for the global loads just issued -- so that the loads' latency is exposed in every K step instead of running
    //  under 16 MFMAs.  The last step's store goes to the stage nobody reads any more.)
    __builtin_amdgcn_sched_barrier(0);
    lstore(buf ^ 1);                             // the other stage: its last readers passed the previous barrier
    __syncthreads();
  }

  // ---- epilogue, from the accumulator registers: row m = lane & 31 of the fragment, channels 8 g + 4 (lane >> 5) + (0..3)
#pragma unroll
  for (int j = 0; j < NF; ++j) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = n0 + (wc * NF + j) * 32 + 8 * g + 4 * lh;
      f32x4_t sc = {1.f, 1.f, 1.f, 1.f}, bi = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (p.scale) sc[t] = p.scale[n + t];
        if (p.bias) bi[t] = p.bias[n + t];
      }
#pragma unroll
      for (int i = 0; i < MF; ++i) {
        const int m = m0 + (wr * MF + i) * 32 + l31;
        float v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          v[t] = fmaf(acc[i][j][4 * g + t], sc[t], bi[t]);
          if (p.relu) v[t] = fmaxf(v[t], 0.f);
        }
        if (m >= p.M) continue;
        if (OUT_F8) {
          const unsigned o = pack_f8x4(clamp448(v[0] * p.out_inv), clamp448(v[1] * p.out_inv), clamp448(v[2] * p.out_inv),
                                       clamp448(v[3] * p.out_inv));
          *reinterpret_cast<unsigned*>(static_cast<unsigned char*>(p.out) + (size_t)m * p.Cout + n) = o;
        } else {
          const u32x2f_t o = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
          *reinterpret_cast<u32x2f_t*>(static_cast<bf16_t*>(p.out) + (size_t)m * p.Cout + n) = o;
        }
      }
    }
  }
}

// The tile class of an admitted layer (the BN of its kernel), or -1: 1x1 / pad 0 or 3x3 / pad 1, stride 1, dil 1,
// Cin % 128 == 0, Cout % 64 == 0, bf16 or fp8 on either side, at least one row, and a row count that keeps the grid and every
// 32-bit row index in range.
int plan_f8(long long N, long long H, long long W, int Cin, int Cout, int R, int S, int stride, int pad, int dil, int in_dtype,
            int out_dtype) {
  if (N < 1 || H < 1 || W < 1 || Cin < 128 || Cout < 64 || Cin % 128 != 0 || Cout % 64 != 0) return -1;
  if (!((R == 1 && S == 1 && pad == 0) || (R == 3 && S == 3 && pad == 1)) || stride != 1 || dil != 1) return -1;
  if ((in_dtype != MEGA_BF16 && in_dtype != MEGA_F8) || (out_dtype != MEGA_BF16 && out_dtype != MEGA_F8)) return -1;
  if (H > (1 << 20) || W > (1 << 20) || N * H * W > 0x3FFFFFFFll) return -1;
  const int bn = Cout % 256 == 0 ? 256 : 64;
  if (((N * H * W + BMF - 1) / BMF) * (Cout / bn) > 0x7FFFFFFFll) return -1;
  return bn;
}

template <int BN, bool IN_BF16, bool OUT_F8>
int launch_f8(const F8Params& p, hipStream_t st) {
  const unsigned grid = (unsigned)cdiv(p.M, BMF) * (unsigned)(p.Cout / BN);
  return launch_lds(igemm_f8_kernel<BN, IN_BF16, OUT_F8>, dim3(grid), dim3(NTF), (size_t)2 * (BMF + BN) * KSTEP, st, p);
}

template <int BN>
int launch_f8_io(const F8Params& p, int in_dtype, int out_dtype, hipStream_t st) {
  if (in_dtype == MEGA_BF16) return out_dtype == MEGA_F8 ? launch_f8<BN, true, true>(p, st) : launch_f8<BN, true, false>(p, st);
  return out_dtype == MEGA_F8 ? launch_f8<BN, false, true>(p, st) : launch_f8<BN, false, false>(p, st);
}

}  // namespace

extern "C" int mega_conv2d_nhwc_f8_plan(int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int dil,
                                        int in_dtype, int out_dtype) {
  return plan_f8(N, H, W, Cin, Cout, R, S, stride, pad, dil, in_dtype, out_dtype);
}

extern "C" int mega_conv2d_nhwc_f8(const void* in, int in_dtype, float in_inv_scale, const void* w_f8, const float* scale,
                                   const float* bias, void* out, int out_dtype, float out_inv_scale, int N, int H, int W, int Cin,
                                   int Cout, int R, int S, int stride, int pad, int dil, int relu, void* stream) {
  const int bn = plan_f8(N, H, W, Cin, Cout, R, S, stride, pad, dil, in_dtype, out_dtype);
  if (bn < 0 || !in || !w_f8 || !out || (relu != 0 && relu != 1)) return MEGA_ERR_ARG;
  mega_clear_error();
  F8Params p;
  p.in = in; p.w = w_f8; p.scale = scale; p.bias = bias; p.out = out;
  p.in_inv = in_inv_scale; p.out_inv = out_inv_scale;
  p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.R = R; p.S = S; p.pad = pad; p.M = N * H * W; p.relu = relu;
  hipStream_t st = (hipStream_t)stream;
  return bn == 256 ? launch_f8_io<256>(p, in_dtype, out_dtype, st) : launch_f8_io<64>(p, in_dtype, out_dtype, st);
}
