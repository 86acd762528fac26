// Launch parameters shared by the implicit-GEMM kernels (igemm.hip: register-staged 2-barrier tiles;
// igemm8.hip: LDS-DMA 8-phase 256-wide tiles).
#pragma once
#include <hip/hip_runtime.h>

struct ConvParams {
  const void* in;
  const void* w;
  const float* scale;
  const float* bias;
  const void* res;
  void* out;
  int N, H, W, Cin, Cout, R, S, stride, pad, dil, Ho, Wo;
  int M, K;
  int ldo, ldr;
  int relu;          // 0 none, 1 ReLU, 2 LeakyReLU(0.1)
  unsigned in_bytes, w_bytes;
  int ksplit;        // > 1: blockIdx.z owns a contiguous range of K-tiles and writes raw f32 partial sums
  float* partial;    // [ksplit][M][Cout] f32 when ksplit > 1
  // ---- Split-precision ("hi | lo planes") activations, sp != 0 (mega_conv2d_nhwc_sp_dt; read by igemm8.hip's SP kernels only): an
  //      f32 activation x [M][C] is stored as 16-bit planes [M][2C] = [hi | lo], hi = bf16(x), lo = bf16(x - hi)  (x = hi + lo to
  //      ~2^-17; IEEE-half pairs with dtype MEGA_F16)
  int sp;            // 1: the fields below apply; 0: plain tensors (every other entry point)
  int ldi;           // pixel stride of `in` in elements (2C for a split input; Cin when the input is a plain tensor)
  int kwrap;         // contraction channel at which the SOURCE channel index wraps to 0 (0: never).  Cin = 3C, kwrap = 2C
                     // reads the planes as [hi | lo | hi]: against weights packed [Wh | Wh | Wl] per tap the K = 3C
                     // contraction is x_hi.Wh + x_lo.Wh + x_hi.Wl = x.W to ~2^-16 on the bf16 matrix cores
  int split_out;     // 1: out is split planes [M][ldo] with hi at column n and lo at column Cout + n (16-bit output only)
                     // (a residual given to an SP launch is ALWAYS split planes: res[m][n] + res[m][Cout + n])
  unsigned mg_howo, sh_howo, mg_wo, sh_wo;   // igemm8 only: magic multipliers / shifts for m / (Ho Wo) and rem / Wo (set by its launcher)
  // ---- Two launch forms that exclude each other share the three words of the unions below, so that the kernels' argument block
  //      keeps one layout:
  //      ps == 1, sub-pixel output (mega_conv2d_nhwc_subpixel; read by igemm.hip's PS kernels and its split-K finalize, and by
  //      igemm8.hip's sub-pixel epilogue): a ConvTranspose2d(k = 4, s = 2) run as a 2 x 2 / pad 1 conv with 4 ps_C output columns
  //      n = (a, b, co): GEMM row m = (t, mh, mw) lands at pixel (2 mh + a - ps_crop, 2 mw + b - ps_crop), channel ps_coff + co of
  //      an NHWC tensor [N][ps_H][ps_W][ldo]; pixels outside it are dropped.
  //      ps == 0 with a residual and rs_stride > 1, residual read at a pixel stride (mega_conv2d_nhwc_rs, a 1x1 / stride 1 conv;
  //      read by igemm8.hip's strided-residual epilogue only): GEMM row m = (t, y, x) adds pixel (s y, s x), s = rs_stride, of an
  //      NHWC tensor [N][rs_H][rs_W][ldr] -- res[:, ::s, ::s, :] read in place.  rs_stride <= 1: res is [M][ldr].
  int ps;
  union { int ps_H, rs_H; };
  union { int ps_W, rs_W; };
  union { int ps_C, rs_stride; };
  int ps_crop, ps_coff;
};

// the launch reads its residual at a pixel stride
inline bool conv_res_strided(const ConvParams& p) { return !p.ps && p.res && p.rs_stride > 1; }

// igemm8.hip: 16-bit operands, 8 waves, bm (256 or 192 rows) x 256 tile; returns MEGA_OK / MEGA_ERR_*.  out_f32: 0 16-bit, 1 f32.
// half_dtype: MEGA_BF16 / MEGA_F16 = the 16-bit type of in / w / residual (and of the output when out_f32 == 0)
int mega_igemm8_launch(const ConvParams& p, int bm, int out_f32, int half_dtype, hipStream_t st);
// 1 when the shape is one igemm8 can take (Cin % 64 == 0, operands < 2 GiB, ...)
int mega_igemm8_supports(const ConvParams& p);
// 1 when a launch of `taps` = R * S kernel taps and GEMM depth K belongs to igemm8's streaming class (1x1, K <= 512)
int mega_igemm8_streaming(int taps, int K);
// 1 when a plain or split-precision launch runs igemm8's streaming (CLS 1) instantiation, 0 the matrix (CLS 0) one: what
// launch8_mode instantiates and what the plan entry points report
int mega_igemm8_class(int taps, int K, int ksplit);
// conv64.hip: persistent 3x3 / 64 -> 64 channel kernel (layer1's conv2); bit-identical to the generic tiles
int mega_conv64_supports(const ConvParams& p, int out_f32);
int mega_conv64_launch(const ConvParams& p, int half_dtype, hipStream_t st);
