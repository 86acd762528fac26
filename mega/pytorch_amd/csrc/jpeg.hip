// Device half of the JPEG decode (mega/pytorch_amd/jpeg.py defines it; tests/jpeg_twin.py is its numpy twin): the raw DCT
// coefficients that jpeg_entropy.h decoded on the host become the [N][H][W][3] uint8 RGB frames Pillow would have produced,
// bit for bit.  Integer arithmetic only (no floating point anywhere, so no contraction flag).
//
// Launch 1, jpeg_idct_kernel, one thread per 8x8 block: 64 int16 coefficients (8 x 16-byte loads) times the component's
//   table, libjpeg's accurate integer IDCT (jidctint.c: CONST_BITS 13, PASS1_BITS 2; columns descaled by 11, rows by 18,
//   round half up) with both passes in registers, + 128, clamp, 8 stores of 8 bytes into the component's plane.  Lanes run
//   along a block row, so a wave's stores to one plane row are contiguous.  Products and sums wrap in 32 bits (computed
//   unsigned): for dequantised coefficients within int16 nothing wraps and the result is the library's; outside that range
//   the final clamp saturates where the library's range table would wrap.
// Launch 2, jpeg_rgb_kernel, one thread per 4 pixels of an output row: libjpeg's "fancy" (triangle) chroma upsampling --
//   h2v1: (3 s + left + 1) >> 2 and (3 s + right + 2) >> 2, copies at both ends; h2v2: column sums c = 3 near + far,
//   (3 c + c_left + 8) >> 4 and (3 c + c_right + 7) >> 4, (4 c + 8) >> 4 and (4 c + 7) >> 4 at the ends, the row beyond
//   the first / last chroma row being that row itself; a chroma plane of 1 or 2 columns is replicated instead, as the
//   library does -- then YCbCr -> RGB in 16-bit fixed point, clamped.  12 bytes go out as 3 dwords when W % 4 == 0 (every
//   row then starts on a dword), else byte by byte.  Neighbours are taken within the component's own size
//   ceil(W / 2) x ceil(H / 2): the MCU padding of a plane is never read as a neighbour.
#include "launch.h"
#include "workspace.h"
#include "jpeg_entropy.h"

namespace {

constexpr int JP_THREADS = 256;

struct JpGeom {
  int bw[3], bh[3];             // blocks per row / column of each component (MCU-padded)
  int boff[4];                  // first block of each component within a frame, [3] = blocks per frame
};

inline bool jp_geom(int W, int H, int sampling, JpGeom& g) {
  if (!mega_jpeg::geometry(W, H, sampling, g.bw, g.bh)) return false;
  g.boff[0] = 0;
  for (int c = 0; c < 3; ++c) g.boff[c + 1] = g.boff[c] + g.bw[c] * g.bh[c];
  return true;
}

#define JP_MUL(a, k) ((a) * (unsigned)(k))
__device__ __forceinline__ unsigned jp_descale(unsigned x, int n) { return (unsigned)((int)(x + (1u << (n - 1))) >> n); }

// one 1-D pass of jidctint.c on 8 values, results NOT yet descaled (unsigned = wrapping int32)
__device__ __forceinline__ void jp_idct8(const unsigned in[8], unsigned out[8]) {
  unsigned z2 = in[2], z3 = in[6];
  unsigned z1 = JP_MUL(z2 + z3, 4433);
  unsigned tmp2 = z1 + JP_MUL(z3, -15137);
  unsigned tmp3 = z1 + JP_MUL(z2, 6270);
  unsigned tmp0 = (in[0] + in[4]) << 13;
  unsigned tmp1 = (in[0] - in[4]) << 13;
  const unsigned tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7];
  tmp1 = in[5];
  tmp2 = in[3];
  tmp3 = in[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  unsigned z4 = tmp1 + tmp3;
  const unsigned z5 = JP_MUL(z3 + z4, 9633);
  tmp0 = JP_MUL(tmp0, 2446);
  tmp1 = JP_MUL(tmp1, 16819);
  tmp2 = JP_MUL(tmp2, 25172);
  tmp3 = JP_MUL(tmp3, 12299);
  z1 = JP_MUL(z1, -7373);
  z2 = JP_MUL(z2, -20995);
  z3 = JP_MUL(z3, -16069) + z5;
  z4 = JP_MUL(z4, -3196) + z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  out[0] = tmp10 + tmp3;
  out[7] = tmp10 - tmp3;
  out[1] = tmp11 + tmp2;
  out[6] = tmp11 - tmp2;
  out[2] = tmp12 + tmp1;
  out[5] = tmp12 - tmp1;
  out[3] = tmp13 + tmp0;
  out[4] = tmp13 - tmp0;
}

__device__ __forceinline__ unsigned jp_clamp255(int v) { return (unsigned)min(max(v, 0), 255); }

__global__ __launch_bounds__(JP_THREADS) void jpeg_idct_kernel(const short* __restrict__ coef, long long stride,
                                                               unsigned char* __restrict__ planes, JpGeom g) {
  const int t = blockIdx.x * JP_THREADS + threadIdx.x;
  if (t >= g.boff[3]) return;
  const int c = t >= g.boff[2] ? 2 : (t >= g.boff[1] ? 1 : 0);
  const int b = t - g.boff[c];
  const int by = b / g.bw[c], bx = b - by * g.bw[c];
  const short* frame = coef + (size_t)blockIdx.y * (size_t)stride;
  const short* __restrict__ qt = frame + 64 * c;
  const uint4* __restrict__ src = (const uint4*)(frame + mega_jpeg::QT_ELEMS + 64 * (size_t)t);
  const uint4* __restrict__ q4 = (const uint4*)qt;
  unsigned ws[8][8];
  // dequantise; columns first: ws[r][col]
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint4 v = src[r], q = q4[r];
    const unsigned vw[4] = {v.x, v.y, v.z, v.w}, qw[4] = {q.x, q.y, q.z, q.w};
    for (int k = 0; k < 4; ++k) {
      ws[r][2 * k] = (unsigned)((int)(short)(vw[k] & 0xffffu) * (int)(short)(qw[k] & 0xffffu));
      ws[r][2 * k + 1] = (unsigned)((int)(short)(vw[k] >> 16) * (int)(short)(qw[k] >> 16));
    }
  }
#pragma unroll
  for (int col = 0; col < 8; ++col) {
    unsigned in[8], out[8];
    for (int r = 0; r < 8; ++r) in[r] = ws[r][col];
    jp_idct8(in, out);
    for (int r = 0; r < 8; ++r) ws[r][col] = jp_descale(out[r], 11);
  }
  const int pitch = g.bw[c] * 8;
  unsigned char* plane = planes + (size_t)blockIdx.y * ((size_t)g.boff[3] * 64) + (size_t)g.boff[c] * 64;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    unsigned out[8];
    jp_idct8(ws[r], out);
    unsigned px[8];
    for (int k = 0; k < 8; ++k) px[k] = jp_clamp255((int)jp_descale(out[k], 18) + 128);
    uint2 w;
    w.x = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    w.y = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
    *(uint2*)(plane + (size_t)(by * 8 + r) * pitch + bx * 8) = w;
  }
}

// the 4 upsampled samples of one chroma plane at output columns x0 .. x0 + 3 of output row y
__device__ __forceinline__ void jp_chroma4(const unsigned char* __restrict__ p, int pitch, int cw, int chh, int hs, int vs,
                                           int x0, int y, int v[4]) {
  if (hs == 1) {      // 4:4:4
    const unsigned char* row = p + (size_t)y * pitch;
    for (int k = 0; k < 4; ++k) v[k] = row[x0 + k];      // (columns beyond W lie in the plane's padding: in bounds, unused)
    return;
  }
  const int cy = vs == 2 ? (y >> 1) : y;
  const int cx = x0 >> 1;
  const unsigned char* near = p + (size_t)cy * pitch;
  if (cw <= 2) {      // the library replicates planes this narrow
    const int a = near[cx], b = near[min(cx + 1, cw - 1)];
    v[0] = v[1] = a;
    v[2] = v[3] = b;
    return;
  }
  int s[4];      // columns cx - 1 .. cx + 2, indices clamped into the plane (a clamped one is never used as a neighbour)
  if (vs == 2) {
    const int fy = (y & 1) ? min(cy + 1, chh - 1) : max(cy - 1, 0);
    const unsigned char* far = p + (size_t)fy * pitch;
    for (int k = 0; k < 4; ++k) {
      const int xc = min(max(cx - 1 + k, 0), cw - 1);
      s[k] = 3 * near[xc] + far[xc];
    }
    v[0] = cx == 0 ? (4 * s[1] + 8) >> 4 : (3 * s[1] + s[0] + 8) >> 4;
    v[1] = cx == cw - 1 ? (4 * s[1] + 7) >> 4 : (3 * s[1] + s[2] + 7) >> 4;
    v[2] = (3 * s[2] + s[1] + 8) >> 4;
    v[3] = cx + 1 >= cw - 1 ? (4 * s[2] + 7) >> 4 : (3 * s[2] + s[3] + 7) >> 4;
  } else {
    for (int k = 0; k < 4; ++k) s[k] = near[min(max(cx - 1 + k, 0), cw - 1)];
    v[0] = cx == 0 ? s[1] : (3 * s[1] + s[0] + 1) >> 2;
    v[1] = cx == cw - 1 ? s[1] : (3 * s[1] + s[2] + 2) >> 2;
    v[2] = (3 * s[2] + s[1] + 1) >> 2;
    v[3] = cx + 1 >= cw - 1 ? s[2] : (3 * s[2] + s[3] + 2) >> 2;
  }
}

__global__ __launch_bounds__(JP_THREADS) void jpeg_rgb_kernel(const unsigned char* __restrict__ planes,
                                                              unsigned char* __restrict__ rgb, int H, int W, int sampling,
                                                              JpGeom g) {
  const int x0 = (blockIdx.x * JP_THREADS + threadIdx.x) * 4;
  const int y = blockIdx.y, n = blockIdx.z;
  if (x0 >= W) return;
  const unsigned char* fp = planes + (size_t)n * ((size_t)g.boff[3] * 64);
  const unsigned yw = *(const unsigned*)(fp + (size_t)y * (g.bw[0] * 8) + x0);      // pitch % 8 == 0, x0 % 4 == 0
  unsigned char o[12];
  if (sampling == mega_jpeg::SAMP_GRAY) {
    for (int k = 0; k < 4; ++k) o[3 * k] = o[3 * k + 1] = o[3 * k + 2] = (unsigned char)((yw >> (8 * k)) & 255u);
  } else {
    const int hs = sampling >= mega_jpeg::SAMP_422 ? 2 : 1, vs = sampling == mega_jpeg::SAMP_420 ? 2 : 1;
    const int cw = (W + hs - 1) / hs, chh = (H + vs - 1) / vs;
    const int pitch = g.bw[1] * 8;
    int cb[4], cr[4];
    jp_chroma4(fp + (size_t)g.boff[1] * 64, pitch, cw, chh, hs, vs, x0, y, cb);
    jp_chroma4(fp + (size_t)g.boff[2] * 64, pitch, cw, chh, hs, vs, x0, y, cr);
    for (int k = 0; k < 4; ++k) {
      const int yy = (int)((yw >> (8 * k)) & 255u), b = cb[k] - 128, r = cr[k] - 128;
      o[3 * k] = (unsigned char)jp_clamp255(yy + ((91881 * r + 32768) >> 16));
      o[3 * k + 1] = (unsigned char)jp_clamp255(yy + ((-22554 * b - 46802 * r + 32768) >> 16));
      o[3 * k + 2] = (unsigned char)jp_clamp255(yy + ((116130 * b + 32768) >> 16));
    }
  }
  unsigned char* dst = rgb + (((size_t)n * H + y) * W + x0) * 3;
  if ((W & 3) == 0) {
    unsigned* d4 = (unsigned*)dst;
    for (int k = 0; k < 3; ++k)
      d4[k] = (unsigned)o[4 * k] | ((unsigned)o[4 * k + 1] << 8) | ((unsigned)o[4 * k + 2] << 16) | ((unsigned)o[4 * k + 3] << 24);
  } else {
    const int cnt = min(4, W - x0) * 3;
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < cnt) dst[k] = o[k];
  }
}

struct JpWs {
  unsigned char* planes;
  size_t bytes;
  JpWs(void* ws, int N, const JpGeom& g) {
    WsCarver c(ws);
    planes = c.take<unsigned char>((size_t)N * g.boff[3] * 64);      // per frame: the Y, Cb, Cr planes over the padded grids
    bytes = c.bytes;
  }
};

}  // namespace

extern "C" int mega_jpeg_probe(const unsigned char* data, long long nbytes, int* info) {
  return mega_jpeg::probe(data, nbytes, info) == mega_jpeg::JPG_OK ? MEGA_OK : MEGA_ERR_ARG;
}

extern "C" int mega_jpeg_entropy_decode(const unsigned char* data, long long nbytes, const int* info, short* out,
                                        long long out_elems) {
  return mega_jpeg::entropy_decode(data, nbytes, info, out, out_elems) == mega_jpeg::JPG_OK ? MEGA_OK : MEGA_ERR_ARG;
}

extern "C" size_t mega_jpeg_reconstruct_workspace_bytes(int N, int H, int W, int sampling) {
  JpGeom g;
  if (N <= 0 || N > 65535 || !jp_geom(W, H, sampling, g)) return 0;      // (N is a grid dimension)
  return JpWs(nullptr, N, g).bytes;
}

extern "C" int mega_jpeg_reconstruct(const short* coef, long long stride, int N, int H, int W, int sampling,
                                     unsigned char* rgb, void* ws, size_t ws_bytes, void* stream) {
  mega_clear_error();
  JpGeom g;
  if (N <= 0 || N > 65535 || !jp_geom(W, H, sampling, g)) return MEGA_ERR_ARG;
  // frames start on 16-byte boundaries: the block loads are 16-byte vectors
  if (stride < mega_jpeg::QT_ELEMS + 64ll * g.boff[3] || (stride & 7) != 0) return MEGA_ERR_ARG;
  // rgb: the dword stores are taken when W % 4 == 0 (a frame is then a multiple of 4 bytes); any other width stores bytes
  if (!coef || !rgb || !ws || ((uintptr_t)coef & 15) != 0 || ((uintptr_t)ws & 7) != 0) return MEGA_ERR_ARG;
  if ((W & 3) == 0 && ((uintptr_t)rgb & 3) != 0) return MEGA_ERR_ARG;
  const JpWs w(ws, N, g);
  if (ws_bytes < w.bytes) return MEGA_ERR_WS;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3(cdiv(g.boff[3], JP_THREADS), N), dim3(JP_THREADS), 0, st, coef, stride, w.planes, g);
  hipLaunchKernelGGL(jpeg_rgb_kernel, dim3(cdiv(cdiv(W, 4), JP_THREADS), H, N), dim3(JP_THREADS), 0, st,
                     (const unsigned char*)w.planes, rgb, H, W, sampling, g);
  return mega_check_launch();
}
