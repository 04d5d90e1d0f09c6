// Tiled VAE (comfy/utils.py:448-475 tiled_scale; comfy/sd.py:302-327 decode_tiled_ / encode_tiled_): the tile cut, the feathered
// blend, the three-pass average, and a row softmax with a valid-column count for padded score matrices: bandwidth-bound helpers
// around the launch plans of libsr_hip.so.  libsr_tiled.so, C ABI in include/sr_tiled.h; why it is a library of its own:
// csrc/sidelib.py.
#include <cmath>
#include <cstdint>
#include "../../../include/sr_tiled.h"
#define SR_SIDE tiled
#define SR_SIDE_UC TILED
#ifndef SR_TILED_SRC_HASH
#define SR_TILED_SRC_HASH "unstamped"
#endif
#include "../sr_side.h"
#define SR_F16 SR_TILED_F16

namespace {

__device__ __forceinline__ float sr_load_f(const float* p) { return *p; }
__device__ __forceinline__ float sr_load_f(const _Float16* p) { return (float)*p; }
__device__ __forceinline__ void sr_store_f(float* p, float v) { *p = v; }
__device__ __forceinline__ void sr_store_f(_Float16* p, float v) { *p = (_Float16)v; }

// row softmax over the first `cols` entries of rows that are `ld` apart; entries [cols, ld) are written as 0 (the zero-padded
// key columns of the VAE mid attention when h*w is no multiple of the GEMM's K-step)
template <typename T>
__global__ __launch_bounds__(256) void softmax_rows_ld_kernel(T* __restrict__ x, int cols, int ld) {
  __shared__ float red[4];
  T* row = x + (int64_t)blockIdx.x * ld;
  const int tid = threadIdx.x;
  float mx = -INFINITY;
  for (int i = tid; i < cols; i += 256) mx = fmaxf(mx, sr_load_f(row + i));
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float s = 0.f;
  for (int i = tid; i < cols; i += 256) s += __expf(sr_load_f(row + i) - mx);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  s = (red[0] + red[1]) + (red[2] + red[3]);
  const float inv = 1.0f / s;
  for (int i = tid; i < cols; i += 256) sr_store_f(row + i, __expf(sr_load_f(row + i) - mx) * inv);
  for (int i = cols + tid; i < ld; i += 256) sr_store_f(row + i, 0.f);
}

// ---- tiled VAE (comfy/utils.py:448-475 tiled_scale; comfy/sd.py:302-327 decode_tiled_ / encode_tiled_) -----------------------
// A "plane" is one (H, W) image of `cpp` interleaved components per pixel: cpp = 1 for NCHW tensors (planes = B*C), cpp = C for
// NHWC ones (planes = B).  A tile row is then tw*cpp contiguous floats on both sides; VEC = 4 moves it as float4 when every row
// start is 16-byte aligned (the decoder's 8x-upscaled RGB rows always are).

// Launch shape of the three kernels: blockIdx.z = plane, blockIdx.y = row, x over the row's chunks, so a thread's position is
// 32-bit arithmetic and the row's weight is computed once per workgroup (uniform).

// s_in = s[:, :, y:y+tile_y, x:x+tile_x] (utils.py:459): dst[p, i, j] = src[p, y0 + i, x0 + j]
template <int VEC>
__global__ void tile_gather_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int y0, int x0, int th, int tw) {
  const int j = (blockIdx.x * blockDim.x + threadIdx.x) * VEC;
  if (j >= tw) return;
  const int i = blockIdx.y;
  const int64_t p = blockIdx.z;
  const float* s = src + ((p * H + (y0 + i)) * W + x0) + j;
  float* d = dst + (p * th + i) * tw + j;
  if constexpr (VEC == 4) *(float4*)d = *(const float4*)s; else *d = *s;
}

// numerator of one axis' feather weight f(i, n) = w / feather^2 (utils.py:462-468: the in-place mask multiplies BOTH ramps where a
// tile is narrower than 2*feather); an integer <= feather^2 <= 2^24, so the weight sum over the tiles of a pass is exact
__device__ __forceinline__ int feather_num(int i, int n, int feather) {
  if (feather <= 0) return 1;
  const int a = i < feather ? i + 1 : feather;
  const int b = n - 1 - i < feather ? n - i : feather;
  return a * b;
}

// out[window] += ps * mask ; out_div[window] += mask (utils.py:469-470) for every plane.  The mask is the same for every plane, so
// its sum is kept once per pixel, as the integer numerator over feather^4; plane 0's threads add it.  One launch touches every
// element of the window once (no atomics); launches of a pass are ordered by the stream.  The weight is rounded to fp32 once (from
// the exact product in fp64) and enters through one fma, which is what the (n + 3) * 2^-24 bound of the blend rests on.
template <int VEC>
__global__ void tile_accumulate_kernel(const float* __restrict__ tile, float* __restrict__ acc, long long* __restrict__ wsum, int H, int W,
                                       int cpp, int y0, int x0, int th, int tw, int feather, double inv_f4) {
  const int L = tw * cpp;
  const int e0 = (blockIdx.x * blockDim.x + threadIdx.x) * VEC;
  if (e0 >= L) return;
  const int i = blockIdx.y;
  const int64_t p = blockIdx.z;
  const float* s = tile + (p * th + i) * L + e0;
  float* d = acc + ((p * H + (y0 + i)) * W + x0) * cpp + e0;
  const int wi = feather_num(i, th, feather);
  const double wrow = (double)wi * inv_f4;                   // per row: uniform over the workgroup
  float t[VEC], a[VEC];
  if constexpr (VEC == 4) {
    const float4 tv = *(const float4*)s, av = *(const float4*)d;
    t[0] = tv.x; t[1] = tv.y; t[2] = tv.z; t[3] = tv.w;
    a[0] = av.x; a[1] = av.y; a[2] = av.z; a[3] = av.w;
  } else { t[0] = *s; a[0] = *d; }
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    const int e = e0 + k, j = e / cpp;
    const int wj = feather_num(j, tw, feather);
    a[k] = fmaf(t[k], (float)(wrow * (double)wj), a[k]);
    if (p == 0 && e - j * cpp == 0) wsum[(int64_t)(y0 + i) * W + (x0 + j)] += (long long)wi * wj;
  }
  if constexpr (VEC == 4) *(float4*)d = make_float4(a[0], a[1], a[2], a[3]); else *d = a[0];
}

// output = out / out_div per pass (utils.py:474), the passes averaged (sd.py:309-313, :323-326); mode 1 then applies process_output
// = clamp((x + 1) / 2, 0, 1) (sd.py:224), which the reference runs AFTER the average.  blockIdx.y = plane, x over H*W*cpp
__global__ void tile_finish_kernel(const float* __restrict__ a0, const float* __restrict__ a1, const float* __restrict__ a2,
                                   const long long* __restrict__ w0, const long long* __restrict__ w1, const long long* __restrict__ w2,
                                   float* __restrict__ out, int per_plane, int cpp, int npass, double f4, int mode) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= per_plane) return;
  const int pix = e / cpp;
  const int64_t at = (int64_t)blockIdx.y * per_plane + e;
  double s = (double)a0[at] * f4 / (double)w0[pix];
  if (npass > 1) s += (double)a1[at] * f4 / (double)w1[pix];
  if (npass > 2) s += (double)a2[at] * f4 / (double)w2[pix];
  float o = (float)(s / (double)npass);
  if (mode == 1) o = fminf(fmaxf((o + 1.0f) / 2.0f, 0.0f), 1.0f);
  out[at] = o;
}

inline unsigned cdiv256(int64_t n) { return (unsigned)((n + 255) / 256); }
// one row of a tile per workgroup row: a wave is enough for the short rows of the encoder's latent tiles
inline unsigned row_block(int64_t chunks) { return chunks <= 64 ? 64u : 256u; }

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int sr_softmax_rows_ld(void* x, int32_t rows, int32_t cols, int32_t ld, int32_t dtype, void* stream) {
  if (!x || rows < 1 || cols < 1 || ld < cols) SR_FAIL(SR_ERR_INVALID, "sr_softmax_rows_ld: bad args (rows %d, cols %d, ld %d)", rows, cols, ld);
  if (dtype == SR_F16) hipLaunchKernelGGL(softmax_rows_ld_kernel<_Float16>, dim3(rows), dim3(256), 0, sr_stream(stream), (_Float16*)x, cols, ld);
  else hipLaunchKernelGGL(softmax_rows_ld_kernel<float>, dim3(rows), dim3(256), 0, sr_stream(stream), (float*)x, cols, ld);
  SR_CHECK_LAUNCH("sr_softmax_rows_ld");
  return SR_OK;
}

static bool tile_window_ok(int32_t planes, int32_t H, int32_t W, int32_t y0, int32_t x0, int32_t th, int32_t tw) {
  return planes >= 1 && planes <= 65535 && H >= 1 && W >= 1 && th >= 1 && th <= 65535 && tw >= 1 && y0 >= 0 && x0 >= 0 &&
         (int64_t)y0 + th <= H && (int64_t)x0 + tw <= W;                 // (planes and rows are grid dimensions)
}

extern "C" int sr_tile_gather(const float* src, float* dst, int32_t planes, int32_t H, int32_t W, int32_t y0, int32_t x0, int32_t th,
                              int32_t tw, void* stream) {
  if (!src || !dst || !tile_window_ok(planes, H, W, y0, x0, th, tw)) SR_FAIL(SR_ERR_INVALID, "sr_tile_gather: bad args (window outside the tensor?)");
  const bool vec = tw % 4 == 0 && W % 4 == 0 && x0 % 4 == 0 && al16(src) && al16(dst);
  const int64_t chunks = tw / (vec ? 4 : 1);
  const unsigned bs = row_block(chunks);
  const dim3 grid((unsigned)((chunks + bs - 1) / bs), th, planes);
  if (vec) hipLaunchKernelGGL(tile_gather_kernel<4>, grid, dim3(bs), 0, sr_stream(stream), src, dst, H, W, y0, x0, th, tw);
  else hipLaunchKernelGGL(tile_gather_kernel<1>, grid, dim3(bs), 0, sr_stream(stream), src, dst, H, W, y0, x0, th, tw);
  SR_CHECK_LAUNCH("sr_tile_gather");
  return SR_OK;
}

extern "C" int sr_tile_accumulate(const float* tile, float* acc, int64_t* wsum, int32_t planes, int32_t H, int32_t W, int32_t cpp, int32_t y0,
                                  int32_t x0, int32_t th, int32_t tw, int32_t feather, void* stream) {
  if (!tile || !acc || !wsum || cpp < 1 || feather < 0 || feather > SR_TILE_FEATHER_MAX || !tile_window_ok(planes, H, W, y0, x0, th, tw))
    SR_FAIL(SR_ERR_INVALID, "sr_tile_accumulate: bad args (window outside the tensor, or feather > %d?)", SR_TILE_FEATHER_MAX);
  const double f = feather > 0 ? (double)feather : 1.0, inv_f4 = 1.0 / (f * f * f * f);
  const int64_t row = (int64_t)tw * cpp;
  const bool vec = row % 4 == 0 && ((int64_t)W * cpp) % 4 == 0 && ((int64_t)x0 * cpp) % 4 == 0 && al16(tile) && al16(acc);
  if (row > 0x7fffffffLL / 2) SR_FAIL(SR_ERR_INVALID, "sr_tile_accumulate: tile row too long");
  const int64_t chunks = row / (vec ? 4 : 1);
  const unsigned bs = row_block(chunks);
  const dim3 grid((unsigned)((chunks + bs - 1) / bs), th, planes);
  if (vec) hipLaunchKernelGGL(tile_accumulate_kernel<4>, grid, dim3(bs), 0, sr_stream(stream), tile, acc, (long long*)wsum, H, W, cpp, y0, x0,
                              th, tw, feather, inv_f4);
  else hipLaunchKernelGGL(tile_accumulate_kernel<1>, grid, dim3(bs), 0, sr_stream(stream), tile, acc, (long long*)wsum, H, W, cpp, y0, x0, th,
                          tw, feather, inv_f4);
  SR_CHECK_LAUNCH("sr_tile_accumulate");
  return SR_OK;
}

extern "C" int sr_tile_finish(const float* acc0, const float* acc1, const float* acc2, const int64_t* wsum0, const int64_t* wsum1,
                              const int64_t* wsum2, float* out, int32_t planes, int32_t H, int32_t W, int32_t cpp, int32_t npass, int32_t feather,
                              int32_t mode, void* stream) {
  if (!out || planes < 1 || H < 1 || W < 1 || cpp < 1 || npass < 1 || npass > 3 || feather < 0 || feather > SR_TILE_FEATHER_MAX || (mode != 0 && mode != 1) ||
      !acc0 || !wsum0 || (npass > 1 && (!acc1 || !wsum1)) || (npass > 2 && (!acc2 || !wsum2)))
    SR_FAIL(SR_ERR_INVALID, "sr_tile_finish: bad args");
  const double f = feather > 0 ? (double)feather : 1.0;
  const int64_t per_plane = (int64_t)H * W * cpp;
  if (per_plane > 0x7fffffffLL / 2 || planes > 65535) SR_FAIL(SR_ERR_INVALID, "sr_tile_finish: plane too large (or more than 65535 planes)");
  hipLaunchKernelGGL(tile_finish_kernel, dim3(cdiv256(per_plane), planes), dim3(256), 0, sr_stream(stream), acc0, acc1, acc2, (const long long*)wsum0,
                     (const long long*)wsum1, (const long long*)wsum2, out, (int)per_plane, cpp, npass, f * f * f * f, mode);
  SR_CHECK_LAUNCH("sr_tile_finish");
  return SR_OK;
}

