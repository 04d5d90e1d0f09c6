// comfy.utils.common_upscale (comfyUI/comfy/utils.py:418-443): F.interpolate in five modes, bislerp (utils.py:335-409) and the 8-bit
// Lanczos of utils.py:411-416: bandwidth-bound, output-stationary kernels.  libsr_resample.so, C ABI in include/sr_resample.h; why
// it is a library of its own: csrc/sidelib.py.
#include <cmath>
#include <cstdint>
#include "../../../include/sr_resample.h"
#define SR_SIDE resample
#define SR_SIDE_UC RESAMPLE
#ifndef SR_RESAMPLE_SRC_HASH
#define SR_RESAMPLE_SRC_HASH "unstamped"
#endif
#include "../sr_side.h"

namespace {

struct Strides { int64_t n, c, y, x; };                      // in elements
inline Strides strides_of(const int64_t* s) { return Strides{s[0], s[1], s[2], s[3]}; }
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// Launch shape of every kernel here: blockIdx.z = image, blockIdx.y = output row, x over the row, so the row's taps are uniform over
// the workgroup and a thread's position is 32-bit arithmetic.  A wave is enough for the short rows of a latent.
inline unsigned row_block(int64_t chunks) { return chunks <= 64 ? 64u : 256u; }
inline bool grid_ok(int32_t N, int32_t rows) { return N <= 65535 && rows <= 65535; }
constexpr int32_t kMaxSide = 1 << 24;                        // (2 o + 1) * in stays far inside int64, o * stride inside int64

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- F.interpolate ---------------------------------------------------------------------------------------------------------------
// The taps of output index o along one axis: up to four (index, weight) pairs; returns how many.  Positions and weights in double:
// every size here is < 2^24, so (o + .5) * in is exact and s carries one rounding.
__device__ __forceinline__ int axis_taps(int mode, int o, int in, int out, int idx[4], double w[4]) {
  if (mode == SR_RESAMPLE_NEAREST_EXACT || mode == SR_RESAMPLE_NEAREST) {
    const int64_t num = mode == SR_RESAMPLE_NEAREST ? (int64_t)2 * o * in : (int64_t)(2 * o + 1) * in;
    idx[0] = min((int)(num / (2 * (int64_t)out)), in - 1);
    w[0] = 1.0;
    return 1;
  }
  const double s = ((double)o + 0.5) * (double)in / (double)out - 0.5;
  if (mode == SR_RESAMPLE_BILINEAR) {
    const double sc = s < 0.0 ? 0.0 : s;
    const int i0 = min((int)floor(sc), in - 1);
    const double l = sc - (double)i0;
    idx[0] = i0;
    idx[1] = min(i0 + 1, in - 1);
    w[0] = 1.0 - l;
    w[1] = l;
    return 2;
  }
  const double A = -0.75, f = floor(s), t = s - f;             // bicubic
  const int i0 = (int)f - 1;
#pragma unroll
  for (int k = 0; k < 4; ++k) idx[k] = clampi(i0 + k, 0, in - 1);
  const double x0 = t + 1.0, x1 = t, x2 = 1.0 - t, x3 = 2.0 - t;
  w[0] = fma(fma(fma(A, x0, -5.0 * A), x0, 8.0 * A), x0, -4.0 * A);
  w[1] = fma(fma(A + 2.0, x1, -(A + 3.0)), x1 * x1, 1.0);
  w[2] = fma(fma(A + 2.0, x2, -(A + 3.0)), x2 * x2, 1.0);
  w[3] = fma(fma(fma(A, x3, -5.0 * A), x3, 8.0 * A), x3, -4.0 * A);
  return 4;
}

// the XV outputs of a thread: one 16-byte store where the caller found every row start aligned and the chunk is whole, else a scalar tail
template <int XV>
__device__ __forceinline__ void store_outputs(float* d, const float (&o)[XV], int x0, int Wo, int64_t dx, bool vec) {
  if constexpr (XV == 4) {
    if (vec) { *(float4*)(d + x0) = make_float4(o[0], o[1], o[2], o[3]); return; }
  }
#pragma unroll
  for (int v = 0; v < XV; ++v) if (x0 + v < Wo) d[(int64_t)(x0 + v) * dx] = o[v];
}

// A thread makes XV consecutive x outputs of one row for every channel: its x taps live in registers and serve all C channels, the
// row's y taps are the same for the whole workgroup.  XV = 4 for planar layouts (float4 store where `vec_store` says every row
// start of dst is 16-byte aligned and its x stride is 1; neighbouring threads read neighbouring x), XV = 1 for interleaved
// ones, where a pixel's channels are adjacent in memory and sit in one thread.  `mode` is uniform: one kernel serves all five.
template <int XV>
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, int Hi, int Wi, int Ho,
                                                       int Wo, Strides ss, Strides ds, int mode, int vec_store) {
  const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * XV;
  if (x0 >= Wo) return;
  const int yo = blockIdx.y;
  const float* sn = src + (int64_t)blockIdx.z * ss.n;
  float* dn = dst + (int64_t)blockIdx.z * ds.n + (int64_t)yo * ds.y;
  const bool full = x0 + XV <= Wo;
  float o[XV];
  if (mode == SR_RESAMPLE_AREA) {
    const int ys = (int)((int64_t)yo * Hi / Ho), ye = (int)(((int64_t)(yo + 1) * Hi + Ho - 1) / Ho);
    int xs[XV], xe[XV];
#pragma unroll
    for (int v = 0; v < XV; ++v) {
      const int xo = min(x0 + v, Wo - 1);                    // (a chunk's tail repeats the last column and is not stored)
      xs[v] = (int)((int64_t)xo * Wi / Wo);
      xe[v] = (int)(((int64_t)(xo + 1) * Wi + Wo - 1) / Wo);
    }
    for (int c = 0; c < C; ++c) {
      const float* sc = sn + (int64_t)c * ss.c;
#pragma unroll
      for (int v = 0; v < XV; ++v) {
        double s = 0.0;
        for (int y = ys; y < ye; ++y) {
          const float* row = sc + (int64_t)y * ss.y;
          for (int x = xs[v]; x < xe[v]; ++x) s += (double)row[(int64_t)x * ss.x];
        }
        o[v] = (float)(s / (double)((int64_t)(ye - ys) * (xe[v] - xs[v])));
      }
      store_outputs<XV>(dn + (int64_t)c * ds.c, o, x0, Wo, ds.x, vec_store && full);
    }
    return;
  }
  int iy[4], ix[XV][4];
  double wy[4], wx[XV][4];
  const int ny = axis_taps(mode, yo, Hi, Ho, iy, wy);
  int nx = 1;
#pragma unroll
  for (int v = 0; v < XV; ++v) nx = axis_taps(mode, min(x0 + v, Wo - 1), Wi, Wo, ix[v], wx[v]);
  for (int c = 0; c < C; ++c) {
    const float* sc = sn + (int64_t)c * ss.c;
    double acc[XV];
#pragma unroll
    for (int v = 0; v < XV; ++v) acc[v] = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= ny) break;
      const float* row = sc + (int64_t)iy[j] * ss.y;
#pragma unroll
      for (int v = 0; v < XV; ++v) {
        double h = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (i >= nx) break;
          h = fma(wx[v][i], (double)row[(int64_t)ix[v][i] * ss.x], h);
        }
        acc[v] = fma(wy[j], h, acc[v]);
      }
    }
#pragma unroll
    for (int v = 0; v < XV; ++v) o[v] = (float)acc[v];
    store_outputs<XV>(dn + (int64_t)c * ds.c, o, x0, Wo, ds.x, vec_store && full);
  }
}

// ---- bislerp -----------------------------------------------------------------------------------------------------------------------
// One slerp pass along x (`along_x`) or y of an (N, C, *, *) tensor with strides `is` into a contiguous (N, C, H, W) tensor: a thread
// makes one output pixel, all C channels.  First sweep over the channels: the two norms and the dot product; then acos and the three
// sines once; second sweep: the C outputs (the second read of the 2 C inputs comes from cache).
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void slerp_kernel(const TI* __restrict__ in, TO* __restrict__ out, int C, int H, int W, Strides is, int in_len,
                                                    const float* __restrict__ ratio, const int* __restrict__ idx1, const int* __restrict__ idx2,
                                                    int along_x) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= W) return;
  const int y = blockIdx.y;
  const int64_t n = blockIdx.z;
  const int o = along_x ? x : y;
  const double r = (double)ratio[o];
  const int a = clampi(idx1[o], 0, in_len - 1), b = clampi(idx2[o], 0, in_len - 1);
  const TI* base = in + n * is.n;
  const TI* p1 = base + (along_x ? (int64_t)y * is.y + (int64_t)a * is.x : (int64_t)a * is.y + (int64_t)x * is.x);
  const TI* p2 = base + (along_x ? (int64_t)y * is.y + (int64_t)b * is.x : (int64_t)b * is.y + (int64_t)x * is.x);
  double q1 = 0.0, q2 = 0.0, d12 = 0.0;
  for (int c = 0; c < C; ++c) {
    const double v1 = (double)p1[(int64_t)c * is.c], v2 = (double)p2[(int64_t)c * is.c];
    q1 = fma(v1, v1, q1);
    q2 = fma(v2, v2, q2);
    d12 = fma(v1, v2, d12);
  }
  const double n1 = sqrt(q1), n2 = sqrt(q2);
  const double inv1 = n1 == 0.0 ? 0.0 : 1.0 / n1, inv2 = n2 == 0.0 ? 0.0 : 1.0 / n2;    // normalised vector = 0 where the norm is 0
  const double dot = d12 * inv1 * inv2;
  double k1, k2;                                             // res = k1 * b1 + k2 * b2
  if (dot < 1e-5 - 1.0) { k1 = 1.0 - r; k2 = r; }            // opposite: plain lerp (utils.py:364, applied last)
  else if (dot > 1.0 - 1e-5) { k1 = 1.0; k2 = 0.0; }         // same direction: b1 (utils.py:363)
  else {
    const double omega = acos(dot), so = sin(omega), scale = n1 * (1.0 - r) + n2 * r;
    k1 = sin((1.0 - r) * omega) / so * inv1 * scale;
    k2 = sin(r * omega) / so * inv2 * scale;
  }
  TO* q = out + ((n * C) * H + y) * (int64_t)W + x;
  for (int c = 0; c < C; ++c) {
    const double v1 = (double)p1[(int64_t)c * is.c], v2 = (double)p2[(int64_t)c * is.c];
    q[(int64_t)c * H * W] = (TO)fma(k2, v2, k1 * v1);
  }
}

// ---- 8-bit Lanczos -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lz_load(const float* p) { return (int)fminf(fmaxf(255.f * *p, 0.f), 255.f); }   // .astype(uint8) truncates
__device__ __forceinline__ int lz_load(const uint8_t* p) { return (int)*p; }
__device__ __forceinline__ void lz_store(uint8_t* p, int v) { *p = (uint8_t)v; }
__device__ __forceinline__ void lz_store(float* p, int v) { *p = (float)v / 255.0f; }

// One pass of PIL's 8-bit resample along x (`along_x`) or y: out = clip8((2^21 + sum q * k) >> 22), a thread makes one pixel's three
// channels.  k == nullptr: no pass at all (both sizes unchanged), the pixel is only quantised.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void lanczos_pass_kernel(const TI* __restrict__ in, TO* __restrict__ out, int W, Strides is, Strides os, int in_len,
                                                           const int* __restrict__ bounds, const int* __restrict__ k, int ksize, int along_x) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= W) return;
  const int y = blockIdx.y;
  const int64_t n = blockIdx.z;
  const int o = along_x ? x : y;
  const int64_t st = along_x ? is.x : is.y;
  const TI* p = in + n * is.n + (along_x ? (int64_t)y * is.y : (int64_t)x * is.x);      // + c * is.c + tap * st
  int v0, v1, v2;
  if (!k) {
    v0 = lz_load(p + (int64_t)o * st); v1 = lz_load(p + is.c + (int64_t)o * st); v2 = lz_load(p + 2 * is.c + (int64_t)o * st);
  } else {
    const int lo = clampi(bounds[2 * o], 0, in_len - 1);
    const int cnt = min(min(bounds[2 * o + 1], ksize), in_len - lo);
    const int* kk = k + (int64_t)o * ksize;
    int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;             // 255 * sum |k| < 2^31: the normalised Lanczos-3 weights sum to < 2 in magnitude
    for (int i = 0; i < cnt; ++i) {
      const TI* t = p + (int64_t)(lo + i) * st;
      const int w = kk[i];
      s0 += lz_load(t) * w; s1 += lz_load(t + is.c) * w; s2 += lz_load(t + 2 * is.c) * w;
    }
    v0 = clampi(s0 >> 22, 0, 255); v1 = clampi(s1 >> 22, 0, 255); v2 = clampi(s2 >> 22, 0, 255);
  }
  TO* q = out + n * os.n + (int64_t)y * os.y + (int64_t)x * os.x;
  lz_store(q, v0); lz_store(q + os.c, v1); lz_store(q + 2 * os.c, v2);
}

template <typename TI, typename TO>
void lanczos_launch(const TI* in, TO* out, int32_t N, int32_t H, int32_t W, Strides is, Strides os, int32_t in_len, const int32_t* bounds,
                    const int32_t* k, int32_t ksize, int along_x, hipStream_t st) {
  const unsigned bs = row_block(W);
  hipLaunchKernelGGL((lanczos_pass_kernel<TI, TO>), dim3((W + bs - 1) / bs, H, N), dim3(bs), 0, st, in, out, W, is, os, in_len, bounds, k, ksize,
                     along_x);
}

inline bool sizes_ok(int32_t N, int32_t C, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo) {
  return N >= 1 && C >= 1 && Hi >= 1 && Wi >= 1 && Ho >= 1 && Wo >= 1 && Hi <= kMaxSide && Wi <= kMaxSide && Ho <= kMaxSide && Wo <= kMaxSide;
}

}  // namespace

extern "C" int sr_resample(const float* src, float* dst, int32_t N, int32_t C, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                           const int64_t* src_strides, const int64_t* dst_strides, int32_t mode, void* stream) {
  if (!src || !dst || !src_strides || !dst_strides) SR_FAIL(SR_ERR_INVALID, "sr_resample: null pointer");
  if (!sizes_ok(N, C, Hi, Wi, Ho, Wo)) SR_FAIL(SR_ERR_INVALID, "sr_resample: sizes must be positive (N %d, C %d, %d x %d -> %d x %d)", N, C, Hi, Wi, Ho, Wo);
  if (mode < SR_RESAMPLE_NEAREST_EXACT || mode > SR_RESAMPLE_AREA) SR_FAIL(SR_ERR_INVALID, "sr_resample: unknown mode %d", mode);
  if (!grid_ok(N, Ho)) SR_FAIL(SR_ERR_INVALID, "sr_resample: more than 65535 images or output rows");
  const Strides ss = strides_of(src_strides), ds = strides_of(dst_strides);
  // interleaved (NHWC memory behind an (n, c, y, x) view): a pixel's channels are adjacent on both sides
  const bool interleaved = C > 1 && ss.c == 1 && ds.c == 1;
  const hipStream_t st = sr_stream(stream);
  if (interleaved) {
    const unsigned bs = row_block(Wo);
    hipLaunchKernelGGL(resample_kernel<1>, dim3((Wo + bs - 1) / bs, Ho, N), dim3(bs), 0, st, src, dst, C, Hi, Wi, Ho, Wo, ss, ds, mode, 0);
  } else {
    const int vec = ds.x == 1 && al16(dst) && ds.n % 4 == 0 && ds.c % 4 == 0 && ds.y % 4 == 0;
    const int64_t chunks = ((int64_t)Wo + 3) / 4;
    const unsigned bs = row_block(chunks);
    hipLaunchKernelGGL(resample_kernel<4>, dim3((unsigned)((chunks + bs - 1) / bs), Ho, N), dim3(bs), 0, st, src, dst, C, Hi, Wi, Ho, Wo, ss, ds,
                       mode, vec);
  }
  SR_CHECK_LAUNCH("sr_resample");
  return SR_OK;
}

extern "C" int sr_bislerp(const float* src, float* dst, double* tmp, int32_t N, int32_t C, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                          const int64_t* src_strides, const float* x_ratio, const int32_t* x_idx1, const int32_t* x_idx2, const float* y_ratio,
                          const int32_t* y_idx1, const int32_t* y_idx2, void* stream) {
  if (!src || !dst || !tmp || !src_strides || !x_ratio || !x_idx1 || !x_idx2 || !y_ratio || !y_idx1 || !y_idx2)
    SR_FAIL(SR_ERR_INVALID, "sr_bislerp: null pointer");
  if (!sizes_ok(N, C, Hi, Wi, Ho, Wo)) SR_FAIL(SR_ERR_INVALID, "sr_bislerp: sizes must be positive (N %d, C %d, %d x %d -> %d x %d)", N, C, Hi, Wi, Ho, Wo);
  if (!grid_ok(N, Hi) || !grid_ok(N, Ho)) SR_FAIL(SR_ERR_INVALID, "sr_bislerp: more than 65535 images or rows");
  const hipStream_t st = sr_stream(stream);
  const unsigned bs = row_block(Wo);
  const dim3 gx((Wo + bs - 1) / bs, Hi, N), gy((Wo + bs - 1) / bs, Ho, N);
  const Strides ts{(int64_t)C * Hi * Wo, (int64_t)Hi * Wo, (int64_t)Wo, 1};
  hipLaunchKernelGGL((slerp_kernel<float, double>), gx, dim3(bs), 0, st, src, tmp, C, Hi, Wo, strides_of(src_strides), Wi, x_ratio, x_idx1, x_idx2, 1);
  SR_CHECK_LAUNCH("sr_bislerp");
  hipLaunchKernelGGL((slerp_kernel<double, float>), gy, dim3(bs), 0, st, (const double*)tmp, dst, C, Ho, Wo, ts, Hi, y_ratio, y_idx1, y_idx2, 0);
  SR_CHECK_LAUNCH("sr_bislerp");
  return SR_OK;
}

extern "C" int sr_lanczos_rgb8(const float* src, float* dst, uint8_t* tmp_u8, int32_t N, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                               const int64_t* src_strides, const int64_t* dst_strides, const int32_t* x_bounds, const int32_t* x_k, int32_t x_ksize,
                               const int32_t* y_bounds, const int32_t* y_k, int32_t y_ksize, void* stream) {
  if (!src || !dst || !src_strides || !dst_strides) SR_FAIL(SR_ERR_INVALID, "sr_lanczos_rgb8: null pointer");
  if (!sizes_ok(N, 3, Hi, Wi, Ho, Wo)) SR_FAIL(SR_ERR_INVALID, "sr_lanczos_rgb8: sizes must be positive (N %d, %d x %d -> %d x %d)", N, Hi, Wi, Ho, Wo);
  const bool horiz = Wi != Wo, vert = Hi != Ho;
  if ((horiz && (!x_bounds || !x_k || x_ksize < 1)) || (vert && (!y_bounds || !y_k || y_ksize < 1)) || (horiz && vert && !tmp_u8))
    SR_FAIL(SR_ERR_INVALID, "sr_lanczos_rgb8: a pass that changes a size needs its tables, and two passes need tmp_u8");
  if (!grid_ok(N, Hi) || !grid_ok(N, Ho)) SR_FAIL(SR_ERR_INVALID, "sr_lanczos_rgb8: more than 65535 images or rows");
  const hipStream_t st = sr_stream(stream);
  const Strides ss = strides_of(src_strides), ds = strides_of(dst_strides);
  const Strides ts{(int64_t)Hi * Wo * 3, 1, (int64_t)Wo * 3, 3};          // tmp_u8 (N, Hi, Wo, 3)
  if (horiz && vert) {
    lanczos_launch(src, tmp_u8, N, Hi, Wo, ss, ts, Wi, x_bounds, x_k, x_ksize, 1, st);
    SR_CHECK_LAUNCH("sr_lanczos_rgb8");
    lanczos_launch((const uint8_t*)tmp_u8, dst, N, Ho, Wo, ts, ds, Hi, y_bounds, y_k, y_ksize, 0, st);
  } else if (horiz) {
    lanczos_launch(src, dst, N, Ho, Wo, ss, ds, Wi, x_bounds, x_k, x_ksize, 1, st);
  } else if (vert) {
    lanczos_launch(src, dst, N, Ho, Wo, ss, ds, Hi, y_bounds, y_k, y_ksize, 0, st);
  } else {
    lanczos_launch(src, dst, N, Ho, Wo, ss, ds, Wi, (const int32_t*)nullptr, (const int32_t*)nullptr, 0, 1, st);
  }
  SR_CHECK_LAUNCH("sr_lanczos_rgb8");
  return SR_OK;
}
