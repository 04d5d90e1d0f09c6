// The image and mask filters of ComfyUI's comfy_extras/nodes_post_processing.py (Blur, Sharpen, Blend) and comfy_extras/nodes_mask.py
// (composite(), GrowMask, FeatherMask, MaskComposite, ImageColorToMask).  libsr_imgproc.so, C ABI in include/sr_imgproc.h; why it
// is a library of its own: csrc/sidelib.py.
#include <cmath>
#include <cstdint>
#include "../../../include/sr_imgproc.h"
#define SR_SIDE imgproc
#define SR_SIDE_UC IMGPROC
#ifndef SR_IMGPROC_SRC_HASH
#define SR_IMGPROC_SRC_HASH "unstamped"
#endif
#include "../sr_side.h"

namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxElems = (int64_t)1 << 31;              // a flat 1-D grid of 256-thread blocks stays below 2^23 blocks
constexpr int32_t kMaxSide = 1 << 24;
inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }
inline unsigned cdiv(int a, int b) { return (unsigned)((a + b - 1) / b); }

struct S3 { int64_t n, y, x; };                              // element strides of a MASK (N,H,W)
struct S4 { int64_t n, y, x, c; };                           // of an IMAGE (B,H,W,C)
struct S4c { int64_t n, c, y, x; };                          // of a (B,C,H,W) tensor or view
inline S3 s3(const int64_t* s) { return S3{s[0], s[1], s[2]}; }
inline S4 s4(const int64_t* s) { return S4{s[0], s[1], s[2], s[3]}; }
inline S4c s4c(const int64_t* s) { return S4c{s[0], s[1], s[2], s[3]}; }

// ---- Blur / Sharpen ----------------------------------------------------------------------------------------------------------------
// One workgroup makes a TH x TW pixel tile of CB channels at a time (CB = C: the staged rows are runs of the NHWC row, read
// coalesced; CB = 1 where all channels of the haloed tile would not fit, i.e. at large radii, where the kernel is bound by the taps
// and not by HBM).  LDS: mid[(TH + 2r)][TW * CB] double, then in[(TH + 2r)][(TW + 2r) * CB] float.
//   stage       in  <- src through reflect(y), reflect(x)
//   horizontal  mid[row][e] = sum_k w[k] in[row][e + k CB]              (double)
//   vertical    out[ty][e]  = sum_k w[k] mid[ty + k][e]                 (double, rounded once)
// Neighbouring lanes touch neighbouring LDS words in all three loops: no bank conflicts.  Every sum runs in tap order: equal bits
// run to run.
// i / d for 0 <= i * d < 2^32 (here i < 2^16, d < 2^9) as one multiply: m = ceil(2^32 / d); d == 1 passes i through
struct FastDiv { uint32_t d, m; };
inline FastDiv fastdiv(int d) { return FastDiv{(uint32_t)d, d == 1 ? 0u : (uint32_t)((((uint64_t)1 << 32) + d - 1) / d)}; }
__device__ __forceinline__ int div_by(int i, FastDiv f) { return f.d == 1 ? i : (int)__umulhi((uint32_t)i, f.m); }

struct GaussWeights { double w[2 * SR_GAUSS_MAX_RADIUS + 1]; };
struct GaussTile { int th, tw, cb; };
inline size_t gauss_lds_bytes(GaussTile t, int r) {
  return (size_t)(t.th + 2 * r) * t.tw * t.cb * sizeof(double) + (size_t)(t.th + 2 * r) * (t.tw + 2 * r) * t.cb * sizeof(float);
}
constexpr size_t kGaussLdsBudget = 64 * 1024;               // two workgroups or more per CU of 160 KB

// reflect without repeating the edge (torch's 'reflect'), then clamped: rows of a tile that hang over the image are never used, but
// their loads stay inside it
__device__ __forceinline__ int reflect_clamped(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

__global__ __launch_bounds__(kThreads) void gauss_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int C, S4 ss,
                                                         int r, int TH, int TW, int CB, FastDiv by_in, FastDiv by_mid, FastDiv by_cb, double amount,
                                                         GaussWeights gw) {
  extern __shared__ double lds[];
  const int rows = TH + 2 * r, in_len = (TW + 2 * r) * CB, mid_len = TW * CB, taps = 2 * r + 1;
  double* mid = lds;
  float* in = (float*)(lds + (size_t)rows * mid_len);
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const float* sn = src + (int64_t)blockIdx.z * ss.n;
  float* dn = dst + (int64_t)blockIdx.z * H * W * C;
  for (int c0 = 0; c0 < C; c0 += CB) {
    for (int i = threadIdx.x; i < rows * in_len; i += kThreads) {
      const int row = div_by(i, by_in), e = i - row * in_len, px = div_by(e, by_cb), ch = c0 + (e - px * CB);
      const int gy = reflect_clamped(y0 - r + row, H), gx = reflect_clamped(x0 - r + px, W);
      in[i] = sn[(int64_t)gy * ss.y + (int64_t)gx * ss.x + (int64_t)ch * ss.c];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < rows * mid_len; i += kThreads) {
      const int row = div_by(i, by_mid), e = i - row * mid_len;
      const float* p = in + row * in_len + e;
      double acc = 0.0;
      for (int k = 0; k < taps; ++k) acc = fma(gw.w[k], (double)p[k * CB], acc);
      mid[i] = acc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TH * mid_len; i += kThreads) {
      const int ty = div_by(i, by_mid), e = i - ty * mid_len, px = div_by(e, by_cb), ch = c0 + (e - px * CB);
      const int y = y0 + ty, x = x0 + px;
      if (y >= H || x >= W) continue;
      const double* p = mid + ty * mid_len + e;
      double acc = 0.0;
      for (int k = 0; k < taps; ++k) acc = fma(gw.w[k], p[k * mid_len], acc);
      if (amount > 0.0) {
        const double centre = (double)in[(ty + r) * in_len + e + r * CB];
        acc = fma(1.0 + amount, centre, -amount * acc);
        acc = acc < 0.0 ? 0.0 : (acc > 1.0 ? 1.0 : acc);
      }
      dn[((int64_t)y * W + x) * C + ch] = (float)acc;
    }
    __syncthreads();
  }
}

// ---- GrowMask ----------------------------------------------------------------------------------------------------------------------
// `steps` <= SR_GROW_MAX_STEP iterations of the 3x3 max (or min) on a 32 x 64 tile and its halo of `steps` cells, ping-ponged in LDS.
// n iterations are one max over the ball of radius n (L1 for the cross, L-infinity for the full footprint), and max is exact and
// associative, so the ball is grown by doubling instead of one cell at a time: radius 1 directly, then from radius a to a + b,
// b <= a, as the max of four balls of radius a centred b away -- at (+-b, 0), (0, +-b) for the diamond, at (+-b, +-b) for the
// square; their union is the ball of radius a + b exactly when b <= a.  16 iterations are 5 passes of 4 to 9 LDS reads per cell.
// Cells outside the mask start as the neutral element (the reference's border mode repeats pixels that are in the window already);
// a cell whose ball of the current radius leaves the haloed tile is wrong, and no cell of the tile ever reads one.
constexpr int kGrowTH = 32, kGrowTW = 64;

template <bool ERODE>
__device__ __forceinline__ float pick(float a, float b) { return ERODE ? fminf(a, b) : fmaxf(a, b); }

template <bool ERODE>
__global__ __launch_bounds__(kThreads) void grow_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, S3 ss, int steps,
                                                        int full) {
  extern __shared__ double lds[];
  const int rows = kGrowTH + 2 * steps, cols = kGrowTW + 2 * steps, cells = rows * cols;
  float* a = (float*)lds;
  float* b = a + cells;
  const float neutral = ERODE ? INFINITY : -INFINITY;
  const int x0 = blockIdx.x * kGrowTW - steps, y0 = blockIdx.y * kGrowTH - steps;
  const float* sn = src + (int64_t)blockIdx.z * ss.n;
  for (int i = threadIdx.x; i < cells; i += kThreads) {
    const int ry = i / cols, rx = i - ry * cols, y = y0 + ry, x = x0 + rx;
    a[i] = (y >= 0 && y < H && x >= 0 && x < W) ? sn[(int64_t)y * ss.y + (int64_t)x * ss.x] : neutral;
  }
  __syncthreads();
  for (int radius = 0; radius < steps;) {
    const int d = radius == 0 ? 1 : min(radius, steps - radius);
    for (int i = threadIdx.x; i < cells; i += kThreads) {
      const int ry = i / cols, rx = i - ry * cols;
      const bool up = ry >= d, dn = ry < rows - d, lf = rx >= d, rt = rx < cols - d;
      float v = a[i];                                        // (from radius 1 on the centre lies inside the four balls; keeping it is harmless)
      if (!full || radius == 0) {
        if (up) v = pick<ERODE>(v, a[i - d * cols]);
        if (dn) v = pick<ERODE>(v, a[i + d * cols]);
        if (lf) v = pick<ERODE>(v, a[i - d]);
        if (rt) v = pick<ERODE>(v, a[i + d]);
      }
      if (full) {
        if (up && lf) v = pick<ERODE>(v, a[i - d * cols - d]);
        if (up && rt) v = pick<ERODE>(v, a[i - d * cols + d]);
        if (dn && lf) v = pick<ERODE>(v, a[i + d * cols - d]);
        if (dn && rt) v = pick<ERODE>(v, a[i + d * cols + d]);
      }
      b[i] = v;
    }
    __syncthreads();
    float* t = a;
    a = b;
    b = t;
    radius += d;
  }
  float* dn_ = dst + (int64_t)blockIdx.z * H * W;
  for (int i = threadIdx.x; i < kGrowTH * kGrowTW; i += kThreads) {
    const int ty = i / kGrowTW, tx = i - ty * kGrowTW, y = blockIdx.y * kGrowTH + ty, x = blockIdx.x * kGrowTW + tx;
    if (y < H && x < W) dn_[(int64_t)y * W + x] = a[(ty + steps) * cols + tx + steps];
  }
}

// ---- FeatherMask -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float rate(int k, int n) { return (float)((double)(k + 1) / (double)n); }

__global__ __launch_bounds__(kThreads) void feather_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t total, int H, int W,
                                                           S3 ss, int left, int top, int right, int bottom) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % W), y = (int)((i / W) % H);
  const int64_t n = i / ((int64_t)W * H);
  float v = src[n * ss.n + (int64_t)y * ss.y + (int64_t)x * ss.x];
  if (x < left) v *= rate(x, left);
  if (right > 0) {                                           // output[:, :, -k]: k = 0 is column 0, k >= 1 is column W - k
    if (x == 0) v *= rate(0, right);
    else if (W - x < right) v *= rate(W - x, right);
  }
  if (y < top) v *= rate(y, top);
  if (bottom > 0) {
    if (y == 0) v *= rate(0, bottom);
    else if (H - y < bottom) v *= rate(H - y, bottom);
  }
  dst[i] = v;
}

// ---- composite() -------------------------------------------------------------------------------------------------------------------
// c_inner: the channel is the fastest index of a thread's position (an IMAGE behind its movedim(-1, 1) view), else x is (a latent)
__global__ __launch_bounds__(kThreads) void composite_kernel(float* __restrict__ dst, const float* __restrict__ src, const float* __restrict__ mask,
                                                             int64_t total, int C, int Bs, int Bm, int top, int left, int h, int w, S4c ds,
                                                             S4c ss, S3 ms, int c_inner) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  int c, x, y;
  int64_t b;
  if (c_inner) {
    c = (int)(i % C);
    x = (int)((i / C) % w);
    y = (int)((i / ((int64_t)C * w)) % h);
  } else {
    x = (int)(i % w);
    y = (int)((i / w) % h);
    c = (int)((i / ((int64_t)w * h)) % C);
  }
  b = i / ((int64_t)C * w * h);
  float* d = dst + b * ds.n + (int64_t)c * ds.c + (int64_t)(top + y) * ds.y + (int64_t)(left + x) * ds.x;
  const float s = src[(b % Bs) * ss.n + (int64_t)c * ss.c + (int64_t)y * ss.y + (int64_t)x * ss.x];
  if (mask == nullptr) {
    *d = s;
    return;
  }
  const double m = (double)mask[(b % Bm) * ms.n + (int64_t)y * ms.y + (int64_t)x * ms.x];
  *d = (float)(m * (double)s + (1.0 - m) * (double)*d);
}

// ---- Blend -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double soft_g(double x) { return x <= 0.25 ? ((16.0 * x - 12.0) * x + 4.0) * x : sqrt(x); }

__global__ __launch_bounds__(kThreads) void blend_kernel(const float* __restrict__ pa, const float* __restrict__ pb, float* __restrict__ dst,
                                                         int64_t total, int H, int W, int C, S4 as, S4 bs, double f, int mode) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C), x = (int)((i / C) % W), y = (int)((i / ((int64_t)C * W)) % H);
  const int64_t n = i / ((int64_t)C * W * H);
  const double a = (double)pa[n * as.n + (int64_t)y * as.y + (int64_t)x * as.x + (int64_t)c * as.c];
  const double b = (double)pb[n * bs.n + (int64_t)y * bs.y + (int64_t)x * bs.x + (int64_t)c * bs.c];
  double m;
  switch (mode) {
    case SR_BLEND_NORMAL: m = b; break;
    case SR_BLEND_MULTIPLY: m = a * b; break;
    case SR_BLEND_SCREEN: m = 1.0 - (1.0 - a) * (1.0 - b); break;
    case SR_BLEND_OVERLAY: m = a <= 0.5 ? 2.0 * a * b : 1.0 - 2.0 * (1.0 - a) * (1.0 - b); break;
    case SR_BLEND_SOFT_LIGHT: m = b <= 0.5 ? a - (1.0 - 2.0 * b) * a * (1.0 - a) : a + (2.0 * b - 1.0) * (soft_g(a) - a); break;
    default: m = a - b; break;
  }
  double o = a * (1.0 - f) + m * f;
  o = o < 0.0 ? 0.0 : (o > 1.0 ? 1.0 : o);
  dst[i] = (float)o;
}

// ---- MaskComposite -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

__global__ __launch_bounds__(kThreads) void combine_kernel(const float* __restrict__ dest, const float* __restrict__ source, float* __restrict__ dst,
                                                           int64_t total, int H, int W, int Ns, S3 ds, S3 ss, int x0, int y0, int x1, int y1,
                                                           int op) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % W), y = (int)((i / W) % H);
  const int64_t n = i / ((int64_t)W * H);
  float d = dest[n * ds.n + (int64_t)y * ds.y + (int64_t)x * ds.x];
  if (x >= x0 && x < x1 && y >= y0 && y < y1) {
    const float s = source[(Ns == 1 ? 0 : n) * ss.n + (int64_t)(y - y0) * ss.y + (int64_t)(x - x0) * ss.x];
    const bool bd = rintf(d) != 0.0f, bs = rintf(s) != 0.0f;
    switch (op) {
      case SR_COMBINE_MULTIPLY: d = d * s; break;
      case SR_COMBINE_ADD: d = d + s; break;
      case SR_COMBINE_SUBTRACT: d = d - s; break;
      case SR_COMBINE_AND: d = (bd && bs) ? 1.0f : 0.0f; break;
      case SR_COMBINE_OR: d = (bd || bs) ? 1.0f : 0.0f; break;
      default: d = (bd != bs) ? 1.0f : 0.0f; break;
    }
  }
  dst[i] = clamp01(d);
}

// ---- ImageColorToMask --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void color_kernel(const float* __restrict__ img, float* __restrict__ dst, int64_t total, int H, int W, S4 is,
                                                         int color) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % W), y = (int)((i / W) % H);
  const int64_t n = i / ((int64_t)W * H);
  const float* p = img + n * is.n + (int64_t)y * is.y + (int64_t)x * is.x;
  int packed = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) packed = (packed << 8) + (int)rintf(clamp01(p[(int64_t)c * is.c]) * 255.0f);
  dst[i] = packed == color ? 255.0f : 0.0f;
}

inline bool sides_ok(int32_t a, int32_t b) { return a >= 1 && b >= 1 && a <= kMaxSide && b <= kMaxSide; }

}  // namespace

extern "C" int sr_filter_gauss(const float* src, float* dst, int32_t B, int32_t H, int32_t W, int32_t C, const int64_t* src_strides,
                               int32_t radius, double sigma, double amount, void* stream) {
  if (!src || !dst || !src_strides) SR_FAIL(SR_ERR_INVALID, "sr_filter_gauss: null pointer");
  if (B < 1 || !sides_ok(H, W) || (int64_t)B * H * W * 4 >= kMaxElems) SR_FAIL(SR_ERR_INVALID, "sr_filter_gauss: sizes %d x %d x %d", B, H, W);
  if (C < 1 || C > 4) SR_FAIL(SR_ERR_INVALID, "sr_filter_gauss: 1 to 4 channels, got %d", C);
  if (radius < 1 || radius > SR_GAUSS_MAX_RADIUS) SR_FAIL(SR_ERR_INVALID, "sr_filter_gauss: radius %d is not in 1..%d", radius, SR_GAUSS_MAX_RADIUS);
  if (radius >= H || radius >= W) SR_FAIL(SR_ERR_INVALID, "sr_filter_gauss: radius %d needs an image larger than %d x %d (reflect padding)", radius, H, W);
  if (!(sigma > 0.0) || !(amount >= 0.0) || !std::isfinite(sigma) || !std::isfinite(amount))
    SR_FAIL(SR_ERR_INVALID, "sr_filter_gauss: sigma %g must be > 0 and amount %g >= 0", sigma, amount);
  GaussWeights gw;
  const int taps = 2 * radius + 1;
  double sum = 0.0;
  for (int k = 0; k < taps; ++k) {
    const double t = -1.0 + 2.0 * (double)k / (double)(taps - 1);
    gw.w[k] = std::exp(-(t * t) / (2.0 * sigma * sigma));
    sum += gw.w[k];
  }
  for (int k = 0; k < taps; ++k) gw.w[k] /= sum;
  for (int k = taps; k < 2 * SR_GAUSS_MAX_RADIUS + 1; ++k) gw.w[k] = 0.0;
  const GaussTile cand[3] = {{32, 32, C}, {16, 32, C}, {32, 32, 1}};
  GaussTile t = cand[2];
  for (int i = 0; i < 3; ++i)
    if (gauss_lds_bytes(cand[i], radius) <= kGaussLdsBudget) { t = cand[i]; break; }
  const size_t lds = gauss_lds_bytes(t, radius);
  if (lds > kGaussLdsBudget) SR_FAIL(SR_ERR_INVALID, "sr_filter_gauss: no tile fits LDS at radius %d", radius);
  const dim3 grid(cdiv(W, t.tw), cdiv(H, t.th), (unsigned)B);
  if (grid.y > 65535 || grid.z > 65535) SR_FAIL(SR_ERR_INVALID, "sr_filter_gauss: grid too large");
  hipLaunchKernelGGL(gauss_kernel, grid, dim3(kThreads), lds, sr_stream(stream), src, dst, H, W, C, s4(src_strides), radius, t.th, t.tw,
                     t.cb, fastdiv((t.tw + 2 * radius) * t.cb), fastdiv(t.tw * t.cb), fastdiv(t.cb), amount, gw);
  SR_CHECK_LAUNCH("sr_filter_gauss");
  return SR_OK;
}

extern "C" int sr_mask_grow(const float* src, float* dst, float* tmp, int32_t N, int32_t H, int32_t W, const int64_t* src_strides,
                            int32_t expand, int32_t tapered, void* stream) {
  if (!src || !dst || !src_strides) SR_FAIL(SR_ERR_INVALID, "sr_mask_grow: null pointer");
  if (N < 1 || !sides_ok(H, W) || (int64_t)N * H * W >= kMaxElems) SR_FAIL(SR_ERR_INVALID, "sr_mask_grow: sizes %d x %d x %d", N, H, W);
  const bool erode = expand < 0;
  int64_t n = erode ? -(int64_t)expand : (int64_t)expand;
  if (n > (int64_t)H + W) n = (int64_t)H + W;               // the ball covers the mask from every pixel: more changes nothing
  const int passes = n == 0 ? 1 : (int)((n + SR_GROW_MAX_STEP - 1) / SR_GROW_MAX_STEP);
  if (passes > 1 && !tmp) SR_FAIL(SR_ERR_INVALID, "sr_mask_grow: %d iterations need the tmp buffer", (int)n);
  const dim3 grid(cdiv(W, kGrowTW), cdiv(H, kGrowTH), (unsigned)N);
  if (grid.y > 65535 || grid.z > 65535) SR_FAIL(SR_ERR_INVALID, "sr_mask_grow: grid too large");
  const float* cur = src;
  S3 cs = s3(src_strides);
  for (int p = 0; p < passes; ++p) {
    const int steps = (int)(n < SR_GROW_MAX_STEP ? n : SR_GROW_MAX_STEP);
    n -= steps;
    float* out = ((passes - 1 - p) % 2 == 0) ? dst : tmp;
    const size_t lds = (size_t)2 * (kGrowTH + 2 * steps) * (kGrowTW + 2 * steps) * sizeof(float);
    if (erode) hipLaunchKernelGGL(grow_kernel<true>, grid, dim3(kThreads), lds, sr_stream(stream), cur, out, H, W, cs, steps, tapered ? 0 : 1);
    else hipLaunchKernelGGL(grow_kernel<false>, grid, dim3(kThreads), lds, sr_stream(stream), cur, out, H, W, cs, steps, tapered ? 0 : 1);
    SR_CHECK_LAUNCH("sr_mask_grow");
    cur = out;
    cs = S3{(int64_t)H * W, (int64_t)W, 1};
  }
  return SR_OK;
}

extern "C" int sr_mask_feather(const float* src, float* dst, int32_t N, int32_t H, int32_t W, const int64_t* src_strides, int32_t left,
                               int32_t top, int32_t right, int32_t bottom, void* stream) {
  if (!src || !dst || !src_strides) SR_FAIL(SR_ERR_INVALID, "sr_mask_feather: null pointer");
  if (N < 1 || !sides_ok(H, W) || (int64_t)N * H * W >= kMaxElems) SR_FAIL(SR_ERR_INVALID, "sr_mask_feather: sizes %d x %d x %d", N, H, W);
  if (left < 0 || top < 0 || right < 0 || bottom < 0) SR_FAIL(SR_ERR_INVALID, "sr_mask_feather: negative width");
  left = left < W ? left : W;
  right = right < W ? right : W;
  top = top < H ? top : H;
  bottom = bottom < H ? bottom : H;
  const int64_t total = (int64_t)N * H * W;
  hipLaunchKernelGGL(feather_kernel, dim3(blocks_for(total)), dim3(kThreads), 0, sr_stream(stream), src, dst, total, H, W, s3(src_strides),
                     left, top, right, bottom);
  SR_CHECK_LAUNCH("sr_mask_feather");
  return SR_OK;
}

extern "C" int sr_composite(float* dst, const float* src, const float* mask, int32_t B, int32_t C, int32_t Hd, int32_t Wd, int32_t Bs,
                            int32_t Bm, int32_t top, int32_t left, int32_t h, int32_t w, const int64_t* dst_strides,
                            const int64_t* src_strides, const int64_t* mask_strides, void* stream) {
  if (!dst || !src || !dst_strides || !src_strides || (mask && !mask_strides)) SR_FAIL(SR_ERR_INVALID, "sr_composite: null pointer");
  if (B < 1 || C < 1 || Bs < 1 || (mask && Bm < 1) || !sides_ok(Hd, Wd)) SR_FAIL(SR_ERR_INVALID, "sr_composite: sizes");
  if (h < 0 || w < 0 || top < 0 || left < 0 || (int64_t)top + h > Hd || (int64_t)left + w > Wd)
    SR_FAIL(SR_ERR_INVALID, "sr_composite: region %d x %d at (%d, %d) leaves the %d x %d destination", h, w, top, left, Hd, Wd);
  if (h == 0 || w == 0) return SR_OK;
  const int64_t total = (int64_t)B * C * h * w;
  if (total >= kMaxElems) SR_FAIL(SR_ERR_INVALID, "sr_composite: too many elements");
  const S3 ms = mask ? s3(mask_strides) : S3{0, 0, 0};
  hipLaunchKernelGGL(composite_kernel, dim3(blocks_for(total)), dim3(kThreads), 0, sr_stream(stream), dst, src, mask, total, C, Bs,
                     mask ? Bm : 1, top, left, h, w, s4c(dst_strides), s4c(src_strides), ms, (C > 1 && dst_strides[1] == 1) ? 1 : 0);
  SR_CHECK_LAUNCH("sr_composite");
  return SR_OK;
}

extern "C" int sr_blend(const float* a, const float* b, float* dst, int32_t B, int32_t H, int32_t W, int32_t C, const int64_t* a_strides,
                        const int64_t* b_strides, double factor, int32_t mode, void* stream) {
  if (!a || !b || !dst || !a_strides || !b_strides) SR_FAIL(SR_ERR_INVALID, "sr_blend: null pointer");
  if (B < 1 || C < 1 || !sides_ok(H, W) || (int64_t)B * H * W * C >= kMaxElems) SR_FAIL(SR_ERR_INVALID, "sr_blend: sizes %d x %d x %d x %d", B, H, W, C);
  if (mode < SR_BLEND_NORMAL || mode > SR_BLEND_DIFFERENCE) SR_FAIL(SR_ERR_INVALID, "sr_blend: unknown mode %d", mode);
  if (!std::isfinite(factor)) SR_FAIL(SR_ERR_INVALID, "sr_blend: factor is not finite");
  const int64_t total = (int64_t)B * H * W * C;
  hipLaunchKernelGGL(blend_kernel, dim3(blocks_for(total)), dim3(kThreads), 0, sr_stream(stream), a, b, dst, total, H, W, C, s4(a_strides),
                     s4(b_strides), factor, mode);
  SR_CHECK_LAUNCH("sr_blend");
  return SR_OK;
}

extern "C" int sr_mask_combine(const float* dest, const float* source, float* dst, int32_t N, int32_t H, int32_t W, int32_t Ns, int32_t Hs,
                               int32_t Ws, const int64_t* dest_strides, const int64_t* source_strides, int32_t x, int32_t y, int32_t op,
                               void* stream) {
  if (!dest || !source || !dst || !dest_strides || !source_strides) SR_FAIL(SR_ERR_INVALID, "sr_mask_combine: null pointer");
  if (N < 1 || !sides_ok(H, W) || !sides_ok(Hs, Ws) || (int64_t)N * H * W >= kMaxElems) SR_FAIL(SR_ERR_INVALID, "sr_mask_combine: sizes");
  if (Ns != N && Ns != 1) SR_FAIL(SR_ERR_INVALID, "sr_mask_combine: source batch %d against destination batch %d", Ns, N);
  if (x < 0 || y < 0) SR_FAIL(SR_ERR_INVALID, "sr_mask_combine: negative offset (%d, %d)", x, y);
  if (op < SR_COMBINE_MULTIPLY || op > SR_COMBINE_XOR) SR_FAIL(SR_ERR_INVALID, "sr_mask_combine: unknown operation %d", op);
  const int64_t x1 = (int64_t)x + Ws < W ? (int64_t)x + Ws : W, y1 = (int64_t)y + Hs < H ? (int64_t)y + Hs : H;
  const int64_t total = (int64_t)N * H * W;
  hipLaunchKernelGGL(combine_kernel, dim3(blocks_for(total)), dim3(kThreads), 0, sr_stream(stream), dest, source, dst, total, H, W, Ns,
                     s3(dest_strides), s3(source_strides), x, y, (int)x1, (int)y1, op);
  SR_CHECK_LAUNCH("sr_mask_combine");
  return SR_OK;
}

extern "C" int sr_color_to_mask(const float* image, float* dst, int32_t B, int32_t H, int32_t W, const int64_t* image_strides, int32_t color,
                                void* stream) {
  if (!image || !dst || !image_strides) SR_FAIL(SR_ERR_INVALID, "sr_color_to_mask: null pointer");
  if (B < 1 || !sides_ok(H, W) || (int64_t)B * H * W >= kMaxElems) SR_FAIL(SR_ERR_INVALID, "sr_color_to_mask: sizes %d x %d x %d", B, H, W);
  const int64_t total = (int64_t)B * H * W;
  hipLaunchKernelGGL(color_kernel, dim3(blocks_for(total)), dim3(kThreads), 0, sr_stream(stream), image, dst, total, H, W, s4(image_strides),
                     color);
  SR_CHECK_LAUNCH("sr_color_to_mask");
  return SR_OK;
}
