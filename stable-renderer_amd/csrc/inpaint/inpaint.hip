// Masked (inpaint) sampling: the blends around a model evaluation (KSamplerX0Inpaint.forward, comfy/samplers.py:399-412, with
// DifferentialDiffusion's threshold), the input staging of a 9-channel inpaint UNet (c_concat), and VAEEncodeForInpaint's mask growth
// and pixel neutralisation (comfyUI/nodes.py:349-386).  libsr_inpaint.so, private C ABI in sr_inpaint.h; why it is a library of its
// own and a private one: csrc/sidelib.py.
//
// All of it is element-wise work on latents of a few hundred KiB (8 views x 4 x 64 x 64 fp32 = 512 KiB): one element per thread,
// coalesced 4-byte accesses, so that pointers need no more than 4-byte alignment and a mask view of any strides is read in place.
#include <cmath>
#include <cstdint>
#include "sr_inpaint.h"
#define SR_SIDE inpaint
#define SR_SIDE_UC INPAINT
#ifndef SR_INPAINT_SRC_HASH
#define SR_INPAINT_SRC_HASH "unstamped"
#endif
#include "../sr_side.h"

namespace {
// the factor of sr_eps_scale_input (csrc/eltwise.hip), formed on the host by the same expression
inline float eps_inv(float sigma) { return 1.0f / sqrtf(sigma * sigma + 1.0f); }
}  // namespace

// Bit equality with the reference needs every fp32 operation rounded on its own, and hipcc contracts a * b + c into a fused
// multiply-add by default; the pragma forbids that for the operators written below it (see csrc/morph/morph.hip).
#pragma clang fp contract(off)

namespace {

struct Mask {
  const float* p;
  int64_t sn, sy, sx;
  int32_t M, N;
  int32_t use_thr;
  float thr;
};

__device__ inline float mask_at(const Mask& m, int n, int y, int x) {
  const int nm = m.M <= m.N ? n % m.M : n;
  const float v = m.p[(int64_t)nm * m.sn + (int64_t)y * m.sy + (int64_t)x * m.sx];
  return m.use_thr ? (v >= m.thr ? 1.0f : 0.0f) : v;
}

__global__ void __launch_bounds__(256) blend_in_kernel(const float* __restrict__ x, const float* __restrict__ noise,
                                                       const float* __restrict__ latent, Mask m, int C, int h, int w, float sigma,
                                                       float* __restrict__ xm, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int xx = (int)(i % w), yy = (int)((i / w) % h), n = (int)(i / ((int64_t)w * h * C));
  const float mv = mask_at(m, n, yy, xx);
  float s = noise[i] * sigma;
  s = s + latent[i];
  const float lm = 1.0f - mv;
  const float a = x[i] * mv;
  const float b = s * lm;
  xm[i] = a + b;
}

__global__ void __launch_bounds__(256) blend_out_kernel(float* den, const float* __restrict__ latent, Mask m, int C, int h, int w,
                                                        const float* __restrict__ x, float* __restrict__ d, float sigma,
                                                        int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int xx = (int)(i % w), yy = (int)((i / w) % h), n = (int)(i / ((int64_t)w * h * C));
  const float mv = mask_at(m, n, yy, xx);
  const float lm = 1.0f - mv;
  const float a = den[i] * mv;
  const float b = latent[i] * lm;
  const float r = a + b;
  den[i] = r;
  if (d) d[i] = (x[i] - r) / sigma;                         // (correctly rounded: hipcc's default for fp32 division)
}

// i over copies * N * 4 * hw: channels 0..3 of every batch item of the (copies * N, Cin, h, w) buffer
__global__ void __launch_bounds__(256) stage_kernel(const float* __restrict__ x, float* __restrict__ xin, int64_t hw, int Cin,
                                                    int64_t per_copy, float inv, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int64_t src = i % per_copy;                          // (n, c, y, x) of x
  const int64_t b = i / (4 * hw);                            // cp * N + n
  xin[b * Cin * hw + (i % (4 * hw))] = x[src] * inv;
}

// i over copies * N * 5 * hw: channels 4..8
__global__ void __launch_bounds__(256) concat_kernel(Mask m, const float* __restrict__ clat, float* __restrict__ xin, int N, int Cin,
                                                     int h, int w, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int64_t hw = (int64_t)h * w;
  const int64_t pos = i % hw;
  const int c = (int)((i / hw) % 5);
  const int64_t b = i / (5 * hw);
  const int n = (int)(b % N);
  const float v = c == 0 ? rintf(mask_at(m, n, (int)(pos / w), (int)(pos % w))) : clat[((int64_t)n * 4 + (c - 1)) * hw + pos];
  xin[(b * Cin + 4 + c) * hw + pos] = v;
}

// rows: tmp[n, i, j] = sum of rintf(mask[n, i, b]) over j - pad <= b < j - pad + g inside the row (g == 0: out = rintf(mask))
__global__ void __launch_bounds__(256) grow_rows_kernel(Mask m, int H, int W, int g, int pad, float* __restrict__ tmp, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i % W), y = (int)((i / W) % H), n = (int)(i / ((int64_t)W * H));
  if (g == 0) {
    tmp[i] = rintf(mask_at(m, n, y, j));
    return;
  }
  const int lo = max(j - pad, 0), hi = min(j - pad + g, W);
  float s = 0.0f;
  for (int b = lo; b < hi; ++b) s = s + rintf(mask_at(m, n, y, b));
  tmp[i] = s;
}

// columns: out[n, i, j] = rintf(clamp(sum of tmp[n, a, j] over i - pad <= a < i - pad + g inside the column, 0, 1))
__global__ void __launch_bounds__(256) grow_cols_kernel(const float* __restrict__ tmp, int H, int W, int g, int pad,
                                                        float* __restrict__ out, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i % W), y = (int)((i / W) % H);
  const int64_t plane = i - (int64_t)y * W - j;
  const int lo = max(y - pad, 0), hi = min(y - pad + g, H);
  float s = 0.0f;
  for (int a = lo; a < hi; ++a) s = s + tmp[plane + (int64_t)a * W + j];
  out[i] = rintf(fminf(fmaxf(s, 0.0f), 1.0f));
}

// i over B * H * W * 3
__global__ void __launch_bounds__(256) neutralise_kernel(const float* __restrict__ p, int64_t ps_b, int64_t ps_y, int64_t ps_x, Mask m,
                                                         int H, int W, int Co, float* __restrict__ out, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % 3);
  const int64_t px = i / 3;
  const int xx = (int)(px % W), yy = (int)((px / W) % H), b = (int)(px / ((int64_t)W * H));
  const float k = 1.0f - rintf(mask_at(m, b, yy, xx));
  float v = p[(int64_t)b * ps_b + (int64_t)yy * ps_y + (int64_t)xx * ps_x + c] - 0.5f;
  v = v * k;
  out[px * Co + c] = v + 0.5f;
}

inline dim3 grid_of(int64_t total) { return dim3((unsigned)((total + 255) / 256)); }

// -> nullptr, or what is wrong with a mask argument
const char* bad_mask(const float* mask, int32_t M, int64_t sn, int64_t sy, int64_t sx) {
  if (!mask) return "null mask";
  if (M <= 0) return "mask batch M is not positive";
  if (sn < 0 || sy < 0 || sx < 0) return "negative mask stride";
  return nullptr;
}

// the launches address at most 2^31 - 1 blocks of 256 elements
inline bool too_many(int64_t total) { return total > (int64_t)0x7fffffff * 256; }

}  // namespace

#define INP_MASK_GUARD(name)                                                                            \
  do {                                                                                                  \
    if (const char* why_ = bad_mask(mask, M, ms_n, ms_y, ms_x)) SR_FAIL(SR_ERR_INVALID, name ": %s", why_); \
  } while (0)

extern "C" int sr_inp_blend_in(const float* x, const float* noise, const float* latent, const float* mask, int32_t M, int64_t ms_n,
                               int64_t ms_y, int64_t ms_x, int32_t N, int32_t C, int32_t h, int32_t w, float sigma, int32_t use_thr,
                               float thr, float* xm, void* stream) {
  if (!x || !noise || !latent || !xm) SR_FAIL(SR_ERR_INVALID, "sr_inp_blend_in: null x, noise, latent or xm");
  INP_MASK_GUARD("sr_inp_blend_in");
  if (N <= 0 || C <= 0 || h <= 0 || w <= 0) SR_FAIL(SR_ERR_INVALID, "sr_inp_blend_in: sizes (%d, %d, %d, %d) must be positive", N, C, h, w);
  if (xm == x) SR_FAIL(SR_ERR_INVALID, "sr_inp_blend_in: xm may not be x");
  const int64_t total = (int64_t)N * C * h * w;
  if (too_many(total)) SR_FAIL(SR_ERR_INVALID, "sr_inp_blend_in: %lld elements are too many", (long long)total);
  const Mask m = {mask, ms_n, ms_y, ms_x, M, N, use_thr, thr};
  hipLaunchKernelGGL(blend_in_kernel, grid_of(total), dim3(256), 0, sr_stream(stream), x, noise, latent, m, C, h, w, sigma, xm, total);
  SR_CHECK_LAUNCH("sr_inp_blend_in");
  return SR_OK;
}

extern "C" int sr_inp_blend_out(float* den, const float* latent, const float* mask, int32_t M, int64_t ms_n, int64_t ms_y, int64_t ms_x,
                                int32_t N, int32_t C, int32_t h, int32_t w, int32_t use_thr, float thr, const float* x, float* d,
                                float sigma, void* stream) {
  if (!den || !latent) SR_FAIL(SR_ERR_INVALID, "sr_inp_blend_out: null den or latent");
  INP_MASK_GUARD("sr_inp_blend_out");
  if (N <= 0 || C <= 0 || h <= 0 || w <= 0) SR_FAIL(SR_ERR_INVALID, "sr_inp_blend_out: sizes (%d, %d, %d, %d) must be positive", N, C, h, w);
  if (d && !x) SR_FAIL(SR_ERR_INVALID, "sr_inp_blend_out: d needs x");
  if (d && !(sigma > 0.0f)) SR_FAIL(SR_ERR_INVALID, "sr_inp_blend_out: d needs sigma > 0, got %g", (double)sigma);
  if (d && (d == den || d == x)) SR_FAIL(SR_ERR_INVALID, "sr_inp_blend_out: d may not be den or x");
  const int64_t total = (int64_t)N * C * h * w;
  if (too_many(total)) SR_FAIL(SR_ERR_INVALID, "sr_inp_blend_out: %lld elements are too many", (long long)total);
  const Mask m = {mask, ms_n, ms_y, ms_x, M, N, use_thr, thr};
  hipLaunchKernelGGL(blend_out_kernel, grid_of(total), dim3(256), 0, sr_stream(stream), den, latent, m, C, h, w, x, d, sigma, total);
  SR_CHECK_LAUNCH("sr_inp_blend_out");
  return SR_OK;
}

extern "C" int sr_inp_stage(const float* x, float* xin, int32_t N, int32_t Cin, int32_t h, int32_t w, int32_t copies, float sigma,
                            void* stream) {
  if (!x || !xin) SR_FAIL(SR_ERR_INVALID, "sr_inp_stage: null x or xin");
  if (N <= 0 || h <= 0 || w <= 0) SR_FAIL(SR_ERR_INVALID, "sr_inp_stage: sizes (%d, %d, %d) must be positive", N, h, w);
  if (Cin <= 4) SR_FAIL(SR_ERR_INVALID, "sr_inp_stage: Cin = %d, this entry serves inputs of more than 4 channels", Cin);
  if (copies != 1 && copies != 2) SR_FAIL(SR_ERR_INVALID, "sr_inp_stage: copies = %d is neither 1 nor 2", copies);
  const int64_t hw = (int64_t)h * w, per_copy = (int64_t)N * 4 * hw, total = per_copy * copies;
  if (too_many(total)) SR_FAIL(SR_ERR_INVALID, "sr_inp_stage: %lld elements are too many", (long long)total);
  hipLaunchKernelGGL(stage_kernel, grid_of(total), dim3(256), 0, sr_stream(stream), x, xin, hw, Cin, per_copy, eps_inv(sigma), total);
  SR_CHECK_LAUNCH("sr_inp_stage");
  return SR_OK;
}

extern "C" int sr_inp_concat(const float* mask, int32_t M, int64_t ms_n, int64_t ms_y, int64_t ms_x, const float* clat, float* xin,
                             int32_t N, int32_t Cin, int32_t h, int32_t w, int32_t copies, void* stream) {
  if (!clat || !xin) SR_FAIL(SR_ERR_INVALID, "sr_inp_concat: null clat or xin");
  INP_MASK_GUARD("sr_inp_concat");
  if (N <= 0 || h <= 0 || w <= 0) SR_FAIL(SR_ERR_INVALID, "sr_inp_concat: sizes (%d, %d, %d) must be positive", N, h, w);
  if (Cin != 9) SR_FAIL(SR_ERR_INVALID, "sr_inp_concat: Cin = %d, c_concat fills channels 4..8 of 9", Cin);
  if (copies != 1 && copies != 2) SR_FAIL(SR_ERR_INVALID, "sr_inp_concat: copies = %d is neither 1 nor 2", copies);
  const int64_t total = (int64_t)copies * N * 5 * h * w;
  if (too_many(total)) SR_FAIL(SR_ERR_INVALID, "sr_inp_concat: %lld elements are too many", (long long)total);
  const Mask m = {mask, ms_n, ms_y, ms_x, M, N, 0, 0.0f};
  hipLaunchKernelGGL(concat_kernel, grid_of(total), dim3(256), 0, sr_stream(stream), m, clat, xin, N, Cin, h, w, total);
  SR_CHECK_LAUNCH("sr_inp_concat");
  return SR_OK;
}

extern "C" int sr_inp_grow(const float* mask, int32_t M, int64_t ms_n, int64_t ms_y, int64_t ms_x, int32_t H, int32_t W, int32_t g,
                           float* tmp, float* out, void* stream) {
  if (!out) SR_FAIL(SR_ERR_INVALID, "sr_inp_grow: null out");
  INP_MASK_GUARD("sr_inp_grow");
  if (H <= 0 || W <= 0) SR_FAIL(SR_ERR_INVALID, "sr_inp_grow: sizes (%d, %d) must be positive", H, W);
  if (g < 0 || g > SR_INP_MAX_GROW) SR_FAIL(SR_ERR_INVALID, "sr_inp_grow: g = %d outside [0, %d]", g, (int)SR_INP_MAX_GROW);
  if (g > 0 && !tmp) SR_FAIL(SR_ERR_INVALID, "sr_inp_grow: null tmp");
  if (g > 0 && tmp == out) SR_FAIL(SR_ERR_INVALID, "sr_inp_grow: tmp may not be out");
  const int64_t total = (int64_t)M * H * W;
  if (too_many(total)) SR_FAIL(SR_ERR_INVALID, "sr_inp_grow: %lld elements are too many", (long long)total);
  const Mask m = {mask, ms_n, ms_y, ms_x, M, M, 0, 0.0f};
  const int pad = g / 2;                                     // ceil((g - 1) / 2) for g >= 1
  hipStream_t st = sr_stream(stream);
  hipLaunchKernelGGL(grow_rows_kernel, grid_of(total), dim3(256), 0, st, m, H, W, g, pad, g == 0 ? out : tmp, total);
  SR_CHECK_LAUNCH("sr_inp_grow (rows)");
  if (g > 0) {
    hipLaunchKernelGGL(grow_cols_kernel, grid_of(total), dim3(256), 0, st, tmp, H, W, g, pad, out, total);
    SR_CHECK_LAUNCH("sr_inp_grow (columns)");
  }
  return SR_OK;
}

extern "C" int sr_inp_neutralise(const float* p, int64_t ps_b, int64_t ps_y, int64_t ps_x, const float* mask, int32_t M, int64_t ms_n,
                                 int64_t ms_y, int64_t ms_x, int32_t B, int32_t H, int32_t W, int32_t Co, float* out, void* stream) {
  if (!p || !out) SR_FAIL(SR_ERR_INVALID, "sr_inp_neutralise: null p or out");
  INP_MASK_GUARD("sr_inp_neutralise");
  if (B <= 0 || H <= 0 || W <= 0) SR_FAIL(SR_ERR_INVALID, "sr_inp_neutralise: sizes (%d, %d, %d) must be positive", B, H, W);
  if (Co < 3) SR_FAIL(SR_ERR_INVALID, "sr_inp_neutralise: out has %d channels, an IMAGE has at least 3", Co);
  if (ps_b < 0 || ps_y < 0 || ps_x < 3) SR_FAIL(SR_ERR_INVALID, "sr_inp_neutralise: bad pixel strides");
  const int64_t total = (int64_t)B * H * W * 3;
  if (too_many(total)) SR_FAIL(SR_ERR_INVALID, "sr_inp_neutralise: %lld elements are too many", (long long)total);
  const Mask m = {mask, ms_n, ms_y, ms_x, M, B, 0, 0.0f};
  hipLaunchKernelGGL(neutralise_kernel, grid_of(total), dim3(256), 0, sr_stream(stream), p, ps_b, ps_y, ps_x, m, H, W, Co, out, total);
  SR_CHECK_LAUNCH("sr_inp_neutralise");
  return SR_OK;
}
