// Model sampling and guidance around the UNet: the parameterisations of a model output (EPS, V_PREDICTION, EDM of
// comfy/model_sampling.py:7-38, LCM and X0 of comfy_extras/nodes_model_advanced.py:7-23) on the plain and on the general
// conditioning path, plain classifier-free guidance, and RescaleCFG (nodes_model_advanced.py:185-206 as comfy/samplers.py:346-349
// applies it).  libsr_guidance.so, private C ABI in sr_guidance.h; why it is a library of its own and a private one: csrc/sidelib.py.
//
// Element-wise work on latents of a few hundred KiB (8 views x 4 x 64 x 64 fp32 = 512 KiB): one element per thread, coalesced
// 4-byte accesses.  The one reduction (RescaleCFG's two standard deviations per sample) is one workgroup per sample, double sums
// through a fixed tree in LDS: no atomics, the same bits every run.
#include <cmath>
#include <cstdint>
#include "sr_guidance.h"
#define SR_SIDE guidance
#define SR_SIDE_UC GUIDANCE
#ifndef SR_GUIDANCE_SRC_HASH
#define SR_GUIDANCE_SRC_HASH "unstamped"
#endif
#include "../sr_side.h"

// Bit equality with the reference needs every fp32 operation rounded on its own, and hipcc contracts a * b + c into a fused
// multiply-add by default; the pragma forbids that for the operators written below it (see csrc/inpaint/inpaint.hip).  fp32
// division and sqrtf are correctly rounded (hipcc's default).
#pragma clang fp contract(off)

namespace {

struct Param {
  int32_t code;
  float s;                                                  // sigma
  float sd, sd2;                                            // sigma_data and its square (formed in double on the host)
  float t;                                                  // the LCM timestep
  int32_t contract;                                         // eps alone: x - out*s as ONE fused multiply-add (sr_cfg_denoise's bits)
};

// calculate_denoised of the parameterisation p.code on one element: x the model input, o the model output
__device__ inline float denoised_of(const Param& p, float x, float o) {
  switch (p.code) {
    case SR_GD_EPS: {
      if (p.contract) return fmaf(-o, p.s, x);              // as csrc/eltwise.hip is compiled: the product is not rounded
      const float a = o * p.s;
      return x - a;
    }
    case SR_GD_V:
    case SR_GD_EDM: {
      float q = p.s * p.s;
      q = q + p.sd2;
      float a = x * p.sd2;
      a = a / q;
      float b = o * p.s;
      b = b * p.sd;
      b = b / sqrtf(q);
      return p.code == SR_GD_V ? a - b : a + b;
    }
    case SR_GD_X0:
      return o;
    default: {                                              // SR_GD_LCM
      float x0 = o * p.s;
      x0 = x - x0;
      const float st = p.t * 10.0f;                         // timestep_scaling
      float q = st * st;
      q = q + 0.25f;
      const float c_skip = 0.25f / q;
      const float c_out = st / sqrtf(q);
      const float a = c_out * x0;
      const float b = c_skip * x;
      return a + b;
    }
  }
}

__global__ void __launch_bounds__(256) denoise_kernel(const float* __restrict__ x, const float* __restrict__ out, float* __restrict__ den_u,
                                                      float* __restrict__ den_c, int64_t n, int copies, Param p) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float xv = x[i];
  if (copies == 2) {
    den_u[i] = denoised_of(p, xv, out[i]);
    den_c[i] = denoised_of(p, xv, out[n + i]);
  } else {
    den_c[i] = denoised_of(p, xv, out[i]);
  }
}

// as cond_accumulate_kernel (csrc/eltwise.hip), every operation rounded: (output * mult) and then the add (samplers.py:309-312)
__global__ void __launch_bounds__(256) accumulate_kernel(const float* __restrict__ x, const float* __restrict__ out,
                                                         const float* __restrict__ mult, const int* __restrict__ kinds,
                                                         float* __restrict__ out_c, float* __restrict__ cnt_c, float* __restrict__ out_u,
                                                         float* __restrict__ cnt_u, int h, int w, int ah, int aw, int y0, int x0,
                                                         int chunks, int64_t per, Param p) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= per) return;
  const int xx = (int)(i % aw), yy = (int)((i / aw) % ah);
  const int64_t nc = i / ((int64_t)aw * ah);
  const int64_t at = (nc * h + (y0 + yy)) * w + (x0 + xx);
  const float xv = x[at];
  float oc = out_c[at], cc = cnt_c[at], ou = out_u[at], cu = cnt_u[at];
  for (int j = 0; j < chunks; ++j) {
    const float den = denoised_of(p, xv, out[(int64_t)j * per + i]);
    const float m = mult[(int64_t)j * per + i];
    const float t = den * m;
    if (kinds[j] == 0) { oc = oc + t; cc = cc + m; } else { ou = ou + t; cu = cu + m; }
  }
  out_c[at] = oc; cnt_c[at] = cc; out_u[at] = ou; cnt_u[at] = cu;
}

struct Pair {
  const float *a_c, *cnt_c, *a_u, *cnt_u;
};

__device__ inline void load_pair(const Pair& q, int64_t i, float& c, float& u) {
  c = q.a_c[i];
  u = q.a_u ? q.a_u[i] : 0.0f;
  if (q.cnt_c) {
    c = c / q.cnt_c[i];
    if (q.a_u) u = u / q.cnt_u[i];
  }
}

__global__ void __launch_bounds__(256) cfg_kernel(Pair q, const float* x, float* den, float* __restrict__ d, int64_t n, float sigma,
                                                  float cfg, int contract) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float c, u;
  load_pair(q, i, c, u);
  float r = c - u;
  if (contract) {
    r = fmaf(r, cfg, u);                                    // sr_cfg_denoise / sr_cfg_combine: one rounding
  } else {
    r = r * cfg;
    r = u + r;
  }
  den[i] = r;
  if (d) d[i] = (x[i] - r) / sigma;
}

struct Rescale {
  float s, q, r;                                            // sigma, sigma*sigma + 1, sqrt of that
  float cfg, mul, om;
};

// -> xs = x / (s*s + 1), vc (cond in v-space), g (x_cfg)
__device__ inline void rescale_vg(const Rescale& k, float xo, float c, float u, float& xs, float& vc, float& g) {
  xs = xo / k.q;
  float ec = xo - c;                                        // args["cond"] = x - cond_pred
  ec = xo - ec;
  ec = xs - ec;
  ec = ec * k.r;
  vc = ec / k.s;
  float eu = xo - u;
  eu = xo - eu;
  eu = xs - eu;
  eu = eu * k.r;
  const float vu = eu / k.s;
  float t = vc - vu;
  t = k.cfg * t;
  g = vu + t;
}

// one workgroup per sample: ws[n] = { sum(vc - vc0), sum((vc - vc0)^2), sum(g - g0), sum((g - g0)^2) }, vc0 / g0 the sample's first
__global__ void __launch_bounds__(256) rescale_stats_kernel(Pair q, const float* __restrict__ x, double* __restrict__ ws, int64_t per,
                                                            Rescale k) {
  __shared__ double sh[4][256];
  const int64_t base = (int64_t)blockIdx.x * per;
  float c, u, xs, vc0, g0;
  load_pair(q, base, c, u);
  rescale_vg(k, x[base], c, u, xs, vc0, g0);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int64_t j = threadIdx.x; j < per; j += 256) {
    float vc, g;
    load_pair(q, base + j, c, u);
    rescale_vg(k, x[base + j], c, u, xs, vc, g);
    const double a = (double)vc - (double)vc0, b = (double)g - (double)g0;
    s0 = s0 + a;
    s1 = s1 + a * a;
    s2 = s2 + b;
    s3 = s3 + b * b;
  }
  sh[0][threadIdx.x] = s0; sh[1][threadIdx.x] = s1; sh[2][threadIdx.x] = s2; sh[3][threadIdx.x] = s3;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half)
      for (int m = 0; m < 4; ++m) sh[m][threadIdx.x] = sh[m][threadIdx.x] + sh[m][threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x < 4) ws[(int64_t)blockIdx.x * 4 + threadIdx.x] = sh[threadIdx.x][0];
}

__device__ inline float std_of(double sum, double sum2, int64_t per) {
  const double var = (sum2 - sum * sum / (double)per) / (double)(per - 1);          // per == 1: 0 / 0 = nan, as torch.std gives
  return (float)sqrt(var < 0.0 ? 0.0 : var);
}

__global__ void __launch_bounds__(256) rescale_apply_kernel(Pair q, const float* x, const double* __restrict__ ws, float* den,
                                                            float* __restrict__ d, int64_t per, int64_t n, Rescale k) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* st = ws + (i / per) * 4;
  const float ro_pos = std_of(st[0], st[1], per), ro_cfg = std_of(st[2], st[3], per);
  const float ratio = ro_pos / ro_cfg;
  float c, u, xs, vc, g;
  load_pair(q, i, c, u);
  const float xo = x[i];
  rescale_vg(k, xo, c, u, xs, vc, g);
  float f = g * ratio;
  f = k.mul * f;
  const float f2 = k.om * g;
  f = f + f2;
  f = f * k.s;
  f = f / k.r;
  f = xs - f;
  f = xo - f;                                               // rescale_cfg's return value
  const float r = xo - f;                                   // samplers.py:349
  den[i] = r;
  if (d) d[i] = (xo - r) / k.s;
}

inline dim3 grid_of(int64_t total) { return dim3((unsigned)((total + 255) / 256)); }

// the launches address at most 2^31 - 1 blocks of 256 elements
inline bool too_many(int64_t total) { return total > (int64_t)0x7fffffff * 256; }

// -> nullptr, or what is wrong with a parameterisation
const char* bad_param(int32_t param, float sigma, float sigma_data, float timestep, int32_t contract) {
  if (param < SR_GD_EPS || param > SR_GD_LCM) return "unknown parameterisation code";
  if (contract != 0 && contract != 1) return "contract is neither 0 nor 1";
  if (contract == 1 && param != SR_GD_EPS) return "contract = 1 serves SR_GD_EPS alone";
  if (!(sigma >= 0.0f) || !std::isfinite(sigma)) return "sigma is negative or not finite";
  if ((param == SR_GD_V || param == SR_GD_EDM) && !(sigma_data > 0.0f && std::isfinite(sigma_data))) return "sigma_data must be positive";
  if (param == SR_GD_LCM && !(timestep >= 0.0f && std::isfinite(timestep))) return "the LCM timestep is negative or not finite";
  return nullptr;
}

inline Param param_of(int32_t param, float sigma, float sigma_data, float timestep, int32_t contract) {
  return Param{param, sigma, sigma_data, (float)((double)sigma_data * (double)sigma_data), timestep, contract};
}

// -> nullptr, or what is wrong with the (a_c, cnt_c, a_u, cnt_u, x, den, d, sigma) arguments the two guidance entries share
const char* bad_pair(const float* a_c, const float* cnt_c, const float* a_u, const float* cnt_u, const float* x, const float* den,
                     const float* d, bool need_x, float sigma) {
  if (!a_c || !den) return "null a_c or den";
  if ((cnt_c != nullptr) != (cnt_u != nullptr)) return "cnt_c and cnt_u are given both or neither";
  if (cnt_u && !a_u) return "cnt_u without a_u";
  if ((need_x || d) && !x) return "null x";
  if (d && !(sigma > 0.0f)) return "d needs sigma > 0";
  if (d && (d == den || d == x || d == a_c || d == a_u || d == cnt_c || d == cnt_u)) return "d may not be another argument";
  if (den == x || den == cnt_c || den == cnt_u) return "den may not be x or a count";
  return nullptr;
}

}  // namespace

#define GD_SIZES_GUARD(name)                                                                                                    \
  do {                                                                                                                          \
    if (N <= 0 || C <= 0 || h <= 0 || w <= 0) SR_FAIL(SR_ERR_INVALID, name ": sizes (%d, %d, %d, %d) must be positive", N, C, h, w); \
  } while (0)

extern "C" int sr_gd_denoise(const float* x, const float* out, float* den_u, float* den_c, int32_t N, int32_t C, int32_t h, int32_t w,
                             int32_t copies, int32_t param, int32_t contract, float sigma, float sigma_data, float timestep,
                             void* stream) {
  if (!x || !out || !den_c) SR_FAIL(SR_ERR_INVALID, "sr_gd_denoise: null x, out or den_c");
  if (copies != 1 && copies != 2) SR_FAIL(SR_ERR_INVALID, "sr_gd_denoise: copies = %d is neither 1 nor 2", copies);
  if (copies == 2 && !den_u) SR_FAIL(SR_ERR_INVALID, "sr_gd_denoise: copies = 2 needs den_u");
  GD_SIZES_GUARD("sr_gd_denoise");
  if (const char* why = bad_param(param, sigma, sigma_data, timestep, contract)) SR_FAIL(SR_ERR_INVALID, "sr_gd_denoise: %s", why);
  if (den_c == x || den_c == out || den_u == x || den_u == out || den_u == den_c)
    SR_FAIL(SR_ERR_INVALID, "sr_gd_denoise: den_u and den_c may not be x, out or each other");
  const int64_t n = (int64_t)N * C * h * w;
  if (too_many(n)) SR_FAIL(SR_ERR_INVALID, "sr_gd_denoise: %lld elements are too many", (long long)n);
  hipLaunchKernelGGL(denoise_kernel, grid_of(n), dim3(256), 0, sr_stream(stream), x, out, den_u, den_c, n, copies,
                     param_of(param, sigma, sigma_data, timestep, contract));
  SR_CHECK_LAUNCH("sr_gd_denoise");
  return SR_OK;
}

extern "C" int sr_gd_accumulate(const float* x, const float* out, const float* mult, const int32_t* kinds, float* out_c, float* cnt_c,
                                float* out_u, float* cnt_u, int32_t N, int32_t C, int32_t h, int32_t w, int32_t ah, int32_t aw,
                                int32_t y0, int32_t x0, int32_t chunks, int32_t param, int32_t contract, float sigma,
                                float sigma_data, float timestep, void* stream) {
  if (!x || !out || !mult || !kinds || !out_c || !cnt_c || !out_u || !cnt_u) SR_FAIL(SR_ERR_INVALID, "sr_gd_accumulate: null argument");
  GD_SIZES_GUARD("sr_gd_accumulate");
  if (ah <= 0 || aw <= 0 || y0 < 0 || x0 < 0 || (int64_t)y0 + ah > h || (int64_t)x0 + aw > w)
    SR_FAIL(SR_ERR_INVALID, "sr_gd_accumulate: the area (%d, %d) at (%d, %d) lies outside the latent (%d, %d)", ah, aw, y0, x0, h, w);
  if (chunks <= 0) SR_FAIL(SR_ERR_INVALID, "sr_gd_accumulate: chunks = %d must be positive", chunks);
  if (const char* why = bad_param(param, sigma, sigma_data, timestep, contract)) SR_FAIL(SR_ERR_INVALID, "sr_gd_accumulate: %s", why);
  const int64_t per = (int64_t)N * C * ah * aw;
  if (too_many(per) || too_many((int64_t)N * C * h * w)) SR_FAIL(SR_ERR_INVALID, "sr_gd_accumulate: %lld elements are too many", (long long)per);
  hipLaunchKernelGGL(accumulate_kernel, grid_of(per), dim3(256), 0, sr_stream(stream), x, out, mult, kinds, out_c, cnt_c, out_u, cnt_u,
                     h, w, ah, aw, y0, x0, chunks, per, param_of(param, sigma, sigma_data, timestep, contract));
  SR_CHECK_LAUNCH("sr_gd_accumulate");
  return SR_OK;
}

extern "C" int sr_gd_cfg(const float* a_c, const float* cnt_c, const float* a_u, const float* cnt_u, const float* x, float* den,
                         float* d, int32_t N, int32_t C, int32_t h, int32_t w, float sigma, float cfg, int32_t contract, void* stream) {
  if (const char* why = bad_pair(a_c, cnt_c, a_u, cnt_u, x, den, d, false, sigma)) SR_FAIL(SR_ERR_INVALID, "sr_gd_cfg: %s", why);
  GD_SIZES_GUARD("sr_gd_cfg");
  if (contract != 0 && contract != 1) SR_FAIL(SR_ERR_INVALID, "sr_gd_cfg: contract = %d is neither 0 nor 1", contract);
  const int64_t n = (int64_t)N * C * h * w;
  if (too_many(n)) SR_FAIL(SR_ERR_INVALID, "sr_gd_cfg: %lld elements are too many", (long long)n);
  const Pair q = {a_c, cnt_c, a_u, cnt_u};
  hipLaunchKernelGGL(cfg_kernel, grid_of(n), dim3(256), 0, sr_stream(stream), q, x, den, d, n, sigma, cfg, contract);
  SR_CHECK_LAUNCH("sr_gd_cfg");
  return SR_OK;
}

extern "C" int sr_gd_rescale(const float* a_c, const float* cnt_c, const float* a_u, const float* cnt_u, const float* x, float* den,
                             float* d, double* ws, int32_t N, int32_t C, int32_t h, int32_t w, float sigma, float cfg, float multiplier,
                             float one_minus, void* stream) {
  if (const char* why = bad_pair(a_c, cnt_c, a_u, cnt_u, x, den, d, true, sigma)) SR_FAIL(SR_ERR_INVALID, "sr_gd_rescale: %s", why);
  if (!ws) SR_FAIL(SR_ERR_INVALID, "sr_gd_rescale: null ws");
  if ((uintptr_t)ws % 8 != 0) SR_FAIL(SR_ERR_INVALID, "sr_gd_rescale: ws is not 8-byte aligned");
  if ((const void*)ws == (const void*)den || (const void*)ws == (const void*)x || (const void*)ws == (const void*)d ||
      (const void*)ws == (const void*)a_c || (const void*)ws == (const void*)a_u)
    SR_FAIL(SR_ERR_INVALID, "sr_gd_rescale: ws may not be another argument");
  GD_SIZES_GUARD("sr_gd_rescale");
  if (!(sigma > 0.0f) || !std::isfinite(sigma)) SR_FAIL(SR_ERR_INVALID, "sr_gd_rescale: sigma must be positive and finite, got %g", (double)sigma);
  const int64_t per = (int64_t)C * h * w, n = per * N;
  if (too_many(n)) SR_FAIL(SR_ERR_INVALID, "sr_gd_rescale: %lld elements are too many", (long long)n);
  const Pair q = {a_c, cnt_c, a_u, cnt_u};
  Rescale k;
  k.s = sigma;
  {
    volatile float q0 = sigma * sigma;                      // (each host operation rounded to fp32 on its own)
    volatile float q1 = q0 + 1.0f;
    k.q = q1;
    k.r = sqrtf(q1);
  }
  k.cfg = cfg;
  k.mul = multiplier;
  k.om = one_minus;
  hipStream_t st = sr_stream(stream);
  hipLaunchKernelGGL(rescale_stats_kernel, dim3((unsigned)N), dim3(256), 0, st, q, x, ws, per, k);
  SR_CHECK_LAUNCH("sr_gd_rescale (statistics)");
  hipLaunchKernelGGL(rescale_apply_kernel, grid_of(n), dim3(256), 0, st, q, x, ws, den, d, per, n, k);
  SR_CHECK_LAUNCH("sr_gd_rescale (apply)");
  return SR_OK;
}
