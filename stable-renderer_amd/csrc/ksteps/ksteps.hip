// The update of a k-diffusion sampler step (comfy/k_diffusion/sampling.py: sample_euler_ancestral, sample_heun, sample_heunpp2,
// sample_dpm_2, sample_dpm_2_ancestral, sample_lms, sample_dpmpp_2s_ancestral, sample_dpmpp_2m) as one launch: a linear combination
// of up to eight fp32 tensors, summed in double and rounded once.  libsr_ksteps.so, private C ABI in sr_ksteps.h; why it is a
// library of its own and a private one: csrc/sidelib.py.
#include <cstdint>
#include "sr_ksteps.h"
#define SR_SIDE ksteps
#define SR_SIDE_UC KSTEPS
#ifndef SR_KSTEPS_SRC_HASH
#define SR_KSTEPS_SRC_HASH "unstamped"
#endif
#include "../sr_side.h"

namespace {

// the whole problem in the kernel's argument block (136 bytes): pointers and coefficients are uniform, they stay in scalar registers
struct Terms {
  const float* t[SR_KSTEPS_MAX_TERMS];
  double c[SR_KSTEPS_MAX_TERMS];
};

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// One thread owns the elements [4 g, 4 g + 4) of every group g it visits (n4 groups, all pointers 16-byte aligned) and, past the
// groups, single elements of the tail [4 n4, n).  It loads every term of its elements before it stores them, so `out` may be one of
// the terms.  n4 == 0 with a tail of n elements is the path of pointers that are only 4-byte aligned.
template <int K>
__global__ void __launch_bounds__(256) combine_kernel(float* out, Terms a, int64_t n4, int64_t n) {   // (out: not __restrict__)
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t g = tid; g < n4; g += stride) {
    float4 v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = *reinterpret_cast<const float4*>(a.t[k] + 4 * g);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      s0 = fma(a.c[k], (double)v[k].x, s0);
      s1 = fma(a.c[k], (double)v[k].y, s1);
      s2 = fma(a.c[k], (double)v[k].z, s2);
      s3 = fma(a.c[k], (double)v[k].w, s3);
    }
    *reinterpret_cast<float4*>(out + 4 * g) = make_float4((float)s0, (float)s1, (float)s2, (float)s3);
  }
  for (int64_t i = 4 * n4 + tid; i < n; i += stride) {
    float v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = a.t[k][i];
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) s = fma(a.c[k], (double)v[k], s);
    out[i] = (float)s;
  }
}

template <int K>
void launch(float* out, const Terms& a, int64_t n4, int64_t n, unsigned blocks, hipStream_t st) {
  hipLaunchKernelGGL(combine_kernel<K>, dim3(blocks), dim3(256), 0, st, out, a, n4, n);
}

}  // namespace

extern "C" int sr_ksteps_combine(float* out, int n_terms, const float* const* terms, const double* coeffs, int64_t n, void* stream) {
  if (n_terms < 1 || n_terms > SR_KSTEPS_MAX_TERMS)
    SR_FAIL(SR_ERR_INVALID, "sr_ksteps_combine: n_terms = %d outside [1, %d]", n_terms, (int)SR_KSTEPS_MAX_TERMS);
  if (n < 0) SR_FAIL(SR_ERR_INVALID, "sr_ksteps_combine: n = %lld is negative", (long long)n);
  if (!out || !terms || !coeffs) SR_FAIL(SR_ERR_INVALID, "sr_ksteps_combine: null out, terms or coeffs");
  Terms a = {};
  bool vec = al16(out);
  for (int k = 0; k < n_terms; ++k) {
    if (!terms[k]) SR_FAIL(SR_ERR_INVALID, "sr_ksteps_combine: terms[%d] is null", k);
    a.t[k] = terms[k];
    a.c[k] = coeffs[k];
    vec = vec && al16(terms[k]);
  }
  if (n == 0) return SR_OK;
  const int64_t n4 = vec ? n / 4 : 0;
  // one item per thread up to 2048 workgroups (8 per CU of a 256-CU part), grid-stride beyond
  const int64_t items = n4 > 0 ? n4 : n;
  int64_t blocks = (items + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipStream_t st = sr_stream(stream);
  switch (n_terms) {
    case 1: launch<1>(out, a, n4, n, (unsigned)blocks, st); break;
    case 2: launch<2>(out, a, n4, n, (unsigned)blocks, st); break;
    case 3: launch<3>(out, a, n4, n, (unsigned)blocks, st); break;
    case 4: launch<4>(out, a, n4, n, (unsigned)blocks, st); break;
    case 5: launch<5>(out, a, n4, n, (unsigned)blocks, st); break;
    case 6: launch<6>(out, a, n4, n, (unsigned)blocks, st); break;
    case 7: launch<7>(out, a, n4, n, (unsigned)blocks, st); break;
    default: launch<8>(out, a, n4, n, (unsigned)blocks, st); break;
  }
  SR_CHECK_LAUNCH("sr_ksteps_combine");
  return SR_OK;
}
