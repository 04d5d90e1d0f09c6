/* C ABI of libsr_ksteps.so (this directory, built by csrc/sidelib.py's PRIVATE table): the update of a k-diffusion sampler step as
 * ONE launch.  A private ABI: only stable-renderer_amd/_ksteps.py binds it (ksamplers.py drives it), which is why this header lies
 * next to its source and not under include/.  Conventions as in include/sr_imgproc.h: caller-owned device pointers to fp32,
 * `stream` a hipStream_t, no allocation, no atomics and no synchronisation inside (the entry point can be captured into a graph),
 * 0 on success or a negative code with the text in sr_ksteps_last_error() (thread-local). */
#ifndef SR_KSTEPS_H
#define SR_KSTEPS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { SR_KSTEPS_OK = 0, SR_KSTEPS_ERR_INVALID = -1, SR_KSTEPS_ERR_LAUNCH = -2 };
enum { SR_KSTEPS_MAX_TERMS = 8 };

const char* sr_ksteps_last_error(void);
const char* sr_ksteps_source_hash(void);                    /* hash of the sources this image was built from */

/* out[i] = (float) sum_{k < n_terms} coeffs[k] * terms[k][i]   for i < n
 * Every update of euler_ancestral, heun, heunpp2, dpm_2, dpm_2_ancestral, lms, dpmpp_2s_ancestral and dpmpp_2m is such a
 * combination of at most six tensors of the latent's size with coefficients the host knows (x + dt d + sigma_up noise;
 * x + dt/2 d + dt/2 d_2; (s'/s) x - expm1(-h) ((1 + 1/2r) den - (1/2r) old); x + sum_j c_j d_{i-j}).
 *   terms, coeffs  HOST arrays of n_terms entries, 1 <= n_terms <= SR_KSTEPS_MAX_TERMS.  The pointers and the coefficients travel
 *                  in the kernel's argument block: no table on the device, nothing the host waits for, and the arrays may be
 *                  reused as soon as the call returns.
 *   arithmetic     the sum is formed in double, in term order, each term entering by one fused multiply-add, and is rounded to
 *                  fp32 once: the result is the correctly rounded value of the double sum.
 *   aliasing       `out` may be exactly one of the terms (x is updated in place) or overlap none of them: a thread reads all the
 *                  terms of its elements before it writes them, and no other thread touches those elements.  An `out` that
 *                  overlaps a term at another offset is not supported.
 *   access         16-byte vector loads and stores where `out` and every term are 16-byte aligned, with a scalar tail for
 *                  n % 4 elements; pointers aligned only to 4 bytes take the scalar path for all n.  Grid-stride.
 *   n == 0         returns SR_KSTEPS_OK without a launch.
 * A null pointer (out, terms, coeffs or a terms[k]), n < 0 or n_terms out of range returns SR_KSTEPS_ERR_INVALID before any launch;
 * no device pointer is dereferenced on the host. */
int sr_ksteps_combine(float* out, int n_terms, const float* const* terms, const double* coeffs, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
