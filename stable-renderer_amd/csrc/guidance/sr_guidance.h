/* C ABI of libsr_guidance.so (this directory, built by csrc/sidelib.py's PRIVATE_EXTRA table): what a MODEL's two sampling hooks
 * compute around the UNet.  `model_sampling` decides how a model output becomes a denoised latent (EPS, V_PREDICTION, EDM of
 * comfy/model_sampling.py:7-38, LCM and X0 of comfy_extras/nodes_model_advanced.py:7-23); `sampler_cfg_function` replaces plain
 * classifier-free guidance (comfy/samplers.py:346-351), here by RescaleCFG (nodes_model_advanced.py:185-206).  A private ABI: only
 * stable-renderer_amd/_guidance.py binds it.  Conventions as in csrc/inpaint/sr_inpaint.h: caller-owned device pointers, `stream` a
 * hipStream_t, no allocation, no atomics and no synchronisation inside, 0 on success or a negative code with the text in
 * sr_guidance_last_error() (thread-local).  Every argument is validated before anything is launched; no device pointer is
 * dereferenced on the host.  Two runs give the same bits.
 *
 * Latents are contiguous fp32 (N, C, h, w) and need only 4-byte alignment.
 *
 * Arithmetic: every fp32 operation is rounded on its own (nothing is contracted into a fused multiply-add; division and square
 * root are correctly rounded), in the order written below, so the element-wise results are bit-equal to the torch expressions they
 * restate.  With s = sigma, sd = sigma_data, q = s*s + sd*sd, out the model output and x the model input:
 *   SR_GD_EPS  x - out*s
 *   SR_GD_V    (x*(sd*sd))/q - ((out*s)*sd)/sqrt(q)
 *   SR_GD_EDM  (x*(sd*sd))/q + ((out*s)*sd)/sqrt(q)
 *   SR_GD_X0   out
 *   SR_GD_LCM  c_out*(x - out*s) + c_skip*x,  st = timestep*10, c_skip = 0.25/(st*st + 0.25), c_out = st/sqrt(st*st + 0.25)
 * `timestep` is read by SR_GD_LCM alone (the integer ModelSamplingDiscreteDistilled.timestep(sigma) as a float), sigma_data by
 * SR_GD_V and SR_GD_EDM alone.
 *
 * contract (0 | 1) of sr_gd_denoise, sr_gd_accumulate and sr_gd_cfg: 0 is the arithmetic above.  1 forms SR_GD_EPS's x - out*s and
 * sr_gd_cfg's u + (c - u)*cfg as ONE fused multiply-add each (the product is not rounded), which is how sr_cfg_denoise,
 * sr_cond_accumulate and sr_cfg_combine of libsr_hip.so are compiled: the results are then those kernels' bits, not torch's.  An
 * eps model sampling is the reference's no-op patch; the runner asks for 1 there so that it is a no-op here as well.  1 with another
 * parameterisation is refused. */
#ifndef SR_GUIDANCE_H
#define SR_GUIDANCE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { SR_GUIDANCE_OK = 0, SR_GUIDANCE_ERR_INVALID = -1, SR_GUIDANCE_ERR_LAUNCH = -2 };
enum { SR_GD_EPS = 0, SR_GD_V = 1, SR_GD_EDM = 2, SR_GD_X0 = 3, SR_GD_LCM = 4 };

const char* sr_guidance_last_error(void);
const char* sr_guidance_source_hash(void);                  /* hash of the sources this image was built from */

/* The plain path.  out is the model output of the [uncond | cond] batch, (copies * N, C, h, w), copies 1 | 2:
 *   copies == 2   den_u = param(x, out[:N]), den_c = param(x, out[N:])
 *   copies == 1   den_c = param(x, out); den_u is not touched and may be NULL
 * den_u and den_c may not overlap x, out or each other. */
int sr_gd_denoise(const float* x, const float* out, float* den_u, float* den_c, int32_t N, int32_t C, int32_t h, int32_t w,
                  int32_t copies, int32_t param, int32_t contract, float sigma, float sigma_data, float timestep, void* stream);

/* The general conditioning path: sr_cond_accumulate (include/sr_hip.h) with param() in place of x - eps*sigma.  For the chunks j
 * of one model call on the area (ah, aw) at (y0, x0) of the latent, in batch order:
 *   den = param(x[area], out_j);  t = den * mult_j;  out_kind[area] = out_kind[area] + t;  cnt_kind[area] = cnt_kind[area] + mult_j
 * kind = kinds[j] (0 cond, otherwise uncond; int32 on the device).  out and mult are (chunks, N, C, ah, aw); x and the four
 * accumulators (N, C, h, w); nothing outside the area is read or written. */
int sr_gd_accumulate(const float* x, const float* out, const float* mult, const int32_t* kinds, float* out_c, float* cnt_c,
                     float* out_u, float* cnt_u, int32_t N, int32_t C, int32_t h, int32_t w, int32_t ah, int32_t aw, int32_t y0,
                     int32_t x0, int32_t chunks, int32_t param, int32_t contract, float sigma, float sigma_data, float timestep,
                     void* stream);

/* Plain classifier-free guidance.  c = a_c (cnt_c == NULL) or a_c / cnt_c, u likewise from a_u, cnt_u; a_u == NULL stands for
 * u = 0 (the reference skips the uncond evaluation at cfg 1 and the sums stay 0).  cnt_c and cnt_u are given both or neither.
 *   den = u + (c - u)*cfg;  d = (x - den) / sigma when d != NULL (x is then required and sigma must be > 0)
 * den may be a_c or a_u; d may not overlap anything else. */
int sr_gd_cfg(const float* a_c, const float* cnt_c, const float* a_u, const float* cnt_u, const float* x, float* den, float* d,
              int32_t N, int32_t C, int32_t h, int32_t w, float sigma, float cfg, int32_t contract, void* stream);

/* RescaleCFG: rescale_cfg (nodes_model_advanced.py:185-206) on cond = x - c, uncond = x - u, then den = x - result
 * (samplers.py:347-349).  c and u as in sr_gd_cfg.  With s = sigma, r = sqrt(s*s + 1):
 *   xs = x / (s*s + 1);  vc = ((xs - (x - (x - c)))*r)/s;  vu likewise from u;  g = vu + cfg*(vc - vu)
 *   ro_pos, ro_cfg = the unbiased standard deviations of vc and of g over the C*h*w elements of each sample
 *   f = multiplier*(g*(ro_pos/ro_cfg)) + one_minus*g;  den = x - (x - (xs - (f*s)/r));  d = (x - den)/s when d != NULL
 * one_minus is 1.0 - multiplier formed in double by the caller, as the reference's Python forms it.
 * Two launches on the stream, nothing returns to the host between them.  The first, one workgroup per sample, sums (v - v0) and
 * (v - v0)^2 in double for v = vc and v = g, v0 the sample's first element, each thread over a fixed stride and the workgroup
 * through a fixed tree in LDS, into ws: (N, 4) doubles, 8-byte aligned.  The second forms
 * ro = (float)sqrt(max(0, (sum2 - sum*sum/n)/(n - 1))) and applies it; ro_pos/ro_cfg is one fp32 division, so a sample whose g is
 * constant gets the reference's inf / nan.  den may be a_c or a_u; d and ws may not overlap anything else. */
int sr_gd_rescale(const float* a_c, const float* cnt_c, const float* a_u, const float* cnt_u, const float* x, float* den, float* d,
                  double* ws, int32_t N, int32_t C, int32_t h, int32_t w, float sigma, float cfg, float multiplier, float one_minus,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif
