/* C ABI of libsr_inpaint.so (this directory, built by csrc/sidelib.py's PRIVATE_EXTRA table): masked (inpaint) sampling.  The two
 * blends KSamplerX0Inpaint.forward wraps around every model evaluation (comfy/samplers.py:399-412), DifferentialDiffusion's threshold
 * on the mask, the input staging of a UNet with more than four input channels (c_concat, comfy/model_base.py:93-127), and the mask
 * growth and pixel neutralisation of VAEEncodeForInpaint / InpaintModelConditioning (comfyUI/nodes.py:349-445).  A private ABI: only
 * stable-renderer_amd/_inpaint.py binds it.  Conventions as in include/sr_imgproc.h: caller-owned device pointers to fp32, `stream` a
 * hipStream_t, no allocation, no atomics and no synchronisation inside, 0 on success or a negative code with the text in
 * sr_inpaint_last_error() (thread-local).  Every argument is validated before anything is launched; no device pointer is
 * dereferenced on the host.
 *
 * Arithmetic: every fp32 operation is rounded on its own (nothing is contracted into a fused multiply-add), in the order written
 * below, so the results are bit-equal to the torch expressions they restate.
 *
 * Latents x, noise, latent, xm, den, d are contiguous (N, C, h, w) and need only 4-byte alignment.
 *
 * The mask is ONE channel, (M, 1, h, w), addressed through element strides (ms_n, ms_y, ms_x): any view, never materialised per
 * channel or per batch item.  Batch item n reads mask[n % M] when M <= N (repeat_to_batch_size) and mask[n] when M > N (its cut);
 * exactly the elements n' * ms_n + y * ms_y + x * ms_x of the mask items so selected are read.
 * use_thr != 0 replaces every mask value m by (m >= thr ? 1 : 0) first (DifferentialDiffusion, nodes_differential_diffusion.py). */
#ifndef SR_INPAINT_H
#define SR_INPAINT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { SR_INPAINT_OK = 0, SR_INPAINT_ERR_INVALID = -1, SR_INPAINT_ERR_LAUNCH = -2 };
enum { SR_INP_MAX_GROW = 64 };

const char* sr_inpaint_last_error(void);
const char* sr_inpaint_source_hash(void);                   /* hash of the sources this image was built from */

/* xm = x * m + (noise * sigma + latent) * (1 - m): noise*sigma, +latent, 1-m, the two products, their sum.
 * xm must not overlap x, noise, latent or the mask (the sampler's x survives the call). */
int sr_inp_blend_in(const float* x, const float* noise, const float* latent, const float* mask, int32_t M, int64_t ms_n, int64_t ms_y,
                    int64_t ms_x, int32_t N, int32_t C, int32_t h, int32_t w, float sigma, int32_t use_thr, float thr, float* xm,
                    void* stream);

/* den = den * m + latent * (1 - m), in place.  With d != NULL also d = (x - den) / sigma with the blended den and the sampler's
 * unblended x (k-diffusion's to_d): x is then required and sigma must be > 0.  d may not overlap den, x, latent or the mask. */
int sr_inp_blend_out(float* den, const float* latent, const float* mask, int32_t M, int64_t ms_n, int64_t ms_y, int64_t ms_x, int32_t N,
                     int32_t C, int32_t h, int32_t w, int32_t use_thr, float thr, const float* x, float* d, float sigma, void* stream);

/* xin[cp * N + n, c, :, :] = x[n, c, :, :] * (1 / sqrt(sigma^2 + 1)) for c < 4, cp < copies (1 | 2): channels 0..3 of the plan's
 * (copies * N, Cin, h, w) input, Cin > 4; the other channels are not touched.  x is (N, 4, h, w).  The factor is formed on the host
 * as sr_eps_scale_input forms it, so these channels carry its bits. */
int sr_inp_stage(const float* x, float* xin, int32_t N, int32_t Cin, int32_t h, int32_t w, int32_t copies, float sigma, void* stream);

/* c_concat of an inpaint UNet into channels 4..8 of that buffer (Cin == 9), for both copies, unscaled:
 * xin[cp * N + n, 4] = rintf(mask[n']) (half to even), xin[cp * N + n, 5 + c] = clat[n, c], clat contiguous (N, 4, h, w).
 * Channels 0..3 are not touched. */
int sr_inp_concat(const float* mask, int32_t M, int64_t ms_n, int64_t ms_y, int64_t ms_x, const float* clat, float* xin, int32_t N,
                  int32_t Cin, int32_t h, int32_t w, int32_t copies, void* stream);

/* VAEEncodeForInpaint's mask growth on a mask view (M, 1, H, W):
 *   g == 0   out = rintf(mask)
 *   g >= 1   out[i, j] = rintf(clamp(sum of rintf(mask[a, b]) over i - pad <= a < i - pad + g, j - pad <= b < j - pad + g, 0, 1)),
 *            pad = ceil((g - 1) / 2), elements outside the view counting 0: conv2d with a g x g box of ones and zero padding `pad`,
 *            cut to [:H, :W].  An even g makes the window reach one further up / left than down / right.
 * Two separable passes, g reads per output each: rows into tmp, columns into out; tmp and out are contiguous (M, H, W), tmp is
 * not used when g == 0 (it may then be NULL).  The sums are of integers below 2^24, so their order does not matter.
 * out and tmp may not overlap the mask or each other. */
int sr_inp_grow(const float* mask, int32_t M, int64_t ms_n, int64_t ms_y, int64_t ms_x, int32_t H, int32_t W, int32_t g, float* tmp,
                float* out, void* stream);

/* out[b, y, x, c] = (p[b, y, x, c] - 0.5) * (1 - rintf(mask[b', y, x])) + 0.5 for c < 3, on an IMAGE in NHWC memory.
 * p is a view of (B, H, W, >= 3) with element strides (ps_b, ps_y, ps_x) and channel stride 1; out is (B, H, W, Co) contiguous,
 * Co >= 3, and only its first three channels are written: a fourth is left alone.  out may not overlap p or the mask. */
int sr_inp_neutralise(const float* p, int64_t ps_b, int64_t ps_y, int64_t ps_x, const float* mask, int32_t M, int64_t ms_n,
                      int64_t ms_y, int64_t ms_x, int32_t B, int32_t H, int32_t W, int32_t Co, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
