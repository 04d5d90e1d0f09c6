/* C ABI of libsr_resample.so (stable-renderer_amd/csrc/resample/, built by csrc/sidelib.py): comfy.utils.common_upscale (comfyUI/comfy/utils.py:418-443) --
 * torch.nn.functional.interpolate in five modes, bislerp (utils.py:335-409) and the 8-bit Lanczos of utils.py:411-416.  Same conventions
 * as include/sr_hip.h and include/sr_tiled.h: caller-owned device pointers, `stream` a hipStream_t, no allocation, no atomics and no
 * synchronisation inside (every entry point can be captured into a graph), 0 on success or a negative code with the text in
 * sr_resample_last_error() (thread-local).
 * Alignment and extents: a pointer needs only the natural alignment of its element type (1 byte for tmp_u8, 4 for fp32 / int32, 8 for
 * fp64); 16-byte accesses are used only where the library finds the pointer and every row start 16-byte aligned.  Every tensor is
 * exactly as long as its stated shape (a strided one ends at its last element) and nothing outside it is read or written;
 * temporaries need no initialisation. */
#ifndef SR_RESAMPLE_H
#define SR_RESAMPLE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { SR_RESAMPLE_OK = 0, SR_RESAMPLE_ERR_INVALID = -1, SR_RESAMPLE_ERR_LAUNCH = -2 };
/* the `mode` strings of F.interpolate that common_upscale passes through (utils.py:443) */
enum { SR_RESAMPLE_NEAREST_EXACT = 0, SR_RESAMPLE_NEAREST = 1, SR_RESAMPLE_BILINEAR = 2, SR_RESAMPLE_BICUBIC = 3, SR_RESAMPLE_AREA = 4 };

const char* sr_resample_last_error(void);
const char* sr_resample_source_hash(void);                  /* hash of the sources this image was built from */

/* F.interpolate(src, size=(Ho, Wo), mode=...) (utils.py:443), fp32 -> fp32, both axes in one launch.  `src_strides` / `dst_strides`:
 * HOST arrays of the four element strides of (n, c, y, x), so a centre crop (utils.py:419-436) is a pointer offset and an
 * image.movedim(-1, 1) view (comfyUI/nodes.py:1750, :1774) is resampled where it lies.  Per axis, o -> input index:
 *   nearest-exact  i = min(floor((o + .5) in / out), in - 1)
 *   nearest        i = min(floor(o in / out), in - 1)
 *   bilinear       s = max((o + .5) in / out - .5, 0); i0 = min(floor(s), in - 1), i1 = min(i0 + 1, in - 1), weights 1 - (s - i0), s - i0
 *   bicubic        s = (o + .5) in / out - .5 (not clamped), f = floor(s), t = s - f; taps clamp(f - 1 + k, 0, in - 1), k = 0..3,
 *                  weights c2(t + 1), c1(t), c1(1 - t), c2(2 - t), A = -0.75 (align_corners False, no antialias, as the reference)
 *   area           mean over [floor(o in / out), ceil((o + 1) in / out))  (= adaptive_avg_pool2d)
 * Positions and weights are formed in double and the taps are summed in double, so an output is the exact value rounded once. */
int sr_resample(const float* src, float* dst, int32_t N, int32_t C, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                const int64_t* src_strides, const int64_t* dst_strides, int32_t mode, void* stream);

/* bislerp (utils.py:335-409): slerp of the C-vectors of two pixels along W into tmp (N, C, Hi, Wo; fp64, contiguous), then along H
 * into dst (N, C, Ho, Wo; fp32, contiguous).  src is fp32 with HOST element strides of (n, c, y, x).  The DEVICE tables x_ratio (fp32),
 * x_idx1, x_idx2 (int32), Wo entries each, and y_* with Ho entries, are generate_bilinear_data's (utils.py:367-377) ratios, coords_1
 * and coords_2; indices outside the axis are clamped into it.  slerp (utils.py:336-365): a normalised vector is 0 where its norm
 * is 0; dot > 1 - 1e-5 gives b1; dot < 1e-5 - 1 gives b1 (1 - r) + b2 r.  The norms, acos and the three sines are taken once per
 * pixel, in double. */
int sr_bislerp(const float* src, float* dst, double* tmp, int32_t N, int32_t C, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
               const int64_t* src_strides, const float* x_ratio, const int32_t* x_idx1, const int32_t* x_idx2, const float* y_ratio,
               const int32_t* y_idx1, const int32_t* y_idx2, void* stream);

/* lanczos (utils.py:411-416): q = uint8(clip(255.f * x, 0, 255)), PIL's 8-bit Image.resize(LANCZOS) -- a horizontal pass into tmp_u8
 * (N, Hi, Wo, 3 bytes) and a vertical pass, each clip((2^21 + sum q * k) >> 22, 0, 255) -- and / 255.f.  RGB only.  src and dst are
 * fp32 with HOST element strides of (n, c, y, x).  Per axis the DEVICE tables are `bounds` (int32 pairs: first tap, tap count, per
 * output index) and `k` (int32, `ksize` per output index); first tap and count are clamped into the axis.  A pass whose size does
 * not change is skipped, as PIL skips it: its tables may then be NULL, and tmp_u8 is needed only when both passes run. */
int sr_lanczos_rgb8(const float* src, float* dst, uint8_t* tmp_u8, int32_t N, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                    const int64_t* src_strides, const int64_t* dst_strides, const int32_t* x_bounds, const int32_t* x_k, int32_t x_ksize,
                    const int32_t* y_bounds, const int32_t* y_k, int32_t y_ksize, void* stream);

#ifdef __cplusplus
}
#endif
#endif
