/* C ABI of libsr_tiled.so (stable-renderer_amd/csrc/tiled/, built by csrc/sidelib.py): the tiled VAE of comfyUI/comfy/sd.py:302-327
 * (VAE.decode_tiled_ / VAE.encode_tiled_) = three passes of comfy.utils.tiled_scale (comfyUI/comfy/utils.py:448-475), averaged.
 * Helpers around the per-tile VAE launch plans of libsr_hip.so (include/sr_hip.h); same conventions: caller-owned device
 * pointers, `stream` a hipStream_t, no allocation or synchronisation inside, 0 on success or a negative code with the text in
 * sr_tiled_last_error() (thread-local).
 * Alignment and extents: a pointer needs only the natural alignment of its element type (4 bytes for fp32 / int32, 8 for fp64 /
 * int64); 16-byte accesses are used only where the library finds the pointer and every row start 16-byte aligned.  Every tensor is
 * exactly as long as its stated shape (a strided one ends at its last element) and nothing outside it is read or written;
 * temporaries need no initialisation. */
#ifndef SR_TILED_H
#define SR_TILED_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { SR_TILED_OK = 0, SR_TILED_ERR_INVALID = -1, SR_TILED_ERR_LAUNCH = -2 };
enum { SR_TILED_F16 = 0, SR_TILED_F32 = 1 };               /* = SR_F16 / SR_F32 of sr_hip.h */

const char* sr_tiled_last_error(void);
const char* sr_tiled_source_hash(void);                     /* hash of the sources this image was built from */

/* In-place row softmax (the VAE mid attention, model.py:173-268) over the first `cols` entries of `rows` rows that are `ld` entries
 * apart (ld >= cols); entries [cols, ld) are written as 0: the zero keys a padded score matrix carries beyond cols get weight 0, not
 * exp(0 - max).  The VAE plans reach the same bits with sr_softmax_rows over all ld columns after a -inf bias on the padded columns
 * (vae.py: _Lowering.attn); this entry point serves callers that hold a padded score matrix without that bias. */
int sr_softmax_rows_ld(void* x, int32_t rows, int32_t cols, int32_t ld, int32_t dtype, void* stream);

/* All tensors below fp32.  A "plane" is one (H, W) image with `cpp` interleaved components per pixel: an NCHW tensor is B*C planes
 * of cpp = 1, an NHWC one is B planes of cpp = C.
 * sr_tile_gather: dst[p, i, j] = src[p, y0 + i, x0 + j], i < th, j < tw (s[:, :, y:y+tile_y, x:x+tile_x], utils.py:459; cpp = 1).
 * sr_tile_accumulate: acc[p, y0 + i, x0 + j, :] += tile[p, i, j, :] * m(i, j) for every plane and, once per pixel,
 *   wsum[y0 + i, x0 + j] += m(i, j) * feather^4 (utils.py:462-470).  m(i, j) = f(i, th) * f(j, tw),
 *   f(i, n) = ((i < feather) ? (i + 1) / feather : 1) * ((n - 1 - i < feather) ? (n - i) / feather : 1): all four sides are
 *   feathered and both ramps multiply where a tile is narrower than 2 * feather, as in the reference's in-place mask.  The weight sum
 *   is kept as the exact integer numerator (int64, one (H, W) map per pass); acc and wsum start zeroed; one launch adds to every
 *   element of its window exactly once: no float atomics.  The tiles of a pass overlap, so their launches go to ONE stream, in the
 *   reference's order.
 * sr_tile_finish: out = (sum over the npass <= 3 passes of acc_k / (wsum_k / feather^4)) / npass (utils.py:474, sd.py:309-313,
 *   :323-326), in the layout of acc; mode 1 then applies process_output = clamp((x + 1) / 2, 0, 1) (sd.py:224), mode 0 nothing. */
#define SR_TILE_FEATHER_MAX 4096
int sr_tile_gather(const float* src, float* dst, int32_t planes, int32_t H, int32_t W, int32_t y0, int32_t x0, int32_t th, int32_t tw,
                   void* stream);
int sr_tile_accumulate(const float* tile, float* acc, int64_t* wsum, int32_t planes, int32_t H, int32_t W, int32_t cpp, int32_t y0,
                       int32_t x0, int32_t th, int32_t tw, int32_t feather, void* stream);
int sr_tile_finish(const float* acc0, const float* acc1, const float* acc2, const int64_t* wsum0, const int64_t* wsum1,
                   const int64_t* wsum2, float* out, int32_t planes, int32_t H, int32_t W, int32_t cpp, int32_t npass, int32_t feather,
                   int32_t mode, void* stream);

#ifdef __cplusplus
}
#endif
#endif
