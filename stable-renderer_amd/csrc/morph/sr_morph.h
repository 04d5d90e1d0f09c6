/* C ABI of libsr_morph.so (this directory, built by csrc/sidelib.py's PRIVATE_NODES table): the k x k box maximum / minimum behind
 * the Morphology node and the 18 Porter-Duff modes behind PorterDuffImageComposite.  A private ABI: only
 * stable-renderer_amd/_morph.py binds it (morph.py drives it), which is why this header lies next to its source and not under
 * include/.  Conventions as in include/sr_imgproc.h: caller-owned device pointers to fp32, `stream` a hipStream_t, no allocation,
 * no atomics and no synchronisation inside (the entry points can be captured into a graph), 0 on success or a negative code with
 * the text in sr_morph_last_error() (thread-local).  No device pointer is dereferenced on the host and nothing is launched on bad
 * arguments.
 * Alignment and extents: a pointer needs only the natural alignment of its element type (4 bytes for fp32 / int32, 8 for fp64 /
 * int64); 16-byte accesses are used only where the library finds the pointer and every row start 16-byte aligned.  Every tensor is
 * exactly as long as its stated shape (a strided one ends at its last element) and nothing outside it is read or written;
 * temporaries need no initialisation. */
#ifndef SR_MORPH_H
#define SR_MORPH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { SR_MORPH_OK = 0, SR_MORPH_ERR_INVALID = -1, SR_MORPH_ERR_LAUNCH = -2 };
/* what the last pass does with its result before it stores it; each is one fp32 subtraction */
enum { SR_MORPH_EPI_NONE = 0, SR_MORPH_EPI_GRADIENT = 1, SR_MORPH_EPI_TOP_HAT = 2, SR_MORPH_EPI_BOTTOM_HAT = 3 };
enum { SR_MORPH_MAX_K = 1 << 20 };
/* the modes of sr_porter_duff, in the order of the reference's PorterDuffMode */
enum { SR_PD_ADD = 0, SR_PD_CLEAR, SR_PD_DARKEN, SR_PD_DST, SR_PD_DST_ATOP, SR_PD_DST_IN, SR_PD_DST_OUT, SR_PD_DST_OVER, SR_PD_LIGHTEN,
       SR_PD_MULTIPLY, SR_PD_OVERLAY, SR_PD_SCREEN, SR_PD_SRC, SR_PD_SRC_ATOP, SR_PD_SRC_IN, SR_PD_SRC_OUT, SR_PD_SRC_OVER, SR_PD_XOR,
       SR_PD_MODES };

const char* sr_morph_last_error(void);
const char* sr_morph_source_hash(void);                     /* hash of the sources this image was built from */

/* The k x k box maximum and minimum of an image (B,H,W,C), in two launches: a pass along x into `scratch`, a pass along y out of it.
 *   definition   at (y, x) the maximum (minimum) over the rows y - k/2 ... y + k - k/2 - 1 and the same span of columns, where every
 *                tap outside the image is -1e4f (+1e4f) and takes part; the window of an even k is asymmetric as that says.  A
 *                window that holds a NaN gives NaN.
 *   src          the element (b, y, x, c) lies at src[b strides[0] + y strides[1] + x strides[2] + c strides[3]] (element strides
 *                >= 0: an IMAGE in its NHWC memory, a crop, a permuted NCHW tensor).  Read once: one read serves both extremes.
 *   out_max,     contiguous (B,H,W,C); either may be null, not both (SR_MORPH_EPI_GRADIENT: out_max receives max - min and
 *   out_min      out_min is null).
 *   scratch      the intermediate between the passes: B H W C floats per extreme that is computed (two for both outputs and for
 *                the gradient), scratch_elems of them are there; too few is an error.  Overlaps nothing else.
 *   epilogue     SR_MORPH_EPI_NONE; _GRADIENT; _TOP_HAT: epi_src - result; _BOTTOM_HAT: result - epi_src, with epi_src an image
 *                (B,H,W,C) with element strides epi_strides (both null otherwise).  So `open` then `x - open` needs no launch of
 *                its own.
 *   work         per output and axis about log2(k) maxima in LDS (windows of doubling length, then two overlapping ones), never
 *                k taps.  In the pass along y neighbouring lanes run along the contiguous x C axis. */
int sr_morph_box(const float* src, float* out_max, float* out_min, float* scratch, int64_t scratch_elems, int B, int H, int W, int C,
                 const int64_t* strides, int k, int epilogue, const float* epi_src, const int64_t* epi_strides, void* stream);

/* porter_duff_composite of the reference (comfy_extras/nodes_compositing.py) for all 18 modes in one launch: contiguous
 * src, dst (n_pix, C) and src_alpha, dst_alpha (n_pix) -> out_image (n_pix, C), out_alpha (n_pix); a pixel's alpha is broadcast
 * over its C channels.  Every operation is a single rounded fp32 operation in the reference's order (nothing is contracted), so
 * the result equals the reference's bit for bit.  16-byte loads and stores where every pointer is 16-byte aligned, with a scalar
 * tail.  The outputs overlap no input. */
int sr_porter_duff(const float* src, const float* src_alpha, const float* dst, const float* dst_alpha, float* out_image,
                   float* out_alpha, int64_t n_pix, int C, int mode, void* stream);

#ifdef __cplusplus
}
#endif
#endif
