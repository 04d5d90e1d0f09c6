/* C ABI of libsr_esrgan.so (this directory, built by csrc/sidelib.py's PRIVATE_MODELS table): the 3x3 convolution of the ESRGAN
 * (RRDBNet) upscale models and the packing of their input.  A private ABI: only stable-renderer_amd/_esrgan.py binds it (esrgan.py
 * drives it), which is why this header lies next to its source and not under include/.  Conventions as in include/sr_imgproc.h:
 * caller-owned device pointers, `stream` a hipStream_t, no allocation, no atomics and no synchronisation inside (the entry points
 * can be captured into a graph), 0 on success or a negative code with the text in sr_esrgan_last_error() (thread-local).  No device
 * pointer is dereferenced on the host and nothing is launched on bad arguments.
 *
 * Activations are fp16 NHWC maps whose pixel rows are `ld` halves apart; a layer reads the first Cin channels of a pixel and writes a
 * slice of Cout channels, so a dense block's concatenation is a matter of where its convolutions write.  Weights are fp16, packed
 * by sr_esr_packed_index's rule; the accumulation is fp32 (MFMA), the epilogue fp32, and a value is rounded to fp16 once, when it is
 * stored.  No split-K: a result does not depend on the launch order, two runs give the same bits. */
#ifndef SR_ESRGAN_H
#define SR_ESRGAN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { SR_ESRGAN_OK = 0, SR_ESRGAN_ERR_INVALID = -1, SR_ESRGAN_ERR_LAUNCH = -2 };
enum { SR_ESR_MAX_LAYERS = 4096 };

/* One 3x3 convolution, padding 1, stride 1, over B maps of H x W output pixels (m = (b, y, x), n = output channel):
 *   v = bias[n] + sum over taps (ky, kx) and c < Cin of  src[b, y + ky - 1, x + kx - 1, c] * w[n, c, ky, kx]      (zeros outside the map)
 *   lrelu:    v = v < 0 ? 0.2f * v : v
 *   r1:       v = v * s1 + r1[m * ld_r1 + n]       then       r2:   v = v * s2 + r2[m * ld_r2 + n]          (fp32, in this order)
 *   out[m * ld_out + c_off + n] = fp16(v), and the same to out2[m * ld_out2 + n] where out2 is given; or, where out_f32 is given,
 *   only out_f32[m * n_store + n] = v for n < n_store (out and out2 are ignored).
 * up = 2: `src` is the (H/2, W/2) map and the pixel (y, x) is read at (y >> 1, x >> 1): nearest-neighbour upsampling fused into the
 * read; H and W are even.  Nothing outside the channel slice [c_off, c_off + Cout) of `out` is written.  `src` may be the buffer
 * `out` points into as long as the slice lies at or above Cin; r1 / r2 may alias out2 (an element is read and written by one thread).
 * Sizes: Cin a multiple of 32, Cout 32 or 64, all pitches and c_off multiples of 8, pointers 16-byte aligned,
 * B * H * W * pitch < 2^31 for every pitch. */
typedef struct {
  const void* src;        /* fp16 */
  const void* w;          /* fp16, packed: 9 * Cin * Cout halves */
  const float* bias;      /* Cout */
  void* out;              /* fp16 */
  void* out2;             /* fp16 or null */
  float* out_f32;         /* or null */
  const void* r1;         /* fp16 or null */
  const void* r2;         /* fp16 or null; only with r1 */
  int32_t B, H, W;
  int32_t Cin, Cout;
  int32_t ld_in, ld_out, c_off, ld_out2;
  int32_t ld_r1, ld_r2;
  int32_t up;             /* 1 or 2 */
  int32_t lrelu;          /* 0 or 1 */
  int32_t n_store;        /* with out_f32: 1..Cout */
  float s1, s2;
} sr_esr_conv;

const char* sr_esrgan_last_error(void);
const char* sr_esrgan_source_hash(void);                    /* hash of the sources this image was built from */

/* Where the weight w[n, c, ky, kx] of a (Cout, Cin, 3, 3) convolution lies in the packed array (an index in halves), or -1 for
 * arguments out of range.  Fragments of 32 output channels x 16 input channels, 512 halves each, ordered [c / 32][ky * 3 + kx]
 * [(c % 32) / 16][n / 32], and inside a fragment [(c % 16) / 8][n % 32][c % 8]: what one lane of an MFMA operand loads as 16 bytes. */
int64_t sr_esr_packed_index(int32_t Cout, int32_t Cin, int32_t n, int32_t c, int32_t ky, int32_t kx);

/* Enqueue n convolutions on one stream, in order.  All n descriptors are checked before the first launch. */
int sr_esr_run(const sr_esr_conv* layers, int32_t n, void* stream);

/* fp32 image window -> the network's fp16 NHWC input.  src element (b, y, x, c) lies at src[b sb + y sy + x sx + c sc] (element
 * strides >= 0: a window of an NHWC IMAGE is a pointer offset, an NCHW tensor other strides), b < B, y < h, x < w, c < C.
 * shuffle s in {1, 2, 4}: the window is reflect-padded on the right and the bottom to multiples of s (hp, wp) and pixel-unshuffled:
 * dst is (B, hp / s, wp / s, ld_dst) with dst[.., c * s * s + dy * s + dx] = padded[b, y * s + dy, x * s + dx, c] and zeros in the
 * channels from C * s * s up to ld_dst.  The padding of a side is smaller than that side. */
int sr_esr_pack_input(const float* src, int64_t sb, int64_t sy, int64_t sx, int64_t sc, int32_t B, int32_t h, int32_t w, int32_t C,
                      int32_t shuffle, void* dst, int32_t ld_dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif
