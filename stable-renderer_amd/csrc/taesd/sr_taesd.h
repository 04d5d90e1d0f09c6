/* C ABI of libsr_taesd.so (this directory, built by csrc/sidelib.py's PRIVATE_EXTRA table): the 3x3 convolution of the TAESD tiny
 * autoencoder (the reference's comfy/taesd/taesd.py: 3x3 convolutions at 64 channels, ReLU, residual adds, nearest x2 upsampling in
 * the decoder, stride-2 convolutions in the encoder) and the packing of its input.  A private ABI: only
 * stable-renderer_amd/_taesd.py binds it (taesd.py drives it), which is why this header lies next to its source and not under
 * include/.  Conventions as in csrc/esrgan/sr_esrgan.h: caller-owned device pointers, `stream` a hipStream_t, no allocation, no
 * atomics and no synchronisation inside (the entry points can be captured into a graph), 0 on success or a negative code with the
 * text in sr_taesd_last_error() (thread-local).  No device pointer is dereferenced on the host and nothing is launched on bad
 * arguments.
 *
 * Activations are fp16 NHWC maps whose pixels are `ld` halves apart; a layer reads the first Cin channels of a pixel and writes a
 * slice of Cout channels.  Weights are fp16, packed by sr_tae_packed_index's rule; the accumulation is fp32 (MFMA), the epilogue
 * fp32, and a value is rounded once, when it is stored.  No split-K: a result does not depend on the launch order, two runs give
 * the same bits. */
#ifndef SR_TAESD_H
#define SR_TAESD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { SR_TAESD_OK = 0, SR_TAESD_ERR_INVALID = -1, SR_TAESD_ERR_LAUNCH = -2 };
enum { SR_TAE_MAX_LAYERS = 256 };

/* One 3x3 convolution, padding 1, over B maps of H x W OUTPUT pixels (m = (b, y, x), n = output channel) read from B source maps of
 * Hs x Ws pixels:
 *   acc = sum over taps (ky, kx) and c < Cin of  src[b, sy, sx, c] * w[n, c, ky, kx]                 (zeros outside the source map)
 *     stride = 1, up = 1:  (sy, sx) = (y + ky - 1, x + kx - 1);                  Hs = H, Ws = W
 *     stride = 1, up = 2:  (sy, sx) = ((y + ky - 1) >> 1, (x + kx - 1) >> 1), zeros where y + ky - 1 or x + kx - 1 leaves [0, H) x
 *                          [0, W): nearest-neighbour x2 upsampling fused into the read;  H = 2 Hs, W = 2 Ws
 *     stride = 2, up = 1:  (sy, sx) = (2 y + ky - 1, 2 x + kx - 1);              Hs = 2 H, Ws = 2 W (an even source only)
 *   v = acc + bias[n]                            (a layer without bias passes zeros)
 *   relu:        v = max(v, 0)
 *   res:         v = v + res[m * ld_res + n]     (fp16)
 *   relu_after:  v = max(v, 0)
 *   out[m * ld_out + c_off + n] = fp16(v); or, where out_f32 is given (out is ignored), for n < n_store
 *   out_f32[b ob + y oy + x ox + n oc] = clamp ? min(max(a v, 0), 1) : a v              (element strides, all >= 1)
 * Nothing outside the channel slice [c_off, c_off + Cout) of `out`, or outside the n_store channels of out_f32, is written.  `res`
 * may be the buffer and slice `out` points into (an element is read and written by one thread); `src` must not overlap the output.
 * Extents: src (B Hs Ws - 1) ld_in + Cin halves (the channels at and above Cin are never read); w 9 Cin Cout halves; bias Cout
 * floats; out (B H W - 1) ld_out + c_off + Cout halves; res (B H W - 1) ld_res + Cout halves; out_f32 up to the element
 * (B-1) ob + (H-1) oy + (W-1) ox + (n_store-1) oc.
 * Sizes: Cin and Cout 32 or 64, all pitches and c_off multiples of 8, src / w / bias / out / res 16-byte aligned, out_f32 4-byte
 * aligned, B <= 65535, B * Hs * Ws * ld_in and B * H * W * pitch < 2^31 for every pitch. */
typedef struct {
  const void* src;        /* fp16 */
  const void* w;          /* fp16, packed: 9 * Cin * Cout halves */
  const float* bias;      /* Cout */
  void* out;              /* fp16, or null with out_f32 */
  float* out_f32;         /* or null */
  const void* res;        /* fp16 or null */
  int64_t ob, oy, ox, oc; /* with out_f32: element strides of (b, y, x, n) */
  int32_t B, H, W;        /* the output maps */
  int32_t Hs, Ws;         /* the source maps */
  int32_t Cin, Cout;
  int32_t ld_in, ld_out, c_off, ld_res;
  int32_t up;             /* 1 or 2 */
  int32_t stride;         /* 1 or 2; not 2 together with up = 2 */
  int32_t relu, relu_after;   /* 0 or 1 */
  int32_t n_store;        /* with out_f32: 1..Cout */
  int32_t clamp;          /* with out_f32: 0 or 1 */
  float a;                /* with out_f32: the scale (finite) */
} sr_tae_conv;

const char* sr_taesd_last_error(void);
const char* sr_taesd_source_hash(void);                     /* hash of the sources this image was built from */

/* Where the weight w[n, c, ky, kx] of a (Cout, Cin, 3, 3) convolution lies in the packed array (an index in halves), or -1 for
 * arguments out of range.  Fragments of 32 output channels x 16 input channels, 512 halves each, ordered [c / 32][ky * 3 + kx]
 * [(c % 32) / 16][n / 32], and inside a fragment [(c % 16) / 8][n % 32][c % 8]: what one lane of an MFMA operand loads as 16 bytes. */
int64_t sr_tae_packed_index(int32_t Cout, int32_t Cin, int32_t n, int32_t c, int32_t ky, int32_t kx);

/* Enqueue n convolutions on one stream, in order.  All n descriptors are checked before the first launch. */
int sr_tae_run(const sr_tae_conv* layers, int32_t n, void* stream);

/* Strided fp32 -> the network's fp16 NHWC input.  src element (b, y, x, c) lies at src[b sb + y sy + x sx + c sc] (element strides
 * >= 0: an NCHW latent, a cropped window of an NHWC image), b < B, y < H, x < W, c < C; the last element read is
 * (B-1) sb + (H-1) sy + (W-1) sx + (C-1) sc.  dst is (B, H, W, ld_dst) halves, 16-byte aligned, ld_dst a multiple of 8 and >= C:
 *   dst[b, y, x, c] = fp16(t),  t = src[..] * a,  and with clamp3 = 1  t = 3 tanh(src[..] * a / 3)  (the decoder's Clamp())
 * for c < C and zeros for C <= c < ld_dst.  B * H * W * ld_dst < 2^31. */
int sr_tae_pack_input(const float* src, int64_t sb, int64_t sy, int64_t sx, int64_t sc, int32_t B, int32_t H, int32_t W, int32_t C,
                      float a, int32_t clamp3, void* dst, int32_t ld_dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif
