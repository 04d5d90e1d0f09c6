/* C ABI of libsr_compact.so (this directory, built by csrc/sidelib.py's PRIVATE_EXTRA table): the 3x3 convolution of the Real-ESRGAN
 * compact upscale models (the reference's comfy_extras/chainner_models/architecture/SRVGG.py, SRVGGNetCompact: 3x3 convolutions at up
 * to 64 channels with a per-channel PReLU, a last convolution to in_nc * s^2 channels, a pixel shuffle, and the nearest-upsampled
 * input added back) and the packing of its input.  A private ABI: only stable-renderer_amd/_compact.py binds it (compact.py drives
 * it), which is why this header lies next to its source and not under include/.  Conventions as in csrc/taesd/sr_taesd.h:
 * caller-owned device pointers, `stream` a hipStream_t, no allocation, no atomics and no synchronisation inside (the entry points can
 * be captured into a graph), 0 on success or a negative code with the text in sr_compact_last_error() (thread-local).  No device
 * pointer is dereferenced on the host and nothing is launched on bad arguments.
 *
 * Activations are fp16 NHWC maps whose pixels are `ld` halves apart; a layer reads the first Cin channels of a pixel and writes a
 * slice of Cout channels.  Weights are fp16, packed by sr_cmp_packed_index's rule; the accumulation is fp32 (MFMA), the epilogue
 * fp32, and a value is rounded once, when it is stored as fp16 (the shuffle store does not round).  No split-K: a result does not
 * depend on the launch order, two runs give the same bits. */
#ifndef SR_COMPACT_H
#define SR_COMPACT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { SR_COMPACT_OK = 0, SR_COMPACT_ERR_INVALID = -1, SR_COMPACT_ERR_LAUNCH = -2 };
enum { SR_CMP_MAX_LAYERS = 256 };

/* One 3x3 convolution, padding 1, stride 1, over B maps of H x W pixels (m = (b, y, x), n = output channel):
 *   acc = sum over taps (ky, kx) and c < Cin of  src[b, y + ky - 1, x + kx - 1, c] * w[n, c, ky, kx]      (zeros outside the map)
 *   v = acc + bias[n]                            (a layer without bias passes zeros)
 *   slope:  v = v >= 0 ? v : slope[n] * v        (PReLU: exactly this select; a slope may be negative or above 1)
 *   out[m * ld_out + c_off + n] = fp16(v); or, where out_f32 is given (out, ld_out and c_off are ignored), THE SHUFFLE STORE: for
 *   n < C s^2, with n = c s^2 + dy s + dx (c < C, dy < s, dx < s),
 *   out_f32[b ob + (y s + dy) oy + (x s + dx) ox + c oc] = v + base[b bb + y by + x bx + c bc]
 * which is PixelShuffle(s) of the layer's output plus the nearest-upsampled `base`, both in fp32: no high-resolution intermediate
 * exists.  ob, oy, ox, oc are element strides >= 1 of the (B, H s, W s, C) result, bb, by, bx, bc element strides >= 0 of the
 * (B, H, W, C) fp32 image the network was given (a window of an NHWC image, a permuted NCHW tensor); `base` is required with out_f32.
 * Nothing outside the channel slice [c_off, c_off + Cout) of `out`, or outside the C s^2 shuffled elements per pixel of out_f32, is
 * written.  `src` and `base` must not overlap the output.
 * Extents: src (B H W - 1) ld_in + Cin halves (the channels at and above Cin are never read); w 9 Cin Cout halves; bias and slope
 * Cout floats; out (B H W - 1) ld_out + c_off + Cout halves; out_f32 up to the element (B-1) ob + (H s - 1) oy + (W s - 1) ox +
 * (C-1) oc; base up to the element (B-1) bb + (H-1) by + (W-1) bx + (C-1) bc.
 * Sizes: Cin and Cout 32 or 64, all pitches and c_off multiples of 8, src / w / bias / slope / out 16-byte aligned, out_f32 and base
 * 4-byte aligned, B <= 65535, B * H * W * ld_in and B * H * W * ld_out < 2^31; s in 1..4, C in 1..4, C s^2 <= Cout. */
typedef struct {
  const void* src;        /* fp16 */
  const void* w;          /* fp16, packed: 9 * Cin * Cout halves */
  const float* bias;      /* Cout */
  const float* slope;     /* Cout, or null: no activation */
  void* out;              /* fp16, or null with out_f32 */
  float* out_f32;         /* or null */
  const float* base;      /* fp32, with out_f32 */
  int64_t ob, oy, ox, oc; /* with out_f32: element strides of the result's (b, y, x, c) */
  int64_t bb, by, bx, bc; /* with out_f32: element strides of base's (b, y, x, c) */
  int32_t B, H, W;
  int32_t Cin, Cout;
  int32_t ld_in, ld_out, c_off;
  int32_t s;              /* with out_f32: the pixel-shuffle factor, 1..4 */
  int32_t C;              /* with out_f32: the image channels, 1..4 */
} sr_cmp_conv;

const char* sr_compact_last_error(void);
const char* sr_compact_source_hash(void);                   /* hash of the sources this image was built from */

/* Where the weight w[n, c, ky, kx] of a (Cout, Cin, 3, 3) convolution lies in the packed array (an index in halves), or -1 for
 * arguments out of range.  Fragments of 32 output channels x 16 input channels, 512 halves each, ordered [c / 32][ky * 3 + kx]
 * [(c % 32) / 16][n / 32], and inside a fragment [(c % 16) / 8][n % 32][c % 8]: what one lane of an MFMA operand loads as 16 bytes. */
int64_t sr_cmp_packed_index(int32_t Cout, int32_t Cin, int32_t n, int32_t c, int32_t ky, int32_t kx);

/* Enqueue n convolutions on one stream, in order.  All n descriptors are checked before the first launch. */
int sr_cmp_run(const sr_cmp_conv* layers, int32_t n, void* stream);

/* Strided fp32 -> the network's fp16 NHWC input.  src element (b, y, x, c) lies at src[b sb + y sy + x sx + c sc] (element strides
 * >= 0: an NCHW tensor, a cropped window of an NHWC image), b < B, y < H, x < W, c < C; the last element read is
 * (B-1) sb + (H-1) sy + (W-1) sx + (C-1) sc.  dst is (B, H, W, ld_dst) halves, 16-byte aligned, ld_dst a multiple of 8 and >= C:
 *   dst[b, y, x, c] = fp16(src[..])  for c < C  and zeros for C <= c < ld_dst.  B * H * W * ld_dst < 2^31. */
int sr_cmp_pack_input(const float* src, int64_t sb, int64_t sy, int64_t sx, int64_t sc, int32_t B, int32_t H, int32_t W, int32_t C,
                      void* dst, int32_t ld_dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif
