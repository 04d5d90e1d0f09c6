/* C ABI of libsr_t2i.so (this directory, built by csrc/sidelib.py's PRIVATE_EXTRA table): the T2I-Adapter network (the reference's
 * comfy/t2i_adapter/adapter.py Adapter: PixelUnshuffle, a 3x3 convolution, eight residual blocks of 3x3 / 1x1 convolutions with ReLU,
 * three 2x downsamplings by average pooling or a stride-2 convolution) and the hand-over of its feature maps to the UNet plan's
 * control buffers.  A private ABI: only stable-renderer_amd/_t2i.py binds it (t2i_adapter.py drives it), which is why this header
 * lies next to its source and not under include/.  Conventions as in csrc/taesd/sr_taesd.h: caller-owned device pointers, `stream`
 * a hipStream_t, no allocation, no atomics and no synchronisation inside, 0 on success or a negative code with the text in
 * sr_t2i_last_error() (thread-local).  No device pointer is dereferenced on the host and nothing is launched on bad arguments.
 *
 * Activations are fp16 NHWC maps whose pixels are `ld` halves apart; a layer reads the first Cin channels of a pixel.  Weights are
 * fp16, packed by sr_t2i_packed_index's rule; the accumulation is fp32 (MFMA), the epilogue fp32, and a value is rounded once, when
 * it is stored.  No split-K: an output element is one accumulator that walks K in one order (tap-major, then input channel) in
 * every tile form, so a result depends neither on the launch order nor on the batch it is computed in. */
#ifndef SR_T2I_H
#define SR_T2I_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { SR_T2I_OK = 0, SR_T2I_ERR_INVALID = -1, SR_T2I_ERR_LAUNCH = -2 };
enum { SR_T2I_MAX_LAYERS = 256, SR_T2I_MAX_C = 1280 };

/* One convolution over B maps of H x W OUTPUT pixels (m = (b, y, x), n = output channel) read from B source maps of Hs x Ws pixels:
 *   ksize = 3 (padding 1):  acc = sum over taps (ky, kx) and c < Cin of src[b, stride y + ky - 1, stride x + kx - 1, c] * w[n, c, ky, kx]
 *                           (zeros outside the source map);  H = (Hs + stride - 1) / stride, W likewise, stride 1 or 2
 *   ksize = 1 (stride 1):   acc = sum over c < Cin of src[b, y, x, c] * w[n, c];  H = Hs, W = Ws
 *   v = acc + bias[n];   relu: v = max(v, 0);   res: v = v + res[m * ld_res + n] (fp16);   out[m * ld_out + n] = fp16(v)
 * Only the Cout channels of a pixel of `out` are written.  `res` may be `out` (an element is read and written by one thread); `src`
 * must not overlap `out`.
 * Extents: src (B Hs Ws - 1) ld_in + Cin halves (the channels at and above Cin are never read); w ksize^2 Cin Cout halves; bias Cout
 * floats; out (B H W - 1) ld_out + Cout halves; res (B H W - 1) ld_res + Cout halves.
 * Sizes: Cin and Cout multiples of 32 up to SR_T2I_MAX_C, pitches multiples of 8, all pointers 16-byte aligned, B Hs Ws ld_in and
 * B H W pitch < 2^31.
 * The tile form follows from (H, W, Cout) alone -- never from B, so an image's bits do not depend on its batch:
 *   H W >= 1024 and Cout % 64 == 0:  a wave computes 64 output channels x 64 pixels (four accumulators, each operand fragment used twice)
 *   otherwise:                       a wave computes 32 output channels x 32 pixels (the small maps take their parallelism from Cout) */
typedef struct {
  const void* src;        /* fp16 */
  const void* w;          /* fp16, packed: ksize^2 * Cin * Cout halves */
  const float* bias;      /* Cout */
  void* out;              /* fp16 */
  const void* res;        /* fp16 or null */
  int32_t B, H, W;        /* the output maps */
  int32_t Hs, Ws;         /* the source maps */
  int32_t Cin, Cout;
  int32_t ld_in, ld_out, ld_res;
  int32_t ksize;          /* 1 or 3 */
  int32_t stride;         /* 1 or 2 (2 with ksize = 3 only) */
  int32_t relu;           /* 0 or 1 */
} sr_t2i_conv;

const char* sr_t2i_last_error(void);
const char* sr_t2i_source_hash(void);                     /* hash of the sources this image was built from */

/* Where the weight w[n, c, ky, kx] of a (Cout, Cin, ksize, ksize) convolution lies in the packed array (an index in halves), or -1
 * for arguments out of range.  Fragments of 32 output channels x 16 input channels, 512 halves each, ordered
 * [ky * ksize + kx][c / 16][n / 32], and inside a fragment [(c % 16) / 8][n % 32][c % 8]: what one lane of an MFMA operand loads
 * as 16 bytes. */
int64_t sr_t2i_packed_index(int32_t Cout, int32_t Cin, int32_t ksize, int32_t n, int32_t c, int32_t ky, int32_t kx);

/* Enqueue n convolutions on one stream, in order, one launch each.  All n descriptors are checked before the first launch. */
int sr_t2i_run(const sr_t2i_conv* layers, int32_t n, void* stream);

/* AvgPool2d(2, 2) with the padding of the reference's Downsample.forward (padding = [H % 2, W % 2], the padding zeros counted):
 *   dst[b, y, x, c] = fp16((sum of src[b, 2y - ph + i, 2x - pw + j, c] over i, j in {0, 1} inside the map) / 4),  ph = H % 2, pw = W % 2
 * src (B, H, W) pixels ld_src apart, dst (B, (H+1)/2, (W+1)/2) pixels ld_dst apart, C channels (a multiple of 8) of each; fp32 sum
 * in the order (0,0), (0,1), (1,0), (1,1).  Pointers 16-byte aligned, pitches multiples of 8, B H W ld_src < 2^31. */
int sr_t2i_pool(const void* src, void* dst, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ld_src, int32_t ld_dst, void* stream);

/* The hint -> the adapter's fp16 NHWC input: channel mean (when Ca = 1 < Ch), then PixelUnshuffle(r).
 * src element (b, ch, y, x) lies at src[b sb + ch sc + y sy + x sx] (fp32, element strides >= 0: NCHW, or an IMAGE's NHWC memory),
 * b < B, ch < Ch, y < H, x < W with H and W multiples of r (8 or 16).  Ca is Ch, or 1: then the value is the mean over the Ch
 * channels, summed in fp32 in channel order and divided by Ch.  dst is (B, H / r, W / r) pixels ld_dst apart:
 *   dst[b, Y, X, c r^2 + dy r + dx] = fp16(value(b, c, Y r + dy, X r + dx)),  c < Ca;  channels Ca r^2 <= k < ld_dst are zeros.
 * ld_dst a multiple of 8, >= Ca r^2; dst 16-byte and src 4-byte aligned; B (H / r) (W / r) ld_dst < 2^31. */
int sr_t2i_unshuffle(const float* src, int64_t sb, int64_t sc, int64_t sy, int64_t sx, int32_t B, int32_t Ch, int32_t H, int32_t W,
                     int32_t Ca, int32_t r, void* dst, int32_t ld_dst, void* stream);

/* One level's feature map, times `strength`, into each of the `copies` batch replicas of a control buffer:
 *   dst[(k N + n) P + p, c] = round(strength * src[n P + p, c]),  k < copies, n < N, p < P (pixels of a map), c < C
 * src fp16 with pixels ld_src apart; dst C channels dense, fp16, or fp32 with dst_f32 = 1.  The product is formed in fp32 and
 * rounded once.  C a multiple of 8, pointers 16-byte aligned, strength finite, copies N P C < 2^31. */
int sr_t2i_emit(const void* src, int32_t ld_src, void* dst, int32_t dst_f32, int32_t N, int32_t P, int32_t C, int32_t copies,
                float strength, void* stream);

#ifdef __cplusplus
}
#endif
#endif
