/* C ABI of libsr_canny.so (this directory, built by csrc/sidelib.py's PRIVATE_EXTRA table): Canny edge detection in two definitions,
 * the integer one of cv2.Canny (behind canny.cv_canny, the ai_canny map) and the float one behind the Canny graph node.  A private
 * ABI: only stable-renderer_amd/_canny.py binds it (canny.py drives it), which is why this header lies next to its source and not
 * under include/.  Conventions as in sr_morph.h: caller-owned device pointers, `stream` a hipStream_t, no allocation, no atomics and
 * no host synchronisation inside (every entry point can be captured into a graph), 0 on success or a negative code with the text in
 * sr_canny_last_error() (thread-local).  No device pointer is dereferenced on the host and nothing is launched on bad arguments.
 * Alignment and extents: a pointer needs only the natural alignment of its element type (1 byte for the class map and uint8 images,
 * 2 for fp16, 4 for fp32 / int32).  Every tensor is exactly as long as its stated shape (a strided one ends at its last element)
 * and nothing outside it is read or written; the class map and the `changed` words need no initialisation.
 *
 * A detection is  classify (sr_canny_cv_classify or sr_canny_k_classify)  ->  sr_canny_hysteresis_round until a round reports no
 * change  ->  sr_canny_finish.  The class map between them is (B,H,W) uint8, contiguous, exactly B H W bytes: 0 none, 1 weak,
 * 2 strong.
 *
 * ---- the integer definition (cv2.Canny(img, t1, t2) with its defaults: aperture 3, L2gradient = False) --------------------------
 *   low = floor(min(t1, t2)), high = floor(max(t1, t2)) are taken by the caller; the entry point receives the two integers.
 *   gradient     per channel the 3 x 3 Sobel in integers with replicated borders,
 *                  gx = (p[y-1,x+1] + 2 p[y,x+1] + p[y+1,x+1]) - (the same at x-1)
 *                  gy = (p[y+1,x-1] + 2 p[y+1,x] + p[y+1,x+1]) - (the same at y-1)
 *   magnitude    m = |gx| + |gy|; the pixel takes (gx, gy, m) of the channel with the largest m, the first channel winning ties
 *                (alpha is a channel like any other).  The magnitude outside the image is 0.
 *   suppression  a pixel with m > low is a candidate if, with xs = |gx|, ys = |gy| << 15, t22 = xs * 13573, t67 = t22 + (xs << 16),
 *                  ys < t22:   m > m[y,x-1] and m >= m[y,x+1]
 *                  ys > t67:   m > m[y-1,x] and m >= m[y+1,x]
 *                  otherwise:  s = -1 if (gx ^ gy) < 0 else 1;  m > m[y-1,x-s] and m > m[y+1,x+s]
 *   classes      a candidate with m > high is strong, any other candidate weak.
 *   hysteresis   8-connected: a weak pixel connected to a strong one through weak pixels becomes strong.  Output 255 at the strong.
 *   The reference's 19 recorded ai_canny images are reproduced bit for bit by this statement (tests/golden/canny_cv.npz holds three).
 *   A float image (fp32 or fp16, values in [0,1]) is converted per value as (uint8)(v * 255) with the product in fp32: truncation.
 *   Deviation: the value is clamped to 0..255 first (NaN gives 0), where numpy's cast is undefined.
 *
 * ---- the float definition (kornia.filters.canny(x, low, high)[1] with its defaults: 5 x 5, sigma 1, hysteresis on) --------------
 *   kornia is not installed where this was written, so nothing has confirmed this restatement against it: the definition below is
 *   what the code is held to (tests/canny_ref.py states it in float64).
 *   grey         C = 3: 0.299 r + 0.587 g + 0.114 b; C = 1: the channel.  H >= 3 and W >= 3.
 *   blur         5 x 5 Gaussian, sigma 1, separable (along x, then along y), taps exp(-(i-2)^2 / 2) normalised to sum 1,
 *                border reflect (index -1 -> 1: no repeated edge).
 *   gradient     the un-normalised 3 x 3 Sobel of the integer definition on the blurred image with replicated border;
 *                mag = sqrt(gx^2 + gy^2 + 1e-6).
 *   direction    q = round-half-even(atan2(gy, gx) * 180/pi / 45); neighbour offsets (dx, dy) for index 0..7:
 *                (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1); the pixel is a maximum if
 *                mag - mag[p + off[q mod 8]] > 0 and mag - mag[p + off[(q + 4) mod 8]] > 0; neighbours outside the image count as 0.
 *   classes      a maximum with mag > high is strong, any other maximum with mag > low is weak.
 *   hysteresis   as above.  Output 1.0 at the strong pixels.
 *   All arithmetic is fp32; sums are in the order written in canny.hip.  Comparisons that sit on a threshold may therefore fall
 *   either way against another fp32 evaluation: tests hold the result between the two envelopes of tests/canny_ref.py. */
#ifndef SR_CANNY_H
#define SR_CANNY_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { SR_CANNY_OK = 0, SR_CANNY_ERR_INVALID = -1, SR_CANNY_ERR_LAUNCH = -2 };
/* element types of an image */
enum { SR_CANNY_U8 = 0, SR_CANNY_F32 = 1, SR_CANNY_F16 = 2 };
/* the classes of a class map */
enum { SR_CANNY_NONE = 0, SR_CANNY_WEAK = 1, SR_CANNY_STRONG = 2 };
/* the tile of a hysteresis workgroup: its side in pixels */
enum { SR_CANNY_TILE = 64 };

const char* sr_canny_last_error(void);
const char* sr_canny_source_hash(void);                     /* hash of the sources this image was built from */

/* Gradient, magnitude, suppression and classification of the integer definition in one launch: no intermediate leaves the chip (a
 * workgroup stages its 32 x 32 pixels and two more on every side in LDS, all channels of a pixel packed into one dword).
 *   src      image (B,H,W,C), C in 1..4, of `dtype` (SR_CANNY_U8 / _F32 / _F16); the element (b, y, x, c) lies at
 *            src[b strides[0] + y strides[1] + x strides[2] + c strides[3]], element strides >= 0 (`strides` is a host pointer to
 *            four int64).  Read only.
 *   cls      class map, B H W bytes, every one of them written.  Overlaps nothing.
 *   low,high -1 <= low <= high (already floored and ordered; magnitudes lie in 0..2040) */
int sr_canny_cv_classify(const void* src, int dtype, int B, int H, int W, int C, const int64_t* strides, int low, int high,
                         uint8_t* cls, void* stream);

/* Grey, blur, gradient, direction, suppression and classification of the float definition in one launch, staged as above with four
 * more pixels on every side.
 *   src      fp32 image (B,H,W,C), C = 1 or 3, H >= 3, W >= 3, element strides as above
 *   low,high thresholds on mag, low <= high, both finite */
int sr_canny_k_classify(const float* src, int B, int H, int W, int C, const int64_t* strides, float low, float high, uint8_t* cls,
                        void* stream);

/* One propagation round over a class map, in place.  Each workgroup owns a tile of SR_CANNY_TILE x SR_CANNY_TILE pixels of one image,
 * loads it and a halo of one pixel (0 outside the image: nothing crosses an image's border) into LDS, promotes weak pixels that are
 * 8-adjacent to a strong one until nothing in the tile changes, with workgroup barriers only, and stores the promoted pixels of its
 * interior.  A workgroup never waits for another one.  A halo pixel may be read while its owner promotes it in the same round; it is
 * a single byte that only ever goes from 1 to 2, so either value is a correct state, and the owner reports the change.
 *   changed        caller-owned scratch of `changed_words` int32.  Round `round` (0 <= round < changed_words) leaves changed[round]
 *                  = 1 if any workgroup promoted a pixel and 0 otherwise: round 0 clears its word with a memset node on the stream
 *                  before its kernel, every round's kernel clears the next round's word, and a workgroup that promoted something
 *                  stores 1 with a plain vector store (the same value from every writer; no atomic).  A round > 0 reads
 *                  changed[round - 1] and does nothing but the clearing if it is 0, so a fixed number of rounds can be enqueued,
 *                  or captured in a graph, and only the last word read back.  Rounds are issued in order on one stream.
 *   The fixed point is unique (promotion is monotone), so the class map after a round that reports 0 does not depend on the tile
 *   size or on scheduling (the number of rounds can: a halo may or may not see a promotion of the same round).  Every round that
 *   reports 1 promoted at least one pixel: at most B H W rounds report 1. */
int sr_canny_hysteresis_round(uint8_t* cls, int B, int H, int W, int32_t* changed, int64_t changed_words, int round, void* stream);

/* Class map -> output: strong gives 255 (out_dtype SR_CANNY_U8, c_out = 1) or 1.0f repeated to c_out channels, c_out in 1..4
 * (SR_CANNY_F32: contiguous (n_pix, c_out), that is NHWC); every other class gives 0.  n_pix = B H W.  Every element is written. */
int sr_canny_finish(const uint8_t* cls, int64_t n_pix, void* out, int out_dtype, int c_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
