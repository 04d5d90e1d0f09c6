// Canny edge detection in the two definitions of sr_canny.h: the integer one of cv2.Canny (the reference's ai_canny map) and the float
// one behind the Canny graph node.  libsr_canny.so, private C ABI in sr_canny.h; why it is a library of its own and a private one:
// csrc/sidelib.py.
//
// classify   one launch per definition.  A workgroup of 256 threads owns 32 x 32 pixels and stages everything its stencils reach in
//            LDS: the integer kernel its pixels and two more on every side (the channels of a pixel packed into one dword), then the
//            winning channel's (gx, gy) and magnitude for its pixels and one more on every side, then the suppression; the float
//            kernel four more pixels of grey, the blur along x, the blur along y, the gradient, the suppression.  Image borders are
//            folded into the staging (clamped or reflected coordinates; magnitude 0 outside), so the stencils themselves are
//            branch-free.  The only traffic is the image read (with the halo's re-reads, which the caches serve) and one byte per
//            pixel written.
// hysteresis one launch per round, a workgroup per 64 x 64 tile: sr_canny.h has the scheme and why it terminates.  A thread owns 16
//            consecutive pixels of a row and sweeps them forwards and backwards, so a run along a row costs one sweep, not 16.
// finish     one byte read, one element written per output channel.
#include <cmath>
#include <cstdint>
#include <hip/hip_fp16.h>
#include "sr_canny.h"
#define SR_SIDE canny
#define SR_SIDE_UC CANNY
#ifndef SR_CANNY_SRC_HASH
#define SR_CANNY_SRC_HASH "unstamped"
#endif
#include "../sr_side.h"

namespace {

constexpr int THREADS = 256;
constexpr int CT = 32;                      // pixels per side of a classify tile
constexpr int HT = SR_CANNY_TILE;           // pixels per side of a hysteresis tile
constexpr int HP = HT + 2;                  // with the halo
constexpr int HPITCH = 68;                  // bytes per row of the hysteresis tile in LDS

struct Image {
  const void* p;
  int64_t s[4];
  int B, H, W, C;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }

// (uint8)(v * 255) with the product in fp32, clamped to 0..255; NaN -> 0
__device__ __forceinline__ unsigned to_u8(float v) {
  const float s = v * 255.f;
  if (!(s > 0.f)) return 0u;
  return s >= 255.f ? 255u : (unsigned)(int)s;
}

template <int DTYPE>
__device__ __forceinline__ unsigned load_u8(const void* p, int64_t off) {
  if (DTYPE == SR_CANNY_U8) return static_cast<const uint8_t*>(p)[off];
  if (DTYPE == SR_CANNY_F32) return to_u8(static_cast<const float*>(p)[off]);
  return to_u8(__half2float(static_cast<const __half*>(p)[off]));
}

// ---- the integer definition -----------------------------------------------------------------------------------------------------------
template <int DTYPE>
__global__ void __launch_bounds__(THREADS) cv_classify_kernel(Image im, int low, int high, uint8_t* __restrict__ cls) {
  constexpr int PW = CT + 4, MW = CT + 2;
  __shared__ uint32_t pix[PW * PW];         // (r, c) is the pixel (y0 - 2 + r, x0 - 2 + c), clamped into the image
  __shared__ int mag[MW * MW];              // (r, c) is the pixel (y0 - 1 + r, x0 - 1 + c); 0 outside the image
  __shared__ int gxy[MW * MW];              // gx in the low half, gy in the high half, of the winning channel
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * CT, y0 = blockIdx.y * CT, b = blockIdx.z;
  const int H = im.H, W = im.W, C = im.C;
  const int64_t base = (int64_t)b * im.s[0];

  for (int e = tid; e < PW * PW; e += THREADS) {
    const int r = e / PW, c = e - r * PW;
    const int y = clampi(y0 - 2 + r, 0, H - 1), x = clampi(x0 - 2 + c, 0, W - 1);
    const int64_t off = base + (int64_t)y * im.s[1] + (int64_t)x * im.s[2];
    uint32_t v = 0;
    for (int ch = 0; ch < C; ++ch) v |= load_u8<DTYPE>(im.p, off + (int64_t)ch * im.s[3]) << (8 * ch);
    pix[e] = v;                             // a channel that is not there is 0 everywhere: its magnitude 0 never wins
  }
  __syncthreads();

  for (int e = tid; e < MW * MW; e += THREADS) {
    const int r = e / MW, c = e - r * MW;
    const int y = y0 - 1 + r, x = x0 - 1 + c;
    int bm = 0, bgx = 0, bgy = 0;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const uint32_t* q = pix + r * PW + c;                    // the 3 x 3 around (r + 1, c + 1)
      const uint32_t a00 = q[0], a01 = q[1], a02 = q[2], a10 = q[PW], a12 = q[PW + 2], a20 = q[2 * PW], a21 = q[2 * PW + 1],
                     a22 = q[2 * PW + 2];
      bm = -1;
      for (int ch = 0; ch < 4; ++ch) {
        const int sh = 8 * ch;
        const int p00 = (a00 >> sh) & 255, p01 = (a01 >> sh) & 255, p02 = (a02 >> sh) & 255, p10 = (a10 >> sh) & 255,
                  p12 = (a12 >> sh) & 255, p20 = (a20 >> sh) & 255, p21 = (a21 >> sh) & 255, p22 = (a22 >> sh) & 255;
        const int gx = (p02 + 2 * p12 + p22) - (p00 + 2 * p10 + p20);
        const int gy = (p20 + 2 * p21 + p22) - (p00 + 2 * p01 + p02);
        const int m = iabs(gx) + iabs(gy);
        if (m > bm) { bm = m; bgx = gx; bgy = gy; }            // strictly greater: the first channel wins a tie
      }
    }
    mag[e] = bm;
    gxy[e] = (bgx & 0xffff) | (int)((unsigned)bgy << 16);
  }
  __syncthreads();

  for (int e = tid; e < CT * CT; e += THREADS) {
    const int r = e / CT, c = e - r * CT;
    const int y = y0 + r, x = x0 + c;
    if (y >= H || x >= W) continue;
    const int* mp = mag + (r + 1) * MW + (c + 1);
    const int m = mp[0];
    int klass = SR_CANNY_NONE;
    if (m > low) {
      const int g = gxy[(r + 1) * MW + (c + 1)];
      const int gx = (int)(int16_t)(g & 0xffff), gy = g >> 16;
      const int xs = iabs(gx), ys = iabs(gy) << 15;
      const int t22 = xs * 13573;
      bool keep;
      if (ys < t22) {
        keep = m > mp[-1] && m >= mp[1];
      } else if (ys > t22 + (xs << 16)) {
        keep = m > mp[-MW] && m >= mp[MW];
      } else {
        const int s = (gx ^ gy) < 0 ? -1 : 1;
        keep = m > mp[-MW - s] && m > mp[MW + s];
      }
      if (keep) klass = m > high ? SR_CANNY_STRONG : SR_CANNY_WEAK;
    }
    cls[((int64_t)b * H + y) * W + x] = (uint8_t)klass;
  }
}

// ---- the float definition -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflecti(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

struct Taps { float w[5]; };

__global__ void __launch_bounds__(THREADS) k_classify_kernel(Image im, Taps tp, float low, float high, uint8_t* __restrict__ cls) {
  constexpr int GW = CT + 8, BW = CT + 4, MW = CT + 2;
  __shared__ float grey[GW * GW];           // (r, c) is the pixel (y0 - 4 + r, x0 - 4 + c) where that lies in the image
  __shared__ float hb[GW * BW];             // blurred along x: row as grey, column c is x = clamp(x0 - 2 + c)
  __shared__ float bl[BW * BW];             // blurred: (r, c) is the pixel (clamp(y0 - 2 + r), clamp(x0 - 2 + c)): the replicated border
  __shared__ float mag[MW * MW];            // (r, c) is the pixel (y0 - 1 + r, x0 - 1 + c); 0 outside the image
  __shared__ float sgx[MW * MW];
  __shared__ float sgy[MW * MW];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * CT, y0 = blockIdx.y * CT, b = blockIdx.z;
  const int H = im.H, W = im.W;
  const float* src = static_cast<const float*>(im.p);
  const int64_t base = (int64_t)b * im.s[0];

  for (int e = tid; e < GW * GW; e += THREADS) {
    const int r = e / GW, c = e - r * GW;
    const int y = y0 - 4 + r, x = x0 - 4 + c;
    float v = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const int64_t off = base + (int64_t)y * im.s[1] + (int64_t)x * im.s[2];
      v = src[off];
      if (im.C == 3) v = 0.299f * v + 0.587f * src[off + im.s[3]] + 0.114f * src[off + 2 * im.s[3]];
    }
    grey[e] = v;
  }
  __syncthreads();

  for (int e = tid; e < GW * BW; e += THREADS) {
    const int r = e / BW, c = e - r * BW;
    const int y = y0 - 4 + r;
    float v = 0.f;
    if (y >= 0 && y < H) {
      const int cx = clampi(x0 - 2 + c, 0, W - 1);
      const float* g = grey + r * GW - (x0 - 4);
      for (int j = 0; j < 5; ++j) v += tp.w[j] * g[reflecti(cx + j - 2, W)];
    }
    hb[e] = v;
  }
  __syncthreads();

  for (int e = tid; e < BW * BW; e += THREADS) {
    const int r = e / BW, c = e - r * BW;
    const int cy = clampi(y0 - 2 + r, 0, H - 1);
    float v = 0.f;
    for (int i = 0; i < 5; ++i) v += tp.w[i] * hb[(reflecti(cy + i - 2, H) - (y0 - 4)) * BW + c];
    bl[e] = v;
  }
  __syncthreads();

  for (int e = tid; e < MW * MW; e += THREADS) {
    const int r = e / MW, c = e - r * MW;
    const int y = y0 - 1 + r, x = x0 - 1 + c;
    float gx = 0.f, gy = 0.f, m = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const float* q = bl + r * BW + c;                        // the 3 x 3 around (r + 1, c + 1)
      gx = (q[2] + 2.f * q[BW + 2] + q[2 * BW + 2]) - (q[0] + 2.f * q[BW] + q[2 * BW]);
      gy = (q[2 * BW] + 2.f * q[2 * BW + 1] + q[2 * BW + 2]) - (q[0] + 2.f * q[1] + q[2]);
      m = sqrtf(gx * gx + gy * gy + 1e-6f);
    }
    mag[e] = m;
    sgx[e] = gx;
    sgy[e] = gy;
  }
  __syncthreads();

  for (int e = tid; e < CT * CT; e += THREADS) {
    const int r = e / CT, c = e - r * CT;
    const int y = y0 + r, x = x0 + c;
    if (y >= H || x >= W) continue;
    const int at = (r + 1) * MW + (c + 1);
    const float m = mag[at];
    const int q = (int)rintf(atan2f(sgy[at], sgx[at]) * 57.29577951308232f / 45.f);      // -4 .. 4, halves to even
    const int i0 = (q + 8) & 7, i1 = (q + 12) & 7;
    // (dx, dy) of the index 0..7: (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1)
    const int dx0 = (i0 == 0 || i0 == 1 || i0 == 7) - (i0 >= 3 && i0 <= 5), dy0 = (i0 >= 1 && i0 <= 3) - (i0 >= 5);
    const int dx1 = (i1 == 0 || i1 == 1 || i1 == 7) - (i1 >= 3 && i1 <= 5), dy1 = (i1 >= 1 && i1 <= 3) - (i1 >= 5);
    const bool is_max = m - mag[at + dy0 * MW + dx0] > 0.f && m - mag[at + dy1 * MW + dx1] > 0.f;
    const int klass = !is_max ? SR_CANNY_NONE : (m > high ? SR_CANNY_STRONG : (m > low ? SR_CANNY_WEAK : SR_CANNY_NONE));
    cls[((int64_t)b * H + y) * W + x] = (uint8_t)klass;
  }
}

// ---- hysteresis -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool strong_near(const uint8_t* t) {
  return t[-HPITCH - 1] == 2 || t[-HPITCH] == 2 || t[-HPITCH + 1] == 2 || t[-1] == 2 || t[1] == 2 || t[HPITCH - 1] == 2 ||
         t[HPITCH] == 2 || t[HPITCH + 1] == 2;
}

// prev: the word of the round before (null in round 0); mine: this round's word, cleared before this launch; next: the word of the
// round after (null when there is none)
__global__ void __launch_bounds__(THREADS) hysteresis_kernel(uint8_t* __restrict__ cls, int H, int W, const int32_t* prev,
                                                             int32_t* mine, int32_t* next) {
  __shared__ uint8_t tile[HP * HPITCH];     // (r, c) is the pixel (y0 - 1 + r, x0 - 1 + c); 0 outside the image
  const int tid = threadIdx.x;
  if (next && tid == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) *next = 0;
  if (prev && *prev == 0) return;           // the round before changed nothing: this one would not either
  const int x0 = blockIdx.x * HT, y0 = blockIdx.y * HT;
  uint8_t* img = cls + (int64_t)blockIdx.z * H * W;

  for (int e = tid; e < HP * HP; e += THREADS) {
    const int r = e / HP, c = e - r * HP;
    const int y = y0 - 1 + r, x = x0 - 1 + c;
    tile[r * HPITCH + c] = (y >= 0 && y < H && x >= 0 && x < W) ? img[(int64_t)y * W + x] : (uint8_t)0;
  }
  __syncthreads();

  // this thread's 16 pixels: row tid / 4 of the interior, columns 16 (tid % 4) ... + 15
  const int row = tid >> 2, col = (tid & 3) * 16;
  uint8_t* mine_px = tile + (row + 1) * HPITCH + (col + 1);
  unsigned weak = 0;
  for (int i = 0; i < 16; ++i) weak |= (mine_px[i] == 1 ? 1u : 0u) << i;
  const unsigned weak0 = weak;
  if (!__syncthreads_or(weak != 0)) return;                    // no weak pixel in the tile: nothing to promote

  for (;;) {
    bool ch = false;
    if (weak) {
      for (int i = 0; i < 16; ++i)
        if ((weak >> i & 1u) && strong_near(mine_px + i)) { mine_px[i] = 2; weak &= ~(1u << i); ch = true; }
      for (int i = 15; i >= 0; --i)
        if ((weak >> i & 1u) && strong_near(mine_px + i)) { mine_px[i] = 2; weak &= ~(1u << i); ch = true; }
    }
    // a sweep in which no thread promoted anything read only settled values (the barrier orders the sweep before): the fixed point
    if (!__syncthreads_or(ch)) break;
  }

  const unsigned promoted = weak0 & ~weak;
  if (promoted) {
    uint8_t* out = img + (int64_t)(y0 + row) * W + (x0 + col);   // a promoted pixel was weak, so it lies in the image
    for (int i = 0; i < 16; ++i)
      if (promoted >> i & 1u) out[i] = 2;
  }
  if (__syncthreads_or(promoted != 0) && tid == 0) *mine = 1;
}

// ---- finish ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(THREADS) finish_u8_kernel(const uint8_t* __restrict__ cls, int64_t n, uint8_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = cls[i] == 2 ? 255 : 0;
}

__global__ void __launch_bounds__(THREADS) finish_f32_kernel(const uint8_t* __restrict__ cls, int64_t n_pix, float* __restrict__ out,
                                                             int c_out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += stride) {
    const float v = cls[i] == 2 ? 1.f : 0.f;
    for (int c = 0; c < c_out; ++c) out[i * c_out + c] = v;
  }
}

// the checks the two classify entry points share -> false with the error set
bool check_image(const char* fn, const void* src, const uint8_t* cls, const int64_t* strides, int B, int H, int W, int C, int cmin,
                 int cmax, int min_side) {
  if (!src || !cls || !strides) { set_error("%s: null src, cls or strides", fn); return false; }
  if (B < 1 || H < 1 || W < 1) { set_error("%s: sizes (%d, %d, %d) must be positive", fn, B, H, W); return false; }
  if (C < cmin || C > cmax || (cmax == 3 && C == 2)) { set_error("%s: C = %d channels are not accepted", fn, C); return false; }
  if (H < min_side || W < min_side) { set_error("%s: H = %d, W = %d: at least %d each", fn, H, W, min_side); return false; }
  for (int i = 0; i < 4; ++i)
    if (strides[i] < 0) { set_error("%s: negative stride", fn); return false; }
  if (B > 65535 || (int64_t)(H + CT - 1) / CT > 65535 || (int64_t)H * W > 0x7fffffffLL) { set_error("%s: the image is too large", fn); return false; }
  return true;
}

Image image_of(const void* src, const int64_t* strides, int B, int H, int W, int C) {
  Image im;
  im.p = src;
  for (int i = 0; i < 4; ++i) im.s[i] = strides[i];
  im.B = B; im.H = H; im.W = W; im.C = C;
  return im;
}

}  // namespace

extern "C" int sr_canny_cv_classify(const void* src, int dtype, int B, int H, int W, int C, const int64_t* strides, int low, int high,
                                    uint8_t* cls, void* stream) {
  if (!check_image("sr_canny_cv_classify", src, cls, strides, B, H, W, C, 1, 4, 1)) return SR_ERR_INVALID;
  if (dtype < SR_CANNY_U8 || dtype > SR_CANNY_F16) SR_FAIL(SR_ERR_INVALID, "sr_canny_cv_classify: unknown dtype %d", dtype);
  if (low < -1 || high < low) SR_FAIL(SR_ERR_INVALID, "sr_canny_cv_classify: thresholds %d, %d: -1 <= low <= high", low, high);
  const Image im = image_of(src, strides, B, H, W, C);
  const dim3 grid((W + CT - 1) / CT, (H + CT - 1) / CT, B), block(THREADS);
  hipStream_t st = sr_stream(stream);
  if (dtype == SR_CANNY_U8) hipLaunchKernelGGL(cv_classify_kernel<SR_CANNY_U8>, grid, block, 0, st, im, low, high, cls);
  else if (dtype == SR_CANNY_F32) hipLaunchKernelGGL(cv_classify_kernel<SR_CANNY_F32>, grid, block, 0, st, im, low, high, cls);
  else hipLaunchKernelGGL(cv_classify_kernel<SR_CANNY_F16>, grid, block, 0, st, im, low, high, cls);
  SR_CHECK_LAUNCH("sr_canny_cv_classify");
  return SR_OK;
}

extern "C" int sr_canny_k_classify(const float* src, int B, int H, int W, int C, const int64_t* strides, float low, float high,
                                   uint8_t* cls, void* stream) {
  if (!check_image("sr_canny_k_classify", src, cls, strides, B, H, W, C, 1, 3, 3)) return SR_ERR_INVALID;
  if (!(low <= high) || !(high - low < 3.0e38f)) SR_FAIL(SR_ERR_INVALID, "sr_canny_k_classify: thresholds %g, %g: finite, low <= high", low, high);
  Taps tp;
  double sum = 0, w[5];
  for (int i = 0; i < 5; ++i) sum += w[i] = exp(-0.5 * (i - 2) * (i - 2));
  for (int i = 0; i < 5; ++i) tp.w[i] = (float)(w[i] / sum);
  const Image im = image_of(src, strides, B, H, W, C);
  const dim3 grid((W + CT - 1) / CT, (H + CT - 1) / CT, B), block(THREADS);
  hipLaunchKernelGGL(k_classify_kernel, grid, block, 0, sr_stream(stream), im, tp, low, high, cls);
  SR_CHECK_LAUNCH("sr_canny_k_classify");
  return SR_OK;
}

extern "C" int sr_canny_hysteresis_round(uint8_t* cls, int B, int H, int W, int32_t* changed, int64_t changed_words, int round,
                                         void* stream) {
  if (!cls || !changed) SR_FAIL(SR_ERR_INVALID, "sr_canny_hysteresis_round: null cls or changed");
  if (B < 1 || H < 1 || W < 1) SR_FAIL(SR_ERR_INVALID, "sr_canny_hysteresis_round: sizes (%d, %d, %d) must be positive", B, H, W);
  if (round < 0 || changed_words <= round)
    SR_FAIL(SR_ERR_INVALID, "sr_canny_hysteresis_round: changed holds %lld words, round %d needs %lld", (long long)changed_words, round,
            (long long)round + 1);
  if (B > 65535 || (int64_t)(H + HT - 1) / HT > 65535 || (int64_t)H * W > 0x7fffffffLL)
    SR_FAIL(SR_ERR_INVALID, "sr_canny_hysteresis_round: the image is too large");
  hipStream_t st = sr_stream(stream);
  if (round == 0) {
    const hipError_t e = hipMemsetAsync(changed, 0, sizeof(int32_t), st);
    if (e != hipSuccess) SR_FAIL(SR_SIDE_ID(_ERR_LAUNCH), "sr_canny_hysteresis_round: memset: %s", hipGetErrorString(e));
  }
  const dim3 grid((W + HT - 1) / HT, (H + HT - 1) / HT, B), block(THREADS);
  hipLaunchKernelGGL(hysteresis_kernel, grid, block, 0, st, cls, H, W, round > 0 ? changed + (round - 1) : nullptr, changed + round,
                     round + 1 < changed_words ? changed + (round + 1) : nullptr);
  SR_CHECK_LAUNCH("sr_canny_hysteresis_round");
  return SR_OK;
}

extern "C" int sr_canny_finish(const uint8_t* cls, int64_t n_pix, void* out, int out_dtype, int c_out, void* stream) {
  if (!cls || !out) SR_FAIL(SR_ERR_INVALID, "sr_canny_finish: null cls or out");
  if (n_pix < 1 || n_pix > (INT64_MAX >> 4)) SR_FAIL(SR_ERR_INVALID, "sr_canny_finish: n_pix = %lld", (long long)n_pix);
  if (out_dtype != SR_CANNY_U8 && out_dtype != SR_CANNY_F32) SR_FAIL(SR_ERR_INVALID, "sr_canny_finish: unknown out_dtype %d", out_dtype);
  if (c_out < 1 || c_out > 4 || (out_dtype == SR_CANNY_U8 && c_out != 1))
    SR_FAIL(SR_ERR_INVALID, "sr_canny_finish: c_out = %d (1 for uint8, 1..4 for fp32)", c_out);
  int64_t blocks = (n_pix + THREADS - 1) / THREADS;
  if (blocks > 2048) blocks = 2048;
  hipStream_t st = sr_stream(stream);
  if (out_dtype == SR_CANNY_U8)
    hipLaunchKernelGGL(finish_u8_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, cls, n_pix, static_cast<uint8_t*>(out));
  else
    hipLaunchKernelGGL(finish_f32_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, cls, n_pix, static_cast<float*>(out), c_out);
  SR_CHECK_LAUNCH("sr_canny_finish");
  return SR_OK;
}
