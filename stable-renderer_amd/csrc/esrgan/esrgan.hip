// libsr_esrgan.so: the 3x3 convolution of the ESRGAN (RRDBNet) upscale models as one patch-stationary implicit-GEMM kernel, and the
// packing of the network's input (sr_esrgan.h).
//
// Why a kernel of its own: a dense block convolves 64, 96, 128, 160 and 192 input channels into 32 (64 for its last layer), applies
// LeakyReLU, and owes its concatenation to where each layer writes; sr_igemm's fp16 path wants multiples of 64, has no LeakyReLU and
// writes whole rows.  N is one or two MFMA tiles here, so the work is in the activation path:
//   a workgroup (4 waves) owns a patch of 8 x 32 output pixels of one image.  Per 32-channel chunk of the input it stages the patch
//   plus its one-pixel halo (10 x 34 pixels x 64 B) into LDS once, and the nine taps read it at nine offsets (the idea of
//   conv3p_kernel in igemm.hip, in plain HIP: global -> registers -> LDS, the next chunk's loads in flight during this chunk's MFMAs,
//   two LDS buffers, one barrier per chunk).  Pixels outside the image are zeros in LDS, so a halo never reaches a neighbouring image.
//   LDS pitch 80 B per pixel (64 B of channels + 16 B): the 16 lanes that a ds_read_b128 serves together read 16 consecutive
//   pixels, 80 B apart, which fall on 16 distinct 16-byte bank groups (5 is coprime to 16); a tap shift is an address offset.
//   MFMA 32x32x16 f16 with the WEIGHTS as the A operand (rows = output channels) and the pixels as B (columns): a lane then holds
//   runs of four consecutive output channels of one pixel, which are 8-byte stores into NHWC and 8-byte loads of the residuals.
//   A wave computes two patch rows (2 x 32 pixels) x Cout.  Weights are not staged: every workgroup reads the same <= 221 KB per
//   layer, packed so that a lane's fragment is 16 contiguous bytes, one tap ahead of its use.
// No split-K, no atomics: the sum order of an output element is fixed by the layer's shape alone.
#include <cstdint>
#include "sr_esrgan.h"
#define SR_SIDE esrgan
#define SR_SIDE_UC ESRGAN
#ifndef SR_ESRGAN_SRC_HASH
#define SR_ESRGAN_SRC_HASH "unstamped"
#endif
#include "../sr_side.h"
#include "../conv3_pack.h"

namespace {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int PH = 8, PW = 32, HW = PW + 2, HPIX = (PH + 2) * HW, PITCH = 80, ABYTES = HPIX * PITCH, SLOTS = HPIX * 4, THREADS = 256;
constexpr int SPT = (SLOTS + THREADS - 1) / THREADS;       // 16-byte halo slots per thread and chunk

template <int NT>
__global__ __launch_bounds__(THREADS) void conv3_kernel(const sr_esr_conv p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * ABYTES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  const int H = p.H, W = p.W, ptx = (W + PW - 1) / PW;
  const int b = blockIdx.y, y0 = ((int)blockIdx.x / ptx) * PH, x0 = ((int)blockIdx.x % ptx) * PW;
  const int Hs = p.up == 2 ? H >> 1 : H, Ws = p.up == 2 ? W >> 1 : W, sh = p.up == 2 ? 1 : 0;
  const _Float16* const in = (const _Float16*)p.src;

  // the halo slots of this thread: element offset of the slot's first channel in chunk 0 (< 2^31 by the host's check), -1 = zeros
  int soff[SPT];
#pragma unroll
  for (int i = 0; i < SPT; ++i) {
    const int u = tid + i * THREADS, hp = u >> 2, q = u & 3, hy = hp / HW, hx = hp - hy * HW;
    const int y = y0 + hy - 1, x = x0 + hx - 1;
    const bool ok = u < SLOTS && y >= 0 && y < H && x >= 0 && x < W;
    soff[i] = ok ? ((b * Hs + (y >> sh)) * Ws + (x >> sh)) * p.ld_in + q * 8 : -1;
  }
  uint4 st[SPT];
  auto load_chunk = [&](int c) {
#pragma unroll
    for (int i = 0; i < SPT; ++i)
      st[i] = soff[i] >= 0 ? *(const uint4*)(in + ((int64_t)soff[i] + c * 32)) : make_uint4(0, 0, 0, 0);
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int i = 0; i < SPT; ++i) {
      const int u = tid + i * THREADS;
      if (u < SLOTS) *(uint4*)(smem + buf * ABYTES + (u >> 2) * PITCH + (u & 3) * 16) = st[i];
    }
  };

  const _Float16* const wl = (const _Float16*)p.w + lane * 8;
  h16x8 wcur[2][NT], wnext[2][NT];
  auto load_w = [&](h16x8 (&wf)[2][NT], int s) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) wf[ks][nt] = *(const h16x8*)(wl + (int64_t)((s * 2 + ks) * NT + nt) * 512);
  };

  f32x16 acc[2][NT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[i][nt][k] = 0.f;

  const int NC = p.Cin / 32, steps = NC * 9;
  load_chunk(0);
  load_w(wcur, 0);
  store_chunk(0);
  __syncthreads();
  // this lane's B fragment (pixel r of the wave's first row, k half h) at tap (0, 0)
  const int xoff = (2 * wv * HW + r) * PITCH + h * 16;
  for (int c = 0; c < NC; ++c) {
    if (c + 1 < NC) load_chunk(c + 1);
    const char* const A = smem + (c & 1) * ABYTES + xoff;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int s = c * 9 + t;
      if (s + 1 < steps) load_w(wnext, s + 1);
      const char* const At = A + ((t / 3) * HW + (t % 3)) * PITCH;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const h16x8 xf = *(const h16x8*)(At + i * HW * PITCH + ks * 32);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[i][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wcur[ks][nt], xf, acc[i][nt], 0, 0, 0);
        }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wcur[ks][nt] = wnext[ks][nt];
    }
    if (c + 1 < NC) store_chunk((c + 1) & 1);       // last read in chunk c - 1, which every wave left at the barrier below
    __syncthreads();
  }

  // epilogue: register 4g + k of a lane is output channel nt * 32 + 8g + 4h + k of pixel r
  const int x = x0 + r;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int y = y0 + 2 * wv + i;
    if (y >= H || x >= W) continue;
    const int64_t m = ((int64_t)b * H + y) * W + x;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = nt * 32 + 8 * g + 4 * h;
        const float4 bb = *(const float4*)(p.bias + n);
        float v[4] = {acc[i][nt][4 * g] + bb.x, acc[i][nt][4 * g + 1] + bb.y, acc[i][nt][4 * g + 2] + bb.z, acc[i][nt][4 * g + 3] + bb.w};
        if (p.lrelu) {
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = v[k] < 0.f ? 0.2f * v[k] : v[k];
        }
        if (p.r1) {
          const h16x4 rr = *(const h16x4*)((const _Float16*)p.r1 + m * p.ld_r1 + n);
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = v[k] * p.s1 + (float)rr[k];
          if (p.r2) {
            const h16x4 r2 = *(const h16x4*)((const _Float16*)p.r2 + m * p.ld_r2 + n);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = v[k] * p.s2 + (float)r2[k];
          }
        }
        if (p.out_f32) {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (n + k < p.n_store) p.out_f32[m * p.n_store + n + k] = v[k];
        } else {
          const h16x4 hv = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
          *(h16x4*)((_Float16*)p.out + m * p.ld_out + p.c_off + n) = hv;
          if (p.out2) *(h16x4*)((_Float16*)p.out2 + m * p.ld_out2 + n) = hv;
        }
      }
  }
}

struct pack_args {
  const float* src;
  _Float16* dst;
  int64_t sb, sy, sx, sc, total;
  int h, w, C, s, ho, wo, ld;
};

__global__ __launch_bounds__(256) void pack_input_kernel(const pack_args a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.total) return;
  const int ch = (int)(e % a.ld);
  const int64_t pix = e / a.ld;
  const int xo = (int)(pix % a.wo), yo = (int)((pix / a.wo) % a.ho), b = (int)(pix / ((int64_t)a.wo * a.ho));
  float v = 0.f;
  const int ss = a.s * a.s;
  if (ch < a.C * ss) {
    const int c = ch / ss, d = ch - c * ss, dy = d / a.s, dx = d - dy * a.s;
    int y = yo * a.s + dy, x = xo * a.s + dx;
    if (y >= a.h) y = 2 * (a.h - 1) - y;            // reflect, without the edge
    if (x >= a.w) x = 2 * (a.w - 1) - x;
    v = a.src[b * a.sb + y * a.sy + x * a.sx + c * a.sc];
  }
  a.dst[e] = (_Float16)v;
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

int check_layer(const sr_esr_conv& L, int i) {
  if (!L.src || !L.w || !L.bias || (!L.out && !L.out_f32)) SR_FAIL(SR_ERR_INVALID, "sr_esr_run: layer %d: null src, w, bias or output", i);
  if (L.B < 1 || L.H < 1 || L.W < 1 || L.B > 65535) SR_FAIL(SR_ERR_INVALID, "sr_esr_run: layer %d: sizes (%d, %d, %d) must be positive (B <= 65535)", i, L.B, L.H, L.W);
  if (L.Cin < 32 || L.Cin % 32 || (L.Cout != 32 && L.Cout != 64)) SR_FAIL(SR_ERR_INVALID, "sr_esr_run: layer %d: Cin = %d must be a multiple of 32 and Cout = %d 32 or 64", i, L.Cin, L.Cout);
  if (L.up != 1 && L.up != 2) SR_FAIL(SR_ERR_INVALID, "sr_esr_run: layer %d: up = %d is not 1 or 2", i, L.up);
  if (L.up == 2 && ((L.H | L.W) & 1)) SR_FAIL(SR_ERR_INVALID, "sr_esr_run: layer %d: up = 2 wants even H and W, not %d x %d", i, L.H, L.W);
  if (L.lrelu != 0 && L.lrelu != 1) SR_FAIL(SR_ERR_INVALID, "sr_esr_run: layer %d: lrelu = %d", i, L.lrelu);
  if (L.r2 && !L.r1) SR_FAIL(SR_ERR_INVALID, "sr_esr_run: layer %d: r2 without r1", i);
  const int64_t pix = (int64_t)L.B * L.H * L.W, lim = (int64_t)1 << 31;
  auto pitch_ok = [&](int ld, int need) { return ld >= need && ld % 8 == 0 && pix * ld < lim; };
  if (!pitch_ok(L.ld_in, L.Cin)) SR_FAIL(SR_ERR_INVALID, "sr_esr_run: layer %d: ld_in = %d (Cin = %d; a multiple of 8; B H W ld < 2^31)", i, L.ld_in, L.Cin);
  if (!aligned16(L.src) || !aligned16(L.w) || !aligned16(L.bias)) SR_FAIL(SR_ERR_INVALID, "sr_esr_run: layer %d: src, w and bias must be 16-byte aligned", i);
  if (L.out_f32) {
    if (L.n_store < 1 || L.n_store > L.Cout || pix * L.n_store >= lim) SR_FAIL(SR_ERR_INVALID, "sr_esr_run: layer %d: n_store = %d", i, L.n_store);
  } else {
    if (L.c_off < 0 || L.c_off % 8 || (int64_t)L.c_off + L.Cout > L.ld_out || !pitch_ok(L.ld_out, L.Cout))
      SR_FAIL(SR_ERR_INVALID, "sr_esr_run: layer %d: c_off = %d, Cout = %d, ld_out = %d (the slice lies inside a row; multiples of 8; B H W ld < 2^31)", i, L.c_off, L.Cout, L.ld_out);
    if (!aligned16(L.out)) SR_FAIL(SR_ERR_INVALID, "sr_esr_run: layer %d: out must be 16-byte aligned", i);
    if (L.out2 && (!pitch_ok(L.ld_out2, L.Cout) || !aligned16(L.out2))) SR_FAIL(SR_ERR_INVALID, "sr_esr_run: layer %d: ld_out2 = %d", i, L.ld_out2);
  }
  if (L.r1 && (!pitch_ok(L.ld_r1, L.Cout) || !aligned16(L.r1))) SR_FAIL(SR_ERR_INVALID, "sr_esr_run: layer %d: ld_r1 = %d", i, L.ld_r1);
  if (L.r2 && (!pitch_ok(L.ld_r2, L.Cout) || !aligned16(L.r2))) SR_FAIL(SR_ERR_INVALID, "sr_esr_run: layer %d: ld_r2 = %d", i, L.ld_r2);
  return SR_OK;
}

}  // namespace

extern "C" int64_t sr_esr_packed_index(int32_t Cout, int32_t Cin, int32_t n, int32_t c, int32_t ky, int32_t kx) {
  return conv3_packed_index(Cout, Cin, n, c, ky, kx);
}

extern "C" int sr_esr_run(const sr_esr_conv* layers, int32_t n, void* stream) {
  if (!layers || n < 1 || n > SR_ESR_MAX_LAYERS) SR_FAIL(SR_ERR_INVALID, "sr_esr_run: null layers or n = %d not in 1..%d", n, (int)SR_ESR_MAX_LAYERS);
  for (int i = 0; i < n; ++i) {
    const int rc = check_layer(layers[i], i);
    if (rc != SR_OK) return rc;
  }
  for (int i = 0; i < n; ++i) {
    const sr_esr_conv& L = layers[i];
    const dim3 grid((unsigned)(((L.W + PW - 1) / PW) * ((L.H + PH - 1) / PH)), (unsigned)L.B);
    if (L.Cout == 32) hipLaunchKernelGGL((conv3_kernel<1>), grid, dim3(THREADS), 0, sr_stream(stream), L);
    else hipLaunchKernelGGL((conv3_kernel<2>), grid, dim3(THREADS), 0, sr_stream(stream), L);
    SR_CHECK_LAUNCH("sr_esr_run");
  }
  return SR_OK;
}

extern "C" int sr_esr_pack_input(const float* src, int64_t sb, int64_t sy, int64_t sx, int64_t sc, int32_t B, int32_t h, int32_t w,
                                 int32_t C, int32_t shuffle, void* dst, int32_t ld_dst, void* stream) {
  if (!src || !dst) SR_FAIL(SR_ERR_INVALID, "sr_esr_pack_input: null pointer");
  if (B < 1 || h < 1 || w < 1 || C < 1) SR_FAIL(SR_ERR_INVALID, "sr_esr_pack_input: sizes (%d, %d, %d, %d) must be positive", B, h, w, C);
  if (shuffle != 1 && shuffle != 2 && shuffle != 4) SR_FAIL(SR_ERR_INVALID, "sr_esr_pack_input: shuffle = %d is not 1, 2 or 4", shuffle);
  if (sb < 0 || sy < 0 || sx < 0 || sc < 0) SR_FAIL(SR_ERR_INVALID, "sr_esr_pack_input: negative stride");
  const int ph = (shuffle - h % shuffle) % shuffle, pw = (shuffle - w % shuffle) % shuffle;
  if (ph >= h || pw >= w) SR_FAIL(SR_ERR_INVALID, "sr_esr_pack_input: the reflect padding (%d, %d) must be smaller than the window %d x %d", ph, pw, h, w);
  if (ld_dst % 8 || (int64_t)C * shuffle * shuffle > ld_dst) SR_FAIL(SR_ERR_INVALID, "sr_esr_pack_input: ld_dst = %d must be a multiple of 8 and hold %d channels", ld_dst, C * shuffle * shuffle);
  pack_args a;
  a.src = src; a.dst = (_Float16*)dst; a.sb = sb; a.sy = sy; a.sx = sx; a.sc = sc;
  a.h = h; a.w = w; a.C = C; a.s = shuffle; a.ho = (h + ph) / shuffle; a.wo = (w + pw) / shuffle; a.ld = ld_dst;
  a.total = (int64_t)B * a.ho * a.wo * ld_dst;
  if (a.total >= ((int64_t)1 << 31)) SR_FAIL(SR_ERR_INVALID, "sr_esr_pack_input: B H W ld = %lld is not below 2^31", (long long)a.total);
  hipLaunchKernelGGL(pack_input_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, sr_stream(stream), a);
  SR_CHECK_LAUNCH("sr_esr_pack_input");
  return SR_OK;
}
