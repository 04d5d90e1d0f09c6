// libsr_t2i.so: the convolutions of the T2I-Adapter network as one MFMA implicit-GEMM kernel, its average pooling, the packing of
// the hint (channel mean + PixelUnshuffle) and the scaled, replicated hand-over of a feature map to the UNet's control buffers
// (sr_t2i.h).  taesd.hip, esrgan.hip, compact.hip and libsr_hip.so stay as they are.
//
// The adapter's four levels differ by 64x in pixel count and by 4x in width: N 64^2 pixels at 320 channels down to N 8^2 at 1280,
// K up to 9 x 1280.  What the levels share is that a map is evaluated ONCE per hint, outside the step plan, so the kernel is built
// for a fixed sum order and for small maps first, not for the last percent at the large ones:
//   GEMM view      m = output pixel (b, y, x) flattened over the batch, n = output channel, k = (tap, input channel), tap-major.
//   MFMA           32x32x16 f16 with the WEIGHTS as the A operand (rows = output channels) and the pixels as B (columns), as in
//                  taesd.hip: a lane then holds runs of four consecutive output channels of one pixel, 8-byte stores into NHWC.
//   operands       read straight from global memory, 16 bytes per lane and fragment: a lane's B fragment is 8 consecutive channels
//                  of its own pixel at the tap (NHWC makes that contiguous), its A fragment 16 contiguous bytes of the packed
//                  weights.  Nothing is staged in LDS and there is no barrier: a workgroup is ONE wave, and the small maps (where
//                  the whole layer is a few hundred waves reading 29 MB of weights) get all the parallelism Cout / 32 can give.
//                  Neighbouring workgroups (blockIdx.x = pixel tile) share their weight fragments through L2.
//   a tap whose source pixel lies outside the map for every lane of the wave is skipped (its products are zeros, and adding +0 to
//   an fp32 accumulator leaves its bits alone): on a 1x1 map eight of nine taps, on 2x2 five of nine, never read.
//   Two tile forms, chosen from (H, W, Cout) only:
//     <2, 2>  64 channels x 64 pixels per wave, four accumulators, each fragment feeds two MFMAs: maps of >= 1024 pixels
//     <1, 1>  32 channels x 32 pixels per wave: everything smaller
//   Both walk K in the same order with one accumulator per output element, so they give the same bits, and so does any batching.
#include <cstdint>
#include "sr_t2i.h"
#define SR_SIDE t2i
#define SR_SIDE_UC T2I
#ifndef SR_T2I_SRC_HASH
#define SR_T2I_SRC_HASH "unstamped"
#endif
#include "../sr_side.h"

namespace {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int PT, int CT>
__global__ __launch_bounds__(64) void conv_kernel(const sr_t2i_conv p) {
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int HW = p.H * p.W, M = p.B * HW;                         // < 2^31 by the host's check
  const int m0 = (int)blockIdx.x * (32 * PT), n0 = (int)blockIdx.y * (32 * CT);
  const int KC = p.Cin / 16, NT = p.Cout / 32;
  const _Float16* const in = (const _Float16*)p.src;

  int pb[PT], py[PT], px[PT];
  bool pv[PT];
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    const int m = m0 + i * 32 + r;
    pv[i] = m < M;
    const int mm = pv[i] ? m : 0;
    pb[i] = mm / HW;
    const int rem = mm - pb[i] * HW;
    py[i] = rem / p.W;
    px[i] = rem - py[i] * p.W;
  }
  f32x16 acc[PT][CT];
#pragma unroll
  for (int i = 0; i < PT; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[i][j][k] = 0.f;

  const h16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  const _Float16* const wl = (const _Float16*)p.w + lane * 8 + (int64_t)(n0 / 32) * 512;
  const int taps = p.ksize * p.ksize;
  for (int t = 0; t < taps; ++t) {
    const int ky = p.ksize == 3 ? t / 3 - 1 : 0, kx = p.ksize == 3 ? t % 3 - 1 : 0;
    const _Float16* sp[PT];
    bool ok[PT], any = false;
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int sy = py[i] * p.stride + ky, sx = px[i] * p.stride + kx;
      ok[i] = pv[i] && sy >= 0 && sy < p.Hs && sx >= 0 && sx < p.Ws;
      sp[i] = in + (ok[i] ? ((int64_t)(pb[i] * p.Hs + sy) * p.Ws + sx) * p.ld_in + h * 8 : 0);
      any = any || ok[i];
    }
    if (!__any(any)) continue;                                    // wave-uniform: every lane's source pixel is padding
    const _Float16* const wt = wl + (int64_t)t * KC * NT * 512;
#pragma unroll 4
    for (int kc = 0; kc < KC; ++kc) {
      h16x8 a[CT], b[PT];
#pragma unroll
      for (int j = 0; j < CT; ++j) a[j] = *(const h16x8*)(wt + ((int64_t)kc * NT + j) * 512);
#pragma unroll
      for (int i = 0; i < PT; ++i) b[i] = ok[i] ? *(const h16x8*)(sp[i] + kc * 16) : zero;
#pragma unroll
      for (int i = 0; i < PT; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[j], b[i], acc[i][j], 0, 0, 0);
    }
  }

  // epilogue: register 4g + k of a lane is output channel 8g + 4h + k (of the 32 of tile j) of pixel r (of tile i)
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    if (!pv[i]) continue;
    const int64_t m = m0 + i * 32 + r;
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + j * 32 + 8 * g + 4 * h;
        const float4 bb = *(const float4*)(p.bias + n);
        float v[4] = {acc[i][j][4 * g] + bb.x, acc[i][j][4 * g + 1] + bb.y, acc[i][j][4 * g + 2] + bb.z, acc[i][j][4 * g + 3] + bb.w};
        if (p.relu) {
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = fmaxf(v[k], 0.f);
        }
        if (p.res) {
          const h16x4 rr = *(const h16x4*)((const _Float16*)p.res + m * p.ld_res + n);
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] += (float)rr[k];
        }
        const h16x4 hv = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
        *(h16x4*)((_Float16*)p.out + m * p.ld_out + n) = hv;
      }
  }
}

struct pool_args {
  const _Float16* src;
  _Float16* dst;
  int H, W, Ho, Wo, C8, ld_src, ld_dst;
  int64_t total;
};

__global__ __launch_bounds__(256) void pool_kernel(const pool_args a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.total) return;
  const int q = (int)(e % a.C8);
  const int64_t pix = e / a.C8;
  const int x = (int)(pix % a.Wo), y = (int)((pix / a.Wo) % a.Ho), b = (int)(pix / ((int64_t)a.Wo * a.Ho));
  const int ph = a.H & 1, pw = a.W & 1;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int sy = 2 * y - ph + i, sx = 2 * x - pw + j;
      if (sy < 0 || sy >= a.H || sx < 0 || sx >= a.W) continue;
      const h16x8 v = *(const h16x8*)(a.src + ((int64_t)(b * a.H + sy) * a.W + sx) * a.ld_src + q * 8);
#pragma unroll
      for (int k = 0; k < 8; ++k) s[k] += (float)v[k];
    }
  h16x8 o;
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = (_Float16)(s[k] * 0.25f);
  *(h16x8*)(a.dst + pix * a.ld_dst + q * 8) = o;
}

struct unshuffle_args {
  const float* src;
  _Float16* dst;
  int64_t sb, sc, sy, sx, total;
  int Ch, Ca, r, Ho, Wo, ld;
};

__global__ __launch_bounds__(256) void unshuffle_kernel(const unshuffle_args a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.total) return;
  const int k = (int)(e % a.ld), rr = a.r * a.r;
  const int64_t pix = e / a.ld;
  const int X = (int)(pix % a.Wo), Y = (int)((pix / a.Wo) % a.Ho), b = (int)(pix / ((int64_t)a.Wo * a.Ho));
  float v = 0.f;
  if (k < a.Ca * rr) {
    const int c = k / rr, dy = (k % rr) / a.r, dx = k % a.r;
    const float* const s = a.src + b * a.sb + (int64_t)(Y * a.r + dy) * a.sy + (int64_t)(X * a.r + dx) * a.sx;
    if (a.Ca == a.Ch) {
      v = s[c * a.sc];
    } else {
      float sum = 0.f;
      for (int ch = 0; ch < a.Ch; ++ch) sum += s[ch * a.sc];
      v = sum / (float)a.Ch;
    }
  }
  a.dst[e] = (_Float16)v;
}

struct emit_args {
  const _Float16* src;
  void* dst;
  int64_t per_copy, total;      // N P C / 8 and the same: one thread per 8 channels of a source pixel
  int C8, ld_src, copies, f32;
  float strength;
};

__global__ __launch_bounds__(256) void emit_kernel(const emit_args a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.total) return;
  const int q = (int)(e % a.C8);
  const int64_t pix = e / a.C8;
  const h16x8 v = *(const h16x8*)(a.src + pix * a.ld_src + q * 8);
  float f[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) f[k] = a.strength * (float)v[k];
  for (int c = 0; c < a.copies; ++c) {
    const int64_t o = (c * a.per_copy + e) * 8;
    if (a.f32) {
      float* const d = (float*)a.dst + o;
      *(float4*)d = make_float4(f[0], f[1], f[2], f[3]);
      *(float4*)(d + 4) = make_float4(f[4], f[5], f[6], f[7]);
    } else {
      h16x8 hv;
#pragma unroll
      for (int k = 0; k < 8; ++k) hv[k] = (_Float16)f[k];
      *(h16x8*)((_Float16*)a.dst + o) = hv;
    }
  }
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

bool wide_form(const sr_t2i_conv& L) { return (int64_t)L.H * L.W >= 1024 && L.Cout % 64 == 0; }

int check_layer(const sr_t2i_conv& L, int i) {
  if (!L.src || !L.w || !L.bias || !L.out) SR_FAIL(SR_ERR_INVALID, "sr_t2i_run: layer %d: null src, w, bias or out", i);
  if (L.B < 1 || L.H < 1 || L.W < 1 || L.Hs < 1 || L.Ws < 1) SR_FAIL(SR_ERR_INVALID, "sr_t2i_run: layer %d: sizes (%d, %d, %d from %d, %d) must be positive", i, L.B, L.H, L.W, L.Hs, L.Ws);
  if (L.Cin < 32 || L.Cin % 32 || L.Cin > SR_T2I_MAX_C || L.Cout < 32 || L.Cout % 32 || L.Cout > SR_T2I_MAX_C)
    SR_FAIL(SR_ERR_INVALID, "sr_t2i_run: layer %d: Cin = %d and Cout = %d must be multiples of 32 in 32..%d", i, L.Cin, L.Cout, (int)SR_T2I_MAX_C);
  if ((L.ksize != 1 && L.ksize != 3) || (L.stride != 1 && L.stride != 2) || (L.ksize == 1 && L.stride != 1))
    SR_FAIL(SR_ERR_INVALID, "sr_t2i_run: layer %d: ksize = %d, stride = %d (3x3 at stride 1 or 2, 1x1 at stride 1)", i, L.ksize, L.stride);
  if (L.H != (L.Hs + L.stride - 1) / L.stride || L.W != (L.Ws + L.stride - 1) / L.stride)
    SR_FAIL(SR_ERR_INVALID, "sr_t2i_run: layer %d: a %d x %d source at stride %d does not give %d x %d", i, L.Hs, L.Ws, L.stride, L.H, L.W);
  if (L.relu != 0 && L.relu != 1) SR_FAIL(SR_ERR_INVALID, "sr_t2i_run: layer %d: relu = %d", i, L.relu);
  const int64_t pix = (int64_t)L.B * L.H * L.W, spix = (int64_t)L.B * L.Hs * L.Ws, lim = (int64_t)1 << 31;
  auto pitch_ok = [&](int ld, int need, int64_t px) { return ld >= need && ld % 8 == 0 && px * ld < lim; };
  if (!pitch_ok(L.ld_in, L.Cin, spix)) SR_FAIL(SR_ERR_INVALID, "sr_t2i_run: layer %d: ld_in = %d (Cin = %d; a multiple of 8; B Hs Ws ld < 2^31)", i, L.ld_in, L.Cin);
  if (!pitch_ok(L.ld_out, L.Cout, pix)) SR_FAIL(SR_ERR_INVALID, "sr_t2i_run: layer %d: ld_out = %d (Cout = %d; a multiple of 8; B H W ld < 2^31)", i, L.ld_out, L.Cout);
  if (L.res && !pitch_ok(L.ld_res, L.Cout, pix)) SR_FAIL(SR_ERR_INVALID, "sr_t2i_run: layer %d: ld_res = %d (Cout = %d; a multiple of 8; B H W ld < 2^31)", i, L.ld_res, L.Cout);
  if (!aligned16(L.src) || !aligned16(L.w) || !aligned16(L.bias) || !aligned16(L.out) || !aligned16(L.res))
    SR_FAIL(SR_ERR_INVALID, "sr_t2i_run: layer %d: src, w, bias, out and res must be 16-byte aligned", i);
  return SR_OK;
}

}  // namespace

extern "C" int64_t sr_t2i_packed_index(int32_t Cout, int32_t Cin, int32_t ksize, int32_t n, int32_t c, int32_t ky, int32_t kx) {
  if (Cout < 32 || Cout % 32 || Cin < 32 || Cin % 32 || (ksize != 1 && ksize != 3) || n < 0 || n >= Cout || c < 0 || c >= Cin || ky < 0 ||
      ky >= ksize || kx < 0 || kx >= ksize)
    return -1;
  const int64_t frag = ((int64_t)(ky * ksize + kx) * (Cin / 16) + c / 16) * (Cout / 32) + n / 32;
  return frag * 512 + (((c % 16) / 8) * 32 + n % 32) * 8 + c % 8;
}

extern "C" int sr_t2i_run(const sr_t2i_conv* layers, int32_t n, void* stream) {
  if (!layers || n < 1 || n > SR_T2I_MAX_LAYERS) SR_FAIL(SR_ERR_INVALID, "sr_t2i_run: null layers or n = %d not in 1..%d", n, (int)SR_T2I_MAX_LAYERS);
  for (int i = 0; i < n; ++i) {
    const int rc = check_layer(layers[i], i);
    if (rc != SR_OK) return rc;
  }
  for (int i = 0; i < n; ++i) {
    const sr_t2i_conv& L = layers[i];
    const int64_t M = (int64_t)L.B * L.H * L.W;
    if (wide_form(L)) {
      const dim3 grid((unsigned)((M + 63) / 64), (unsigned)(L.Cout / 64));
      hipLaunchKernelGGL((conv_kernel<2, 2>), grid, dim3(64), 0, sr_stream(stream), L);
    } else {
      const dim3 grid((unsigned)((M + 31) / 32), (unsigned)(L.Cout / 32));
      hipLaunchKernelGGL((conv_kernel<1, 1>), grid, dim3(64), 0, sr_stream(stream), L);
    }
    SR_CHECK_LAUNCH("sr_t2i_run");
  }
  return SR_OK;
}

extern "C" int sr_t2i_pool(const void* src, void* dst, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ld_src, int32_t ld_dst, void* stream) {
  if (!src || !dst) SR_FAIL(SR_ERR_INVALID, "sr_t2i_pool: null pointer");
  if (B < 1 || H < 1 || W < 1 || C < 8 || C % 8) SR_FAIL(SR_ERR_INVALID, "sr_t2i_pool: sizes (%d, %d, %d) must be positive and C = %d a multiple of 8", B, H, W, C);
  if (ld_src < C || ld_src % 8 || ld_dst < C || ld_dst % 8) SR_FAIL(SR_ERR_INVALID, "sr_t2i_pool: ld_src = %d, ld_dst = %d (multiples of 8, >= C = %d)", ld_src, ld_dst, C);
  if (!aligned16(src) || !aligned16(dst)) SR_FAIL(SR_ERR_INVALID, "sr_t2i_pool: src and dst must be 16-byte aligned");
  const int64_t lim = (int64_t)1 << 31;
  pool_args a;
  a.src = (const _Float16*)src; a.dst = (_Float16*)dst; a.H = H; a.W = W; a.Ho = (H + 1) / 2; a.Wo = (W + 1) / 2; a.C8 = C / 8;
  a.ld_src = ld_src; a.ld_dst = ld_dst;
  if ((int64_t)B * H * W * ld_src >= lim || (int64_t)B * a.Ho * a.Wo * ld_dst >= lim) SR_FAIL(SR_ERR_INVALID, "sr_t2i_pool: B H W ld is not below 2^31");
  a.total = (int64_t)B * a.Ho * a.Wo * a.C8;
  hipLaunchKernelGGL(pool_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, sr_stream(stream), a);
  SR_CHECK_LAUNCH("sr_t2i_pool");
  return SR_OK;
}

extern "C" int sr_t2i_unshuffle(const float* src, int64_t sb, int64_t sc, int64_t sy, int64_t sx, int32_t B, int32_t Ch, int32_t H, int32_t W,
                                int32_t Ca, int32_t r, void* dst, int32_t ld_dst, void* stream) {
  if (!src || !dst) SR_FAIL(SR_ERR_INVALID, "sr_t2i_unshuffle: null pointer");
  if (r != 8 && r != 16) SR_FAIL(SR_ERR_INVALID, "sr_t2i_unshuffle: r = %d must be 8 or 16", r);
  if (B < 1 || Ch < 1 || H < r || W < r || H % r || W % r) SR_FAIL(SR_ERR_INVALID, "sr_t2i_unshuffle: sizes (%d, %d, %d, %d): H and W must be positive multiples of r = %d", B, Ch, H, W, r);
  if (Ca != Ch && Ca != 1) SR_FAIL(SR_ERR_INVALID, "sr_t2i_unshuffle: Ca = %d must be Ch = %d or 1", Ca, Ch);
  if (sb < 0 || sc < 0 || sy < 0 || sx < 0) SR_FAIL(SR_ERR_INVALID, "sr_t2i_unshuffle: negative stride");
  if (ld_dst % 8 || (int64_t)Ca * r * r > ld_dst) SR_FAIL(SR_ERR_INVALID, "sr_t2i_unshuffle: ld_dst = %d must be a multiple of 8 and hold %d channels", ld_dst, Ca * r * r);
  if (((uintptr_t)src & 3) != 0 || !aligned16(dst)) SR_FAIL(SR_ERR_INVALID, "sr_t2i_unshuffle: src must be 4-byte and dst 16-byte aligned");
  unshuffle_args a;
  a.src = src; a.dst = (_Float16*)dst; a.sb = sb; a.sc = sc; a.sy = sy; a.sx = sx; a.Ch = Ch; a.Ca = Ca; a.r = r;
  a.Ho = H / r; a.Wo = W / r; a.ld = ld_dst;
  a.total = (int64_t)B * a.Ho * a.Wo * ld_dst;
  if (a.total >= ((int64_t)1 << 31)) SR_FAIL(SR_ERR_INVALID, "sr_t2i_unshuffle: B (H / r) (W / r) ld = %lld is not below 2^31", (long long)a.total);
  hipLaunchKernelGGL(unshuffle_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, sr_stream(stream), a);
  SR_CHECK_LAUNCH("sr_t2i_unshuffle");
  return SR_OK;
}

extern "C" int sr_t2i_emit(const void* src, int32_t ld_src, void* dst, int32_t dst_f32, int32_t N, int32_t P, int32_t C, int32_t copies,
                           float strength, void* stream) {
  if (!src || !dst) SR_FAIL(SR_ERR_INVALID, "sr_t2i_emit: null pointer");
  if (N < 1 || P < 1 || C < 8 || C % 8 || copies < 1) SR_FAIL(SR_ERR_INVALID, "sr_t2i_emit: sizes (%d, %d, %d) and copies = %d must be positive, C a multiple of 8", N, P, C, copies);
  if (ld_src < C || ld_src % 8) SR_FAIL(SR_ERR_INVALID, "sr_t2i_emit: ld_src = %d (a multiple of 8, >= C = %d)", ld_src, C);
  if (dst_f32 != 0 && dst_f32 != 1) SR_FAIL(SR_ERR_INVALID, "sr_t2i_emit: dst_f32 = %d", dst_f32);
  if (!(strength == strength) || strength - strength != 0.f) SR_FAIL(SR_ERR_INVALID, "sr_t2i_emit: strength = %g is not finite", (double)strength);
  if (!aligned16(src) || !aligned16(dst)) SR_FAIL(SR_ERR_INVALID, "sr_t2i_emit: src and dst must be 16-byte aligned");
  const int64_t lim = (int64_t)1 << 31;
  if ((int64_t)copies * N * P * C >= lim || (int64_t)N * P * ld_src >= lim) SR_FAIL(SR_ERR_INVALID, "sr_t2i_emit: copies N P C is not below 2^31");
  emit_args a;
  a.src = (const _Float16*)src; a.dst = dst; a.C8 = C / 8; a.ld_src = ld_src; a.copies = copies; a.f32 = dst_f32; a.strength = strength;
  a.per_copy = (int64_t)N * P * a.C8; a.total = a.per_copy;
  hipLaunchKernelGGL(emit_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, sr_stream(stream), a);
  SR_CHECK_LAUNCH("sr_t2i_emit");
  return SR_OK;
}
