// libsr_taesd.so: the 3x3 convolution of the TAESD tiny autoencoder as one patch-stationary implicit-GEMM kernel, and the packing
// of the network's input (sr_taesd.h).  Modelled on conv3_kernel of csrc/esrgan/esrgan.hip, which stays as it is.
//
// Every layer of the network is a 3x3 convolution of 32 or 64 channels into 32 or 64, so N is one or two MFMA tiles and the work
// is in the activation path:
//   a workgroup (4 waves) owns a patch of output pixels of one image, 32 wide.  Per 32-channel chunk of the input it stages the
//   source pixels the patch's nine taps touch into LDS once (global -> registers -> LDS; the next chunk's loads are in flight
//   during this chunk's MFMAs), and the nine taps read it at nine constant offsets.  Pixels outside the source map are zeros in
//   LDS, so a halo never reaches a neighbouring image.  LDS pitch 80 B per pixel (64 B of channels + 16 B): the 16 lanes that a
//   ds_read_b128 serves together read 16 consecutive staged pixels, 80 B apart, which fall on 16 distinct 16-byte bank groups
//   (5 is coprime to 16).
//   MFMA 32x32x16 f16 with the WEIGHTS as the A operand (rows = output channels) and the pixels as B (columns): a lane then holds
//   runs of four consecutive output channels of one pixel, which are 8-byte stores into NHWC and 8-byte loads of the residual.
//   Weights are not staged: every workgroup reads the same <= 72 KB per layer, packed so that a lane's fragment is 16 contiguous
//   bytes, one tap ahead of its use.
// The three read modes:
//   stride 1          a patch of 8 x 32 pixels, a wave computes two rows; 10 x 34 staged pixels, two LDS buffers, one barrier per chunk.
//   up = 2            the same patch; a staged pixel (y, x) is loaded from the half-size source at (y >> 1, x >> 1).
//   stride 2          a lane's 32 pixels read source columns 2 apart, so a tap is no constant offset in a row-major image.  Chosen
//                     here: DE-INTERLEAVE THE COLUMNS BY PARITY WHILE STAGING.  A staged row of 65 source columns (2 x0 - 1 ..
//                     2 x0 + 63) is stored as its 33 even-indexed columns followed by its 32 odd-indexed ones; tap kx = 0 / 1 / 2 of
//                     output pixel r is then entry r of the even plane / r of the odd plane / r + 1 of the even plane: constant
//                     offsets again, the same conflict-free 80-byte walk, and the MFMA loop is the stride-1 loop with another
//                     offset table.  The patch is 4 x 32 (a wave computes one row) so that the 9 x 65 staged pixels are 46.8 KB;
//                     they are single-buffered (a second barrier per chunk) because the three stride-2 layers of the encoder are
//                     a few percent of its work: the smaller patch alone would have needed a second lane-to-pixel map, the
//                     de-interleave keeps one.
// No split-K, no atomics: the sum order of an output element is fixed by the layer's shape alone.
#include <cstdint>
#include "sr_taesd.h"
#define SR_SIDE taesd
#define SR_SIDE_UC TAESD
#ifndef SR_TAESD_SRC_HASH
#define SR_TAESD_SRC_HASH "unstamped"
#endif
#include "../sr_side.h"
#include "../conv3_pack.h"

namespace {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int PW = 32, PITCH = 80, THREADS = 256;

// the geometry of a read mode: S = 1 (stride 1, with or without the fused upsample) or 2 (stride 2)
template <int S>
struct geo {
  static constexpr int ROWS = S == 2 ? 1 : 2;                       // output rows per wave
  static constexpr int PH = 4 * ROWS;                               // output rows per workgroup
  static constexpr int SH = S == 2 ? 2 * PH + 1 : PH + 2;           // staged source rows
  static constexpr int SW = S == 2 ? 2 * PW + 1 : PW + 2;           // staged source columns
  static constexpr int EVEN = PW + 1;                               // S = 2: entries of the even plane of a staged row
  static constexpr int HPIX = SH * SW, ABYTES = HPIX * PITCH, SLOTS = HPIX * 4;
  static constexpr int SPT = (SLOTS + THREADS - 1) / THREADS;       // 16-byte slots per thread and chunk
  static constexpr int NBUF = S == 2 ? 1 : 2;
  // where the staged pixel (hy, hx) lies in LDS, in pixels
  static __device__ __forceinline__ int at(int hy, int hx) { return S == 2 ? hy * SW + ((hx & 1) ? EVEN : 0) + (hx >> 1) : hy * SW + hx; }
  // where tap (ky, kx) of the output pixel (row yl of the patch, column 0) lies, in pixels; column r is r entries further
  static __device__ __forceinline__ int tap(int yl, int ky, int kx) {
    return S == 2 ? (2 * yl + ky) * SW + (kx == 1 ? EVEN : 0) + (kx == 2 ? 1 : 0) : (yl + ky) * SW + kx;
  }
};

template <int NT, int S>
__global__ __launch_bounds__(THREADS) void conv3_kernel(const sr_tae_conv p) {
  using G = geo<S>;
  __shared__ __attribute__((aligned(16))) char smem[G::NBUF * G::ABYTES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  const int H = p.H, W = p.W, Hs = p.Hs, Ws = p.Ws, ptx = (W + PW - 1) / PW;
  const int b = blockIdx.y, y0 = ((int)blockIdx.x / ptx) * G::PH, x0 = ((int)blockIdx.x % ptx) * PW;
  const int sh = p.up == 2 ? 1 : 0;
  const _Float16* const in = (const _Float16*)p.src;

  // the staged slots of this thread: element offset of the slot's first channel in chunk 0 (< 2^31 by the host's check), -1 = zeros,
  // and the slot's byte offset in an LDS buffer
  int soff[G::SPT], loff[G::SPT];
#pragma unroll
  for (int i = 0; i < G::SPT; ++i) {
    const int u = tid + i * THREADS, hp = u >> 2, q = u & 3, hy = hp / G::SW, hx = hp - hy * G::SW;
    bool ok = u < G::SLOTS;
    int ys, xs;
    if (S == 2) {
      ys = 2 * y0 - 1 + hy;
      xs = 2 * x0 - 1 + hx;
      ok = ok && ys >= 0 && ys < Hs && xs >= 0 && xs < Ws;
    } else {
      const int y = y0 + hy - 1, x = x0 + hx - 1;
      ok = ok && y >= 0 && y < H && x >= 0 && x < W;
      ys = y >> sh;
      xs = x >> sh;
    }
    soff[i] = ok ? ((b * Hs + ys) * Ws + xs) * p.ld_in + q * 8 : -1;
    loff[i] = G::at(hy, hx) * PITCH + q * 16;
  }
  uint4 st[G::SPT];
  auto load_chunk = [&](int c) {
#pragma unroll
    for (int i = 0; i < G::SPT; ++i)
      st[i] = soff[i] >= 0 ? *(const uint4*)(in + ((int64_t)soff[i] + c * 32)) : make_uint4(0, 0, 0, 0);
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int i = 0; i < G::SPT; ++i)
      if (tid + i * THREADS < G::SLOTS) *(uint4*)(smem + buf * G::ABYTES + loff[i]) = st[i];
  };

  const _Float16* const wl = (const _Float16*)p.w + lane * 8;
  h16x8 wcur[2][NT], wnext[2][NT];
  auto load_w = [&](h16x8 (&wf)[2][NT], int s) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) wf[ks][nt] = *(const h16x8*)(wl + (int64_t)((s * 2 + ks) * NT + nt) * 512);
  };

  f32x16 acc[G::ROWS][NT];
#pragma unroll
  for (int i = 0; i < G::ROWS; ++i)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[i][nt][k] = 0.f;

  const int NC = p.Cin / 32, steps = NC * 9;
  load_chunk(0);
  load_w(wcur, 0);
  store_chunk(0);
  __syncthreads();
  // this lane's B fragment: pixel r of the wave's rows, k half h
  const int xoff = r * PITCH + h * 16;
  for (int c = 0; c < NC; ++c) {
    if (c + 1 < NC) load_chunk(c + 1);
    const char* const A = smem + (G::NBUF == 2 ? (c & 1) * G::ABYTES : 0) + xoff;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int s = c * 9 + t;
      if (s + 1 < steps) load_w(wnext, s + 1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < G::ROWS; ++i) {
          const h16x8 xf = *(const h16x8*)(A + G::tap(G::ROWS * wv + i, t / 3, t % 3) * PITCH + ks * 32);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[i][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wcur[ks][nt], xf, acc[i][nt], 0, 0, 0);
        }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wcur[ks][nt] = wnext[ks][nt];
    }
    if (G::NBUF == 1) __syncthreads();               // one buffer: every wave has left chunk c before it is overwritten
    if (c + 1 < NC) store_chunk(G::NBUF == 2 ? (c + 1) & 1 : 0);     // two buffers: last read in chunk c - 1, left at the barrier below
    __syncthreads();
  }

  // epilogue: register 4g + k of a lane is output channel nt * 32 + 8g + 4h + k of pixel r
  const int x = x0 + r;
#pragma unroll
  for (int i = 0; i < G::ROWS; ++i) {
    const int y = y0 + G::ROWS * wv + i;
    if (y >= H || x >= W) continue;
    const int64_t m = ((int64_t)b * H + y) * W + x;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = nt * 32 + 8 * g + 4 * h;
        const float4 bb = *(const float4*)(p.bias + n);
        float v[4] = {acc[i][nt][4 * g] + bb.x, acc[i][nt][4 * g + 1] + bb.y, acc[i][nt][4 * g + 2] + bb.z, acc[i][nt][4 * g + 3] + bb.w};
        if (p.relu) {
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = fmaxf(v[k], 0.f);
        }
        if (p.res) {
          const h16x4 rr = *(const h16x4*)((const _Float16*)p.res + m * p.ld_res + n);
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] += (float)rr[k];
        }
        if (p.relu_after) {
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = fmaxf(v[k], 0.f);
        }
        if (p.out_f32) {
          float* const o = p.out_f32 + ((int64_t)b * p.ob + (int64_t)y * p.oy + (int64_t)x * p.ox);
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (n + k < p.n_store) {
              const float s = p.a * v[k];
              o[(int64_t)(n + k) * p.oc] = p.clamp ? fminf(fmaxf(s, 0.f), 1.f) : s;
            }
        } else {
          const h16x4 hv = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
          *(h16x4*)((_Float16*)p.out + m * p.ld_out + p.c_off + n) = hv;
        }
      }
  }
}

struct pack_args {
  const float* src;
  _Float16* dst;
  int64_t sb, sy, sx, sc, total;
  int H, W, C, ld, clamp3;
  float a;
};

__global__ __launch_bounds__(256) void pack_input_kernel(const pack_args a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.total) return;
  const int ch = (int)(e % a.ld);
  const int64_t pix = e / a.ld;
  const int x = (int)(pix % a.W), y = (int)((pix / a.W) % a.H), b = (int)(pix / ((int64_t)a.W * a.H));
  float v = 0.f;
  if (ch < a.C) {
    v = a.src[b * a.sb + y * a.sy + x * a.sx + ch * a.sc] * a.a;
    if (a.clamp3) v = 3.f * tanhf(v / 3.f);
  }
  a.dst[e] = (_Float16)v;
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

int check_layer(const sr_tae_conv& L, int i) {
  if (!L.src || !L.w || !L.bias || (!L.out && !L.out_f32)) SR_FAIL(SR_ERR_INVALID, "sr_tae_run: layer %d: null src, w, bias or output", i);
  if (L.B < 1 || L.H < 1 || L.W < 1 || L.B > 65535) SR_FAIL(SR_ERR_INVALID, "sr_tae_run: layer %d: sizes (%d, %d, %d) must be positive (B <= 65535)", i, L.B, L.H, L.W);
  if ((L.Cin != 32 && L.Cin != 64) || (L.Cout != 32 && L.Cout != 64)) SR_FAIL(SR_ERR_INVALID, "sr_tae_run: layer %d: Cin = %d and Cout = %d must be 32 or 64", i, L.Cin, L.Cout);
  if ((L.up != 1 && L.up != 2) || (L.stride != 1 && L.stride != 2) || (L.up == 2 && L.stride == 2))
    SR_FAIL(SR_ERR_INVALID, "sr_tae_run: layer %d: up = %d, stride = %d (each 1 or 2, not both 2)", i, L.up, L.stride);
  if (L.up == 2) {
    if (((L.H | L.W) & 1) || L.Hs != L.H / 2 || L.Ws != L.W / 2)
      SR_FAIL(SR_ERR_INVALID, "sr_tae_run: layer %d: up = 2 wants an even output of twice the source, not %d x %d from %d x %d", i, L.H, L.W, L.Hs, L.Ws);
  } else if (L.stride == 2) {
    if (L.Hs < 2 || L.Ws < 2 || ((L.Hs | L.Ws) & 1) || L.Hs != 2 * L.H || L.Ws != 2 * L.W)
      SR_FAIL(SR_ERR_INVALID, "sr_tae_run: layer %d: stride = 2 wants an even source of twice the output, not %d x %d into %d x %d", i, L.Hs, L.Ws, L.H, L.W);
  } else if (L.Hs != L.H || L.Ws != L.W) {
    SR_FAIL(SR_ERR_INVALID, "sr_tae_run: layer %d: the source %d x %d is not the output %d x %d", i, L.Hs, L.Ws, L.H, L.W);
  }
  if ((L.relu != 0 && L.relu != 1) || (L.relu_after != 0 && L.relu_after != 1)) SR_FAIL(SR_ERR_INVALID, "sr_tae_run: layer %d: relu = %d, relu_after = %d", i, L.relu, L.relu_after);
  const int64_t pix = (int64_t)L.B * L.H * L.W, spix = (int64_t)L.B * L.Hs * L.Ws, lim = (int64_t)1 << 31;
  auto pitch_ok = [&](int ld, int need, int64_t px) { return ld >= need && ld % 8 == 0 && px * ld < lim; };
  if (!pitch_ok(L.ld_in, L.Cin, spix)) SR_FAIL(SR_ERR_INVALID, "sr_tae_run: layer %d: ld_in = %d (Cin = %d; a multiple of 8; B Hs Ws ld < 2^31)", i, L.ld_in, L.Cin);
  if (!aligned16(L.src) || !aligned16(L.w) || !aligned16(L.bias)) SR_FAIL(SR_ERR_INVALID, "sr_tae_run: layer %d: src, w and bias must be 16-byte aligned", i);
  if (L.out_f32) {
    if (L.n_store < 1 || L.n_store > L.Cout) SR_FAIL(SR_ERR_INVALID, "sr_tae_run: layer %d: n_store = %d", i, L.n_store);
    if (L.ob < 1 || L.oy < 1 || L.ox < 1 || L.oc < 1) SR_FAIL(SR_ERR_INVALID, "sr_tae_run: layer %d: the strides of out_f32 must be positive", i);
    if (((uintptr_t)L.out_f32 & 3) != 0) SR_FAIL(SR_ERR_INVALID, "sr_tae_run: layer %d: out_f32 must be 4-byte aligned", i);
    if ((L.clamp != 0 && L.clamp != 1) || !(L.a == L.a) || L.a - L.a != 0.f) SR_FAIL(SR_ERR_INVALID, "sr_tae_run: layer %d: clamp = %d, a = %g", i, L.clamp, (double)L.a);
  } else {
    if (L.c_off < 0 || L.c_off % 8 || (int64_t)L.c_off + L.Cout > L.ld_out || !pitch_ok(L.ld_out, L.Cout, pix))
      SR_FAIL(SR_ERR_INVALID, "sr_tae_run: layer %d: c_off = %d, Cout = %d, ld_out = %d (the slice lies inside a row; multiples of 8; B H W ld < 2^31)", i, L.c_off, L.Cout, L.ld_out);
    if (!aligned16(L.out)) SR_FAIL(SR_ERR_INVALID, "sr_tae_run: layer %d: out must be 16-byte aligned", i);
  }
  if (L.res && (!pitch_ok(L.ld_res, L.Cout, pix) || !aligned16(L.res))) SR_FAIL(SR_ERR_INVALID, "sr_tae_run: layer %d: ld_res = %d or a misaligned res", i, L.ld_res);
  return SR_OK;
}

template <int S>
void launch(const sr_tae_conv& L, hipStream_t st) {
  const dim3 grid((unsigned)(((L.W + PW - 1) / PW) * ((L.H + geo<S>::PH - 1) / geo<S>::PH)), (unsigned)L.B);
  if (L.Cout == 32) hipLaunchKernelGGL((conv3_kernel<1, S>), grid, dim3(THREADS), 0, st, L);
  else hipLaunchKernelGGL((conv3_kernel<2, S>), grid, dim3(THREADS), 0, st, L);
}

}  // namespace

extern "C" int64_t sr_tae_packed_index(int32_t Cout, int32_t Cin, int32_t n, int32_t c, int32_t ky, int32_t kx) {
  return conv3_packed_index(Cout, Cin, n, c, ky, kx);
}

extern "C" int sr_tae_run(const sr_tae_conv* layers, int32_t n, void* stream) {
  if (!layers || n < 1 || n > SR_TAE_MAX_LAYERS) SR_FAIL(SR_ERR_INVALID, "sr_tae_run: null layers or n = %d not in 1..%d", n, (int)SR_TAE_MAX_LAYERS);
  for (int i = 0; i < n; ++i) {
    const int rc = check_layer(layers[i], i);
    if (rc != SR_OK) return rc;
  }
  for (int i = 0; i < n; ++i) {
    if (layers[i].stride == 2) launch<2>(layers[i], sr_stream(stream));
    else launch<1>(layers[i], sr_stream(stream));
    SR_CHECK_LAUNCH("sr_tae_run");
  }
  return SR_OK;
}

extern "C" int sr_tae_pack_input(const float* src, int64_t sb, int64_t sy, int64_t sx, int64_t sc, int32_t B, int32_t H, int32_t W,
                                 int32_t C, float a, int32_t clamp3, void* dst, int32_t ld_dst, void* stream) {
  if (!src || !dst) SR_FAIL(SR_ERR_INVALID, "sr_tae_pack_input: null pointer");
  if (B < 1 || H < 1 || W < 1 || C < 1) SR_FAIL(SR_ERR_INVALID, "sr_tae_pack_input: sizes (%d, %d, %d, %d) must be positive", B, H, W, C);
  if (sb < 0 || sy < 0 || sx < 0 || sc < 0) SR_FAIL(SR_ERR_INVALID, "sr_tae_pack_input: negative stride");
  if (clamp3 != 0 && clamp3 != 1) SR_FAIL(SR_ERR_INVALID, "sr_tae_pack_input: clamp3 = %d", clamp3);
  if (!(a == a) || a - a != 0.f) SR_FAIL(SR_ERR_INVALID, "sr_tae_pack_input: a = %g is not finite", (double)a);
  if (ld_dst % 8 || C > ld_dst) SR_FAIL(SR_ERR_INVALID, "sr_tae_pack_input: ld_dst = %d must be a multiple of 8 and hold %d channels", ld_dst, C);
  if (((uintptr_t)src & 3) != 0 || !aligned16(dst)) SR_FAIL(SR_ERR_INVALID, "sr_tae_pack_input: src must be 4-byte and dst 16-byte aligned");
  pack_args p;
  p.src = src; p.dst = (_Float16*)dst; p.sb = sb; p.sy = sy; p.sx = sx; p.sc = sc;
  p.H = H; p.W = W; p.C = C; p.ld = ld_dst; p.clamp3 = clamp3; p.a = a;
  p.total = (int64_t)B * H * W * ld_dst;
  if (p.total >= ((int64_t)1 << 31)) SR_FAIL(SR_ERR_INVALID, "sr_tae_pack_input: B H W ld = %lld is not below 2^31", (long long)p.total);
  hipLaunchKernelGGL(pack_input_kernel, dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, sr_stream(stream), p);
  SR_CHECK_LAUNCH("sr_tae_pack_input");
  return SR_OK;
}
