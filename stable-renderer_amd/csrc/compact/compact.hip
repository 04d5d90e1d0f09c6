// libsr_compact.so: the 3x3 convolution of the Real-ESRGAN compact (SRVGG) upscale models as one patch-stationary implicit-GEMM
// kernel, and the packing of the network's input (sr_compact.h).  The main loop is the stride-1 loop of csrc/taesd/taesd.hip
// (itself modelled on csrc/esrgan/esrgan.hip), copied: both files stay as they are.  The epilogues are this file's own.
//
// Every layer of the network is a 3x3 convolution of 32 or 64 channels into 32 or 64 at the LOW resolution, so N is one or two MFMA
// tiles and the work is in the activation path:
//   a workgroup (4 waves) owns a patch of 8 x 32 output pixels of one image, a wave two rows of it.  Per 32-channel chunk of the
//   input it stages the 10 x 34 source pixels the patch's nine taps touch into LDS once (global -> registers -> LDS; the next
//   chunk's loads are in flight during this chunk's MFMAs; two LDS buffers, one barrier per chunk), and the nine taps read it at nine
//   constant offsets.  Pixels outside the map are zeros in LDS, so a halo never reaches a neighbouring image.  LDS pitch 80 B per
//   pixel (64 B of channels + 16 B): the 16 lanes that a ds_read_b128 serves together read 16 consecutive staged pixels, 80 B apart,
//   which fall on 16 distinct 16-byte bank groups (5 is coprime to 16).  2 x 27.2 KB per workgroup: two workgroups per CU.
//   MFMA 32x32x16 f16 with the WEIGHTS as the A operand (rows = output channels) and the pixels as B (columns): a lane then holds
//   runs of four consecutive output channels of one pixel, which are 8-byte stores into NHWC.
//   Weights are not staged: every workgroup reads the same <= 72 KB per layer, packed so that a lane's fragment is 16 contiguous
//   bytes, one tap ahead of its use.
// One launch per layer: the layers of a model are dependent through a one-pixel halo, and a launch of 64 x 64 channels over a 512^2
// tile is 1024 workgroups, four per CU.
// The epilogues, in fp32 on the accumulators:
//   PReLU        v >= 0 ? v : slope[n] * v, the slope per output channel.
//   fp16 store   four channels of a pixel as one 8-byte store into the slice [c_off, c_off + Cout).
//   shuffle      the last layer: channel n = c s^2 + dy s + dx of low-resolution pixel (y, x) is channel c of the result's pixel
//                (y s + dy, x s + dx), stored as fp32 together with the caller's own fp32 input at (y, x, c) (the network's residual
//                base, nearest-upsampled by the same index arithmetic).  PixelShuffle and the add never exist as passes of their own.
// No split-K, no atomics: the sum order of an output element is fixed by the layer's shape alone.
#include <cstdint>
#include "sr_compact.h"
#define SR_SIDE compact
#define SR_SIDE_UC COMPACT
#ifndef SR_COMPACT_SRC_HASH
#define SR_COMPACT_SRC_HASH "unstamped"
#endif
#include "../sr_side.h"
#include "../conv3_pack.h"

namespace {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int PW = 32, PITCH = 80, THREADS = 256;
constexpr int ROWS = 2;                                 // output rows per wave
constexpr int PH = 4 * ROWS;                            // output rows per workgroup
constexpr int SH = PH + 2, SW = PW + 2;                 // staged source rows and columns
constexpr int HPIX = SH * SW, ABYTES = HPIX * PITCH, SLOTS = HPIX * 4;
constexpr int SPT = (SLOTS + THREADS - 1) / THREADS;    // 16-byte slots per thread and chunk

template <int NT>
__global__ __launch_bounds__(THREADS) void conv3_kernel(const sr_cmp_conv p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * ABYTES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  const int H = p.H, W = p.W, ptx = (W + PW - 1) / PW;
  const int b = blockIdx.y, y0 = ((int)blockIdx.x / ptx) * PH, x0 = ((int)blockIdx.x % ptx) * PW;
  const _Float16* const in = (const _Float16*)p.src;

  // the staged slots of this thread: element offset of the slot's first channel in chunk 0 (< 2^31 by the host's check), -1 = zeros,
  // and the slot's byte offset in an LDS buffer
  int soff[SPT], loff[SPT];
#pragma unroll
  for (int i = 0; i < SPT; ++i) {
    const int u = tid + i * THREADS, hp = u >> 2, q = u & 3, hy = hp / SW, hx = hp - hy * SW;
    const int y = y0 + hy - 1, x = x0 + hx - 1;
    const bool ok = u < SLOTS && y >= 0 && y < H && x >= 0 && x < W;
    soff[i] = ok ? ((b * H + y) * W + x) * p.ld_in + q * 8 : -1;
    loff[i] = (hy * SW + hx) * PITCH + q * 16;
  }
  uint4 st[SPT];
  auto load_chunk = [&](int c) {
#pragma unroll
    for (int i = 0; i < SPT; ++i)
      st[i] = soff[i] >= 0 ? *(const uint4*)(in + ((int64_t)soff[i] + c * 32)) : make_uint4(0, 0, 0, 0);
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int i = 0; i < SPT; ++i)
      if (tid + i * THREADS < SLOTS) *(uint4*)(smem + buf * ABYTES + loff[i]) = st[i];
  };

  const _Float16* const wl = (const _Float16*)p.w + lane * 8;
  h16x8 wcur[2][NT], wnext[2][NT];
  auto load_w = [&](h16x8 (&wf)[2][NT], int s) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) wf[ks][nt] = *(const h16x8*)(wl + (int64_t)((s * 2 + ks) * NT + nt) * 512);
  };

  f32x16 acc[ROWS][NT];
#pragma unroll
  for (int i = 0; i < ROWS; ++i)
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
    const char* const A = smem + (c & 1) * ABYTES + xoff;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int s = c * 9 + t;
      if (s + 1 < steps) load_w(wnext, s + 1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
          const h16x8 xf = *(const h16x8*)(A + ((ROWS * wv + i + t / 3) * SW + t % 3) * PITCH + ks * 32);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[i][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wcur[ks][nt], xf, acc[i][nt], 0, 0, 0);
        }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wcur[ks][nt] = wnext[ks][nt];
    }
    if (c + 1 < NC) store_chunk((c + 1) & 1);          // the other buffer: last read in chunk c - 1, left at the barrier below
    __syncthreads();
  }

  // epilogue: register 4g + k of a lane is output channel nt * 32 + 8g + 4h + k of pixel r
  const int x = x0 + r;
  const int s = p.s, ss = s * s, n_store = p.C * ss;
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int y = y0 + ROWS * wv + i;
    if (y >= H || x >= W) continue;
    const int64_t m = ((int64_t)b * H + y) * W + x;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = nt * 32 + 8 * g + 4 * h;
        const float4 bb = *(const float4*)(p.bias + n);
        float v[4] = {acc[i][nt][4 * g] + bb.x, acc[i][nt][4 * g + 1] + bb.y, acc[i][nt][4 * g + 2] + bb.z, acc[i][nt][4 * g + 3] + bb.w};
        if (p.slope) {
          const float4 sl = *(const float4*)(p.slope + n);
          const float a[4] = {sl.x, sl.y, sl.z, sl.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = v[k] >= 0.f ? v[k] : a[k] * v[k];
        }
        if (p.out_f32) {
          float* const o = p.out_f32 + ((int64_t)b * p.ob + (int64_t)y * s * p.oy + (int64_t)x * s * p.ox);
          const float* const bs = p.base + ((int64_t)b * p.bb + (int64_t)y * p.by + (int64_t)x * p.bx);
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (n + k < n_store) {
              const int c = (n + k) / ss, rem = (n + k) - c * ss, dy = rem / s, dx = rem - dy * s;
              o[(int64_t)dy * p.oy + (int64_t)dx * p.ox + (int64_t)c * p.oc] = v[k] + bs[(int64_t)c * p.bc];
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
  int H, W, C, ld;
};

__global__ __launch_bounds__(256) void pack_input_kernel(const pack_args a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.total) return;
  const int ch = (int)(e % a.ld);
  const int64_t pix = e / a.ld;
  const int x = (int)(pix % a.W), y = (int)((pix / a.W) % a.H), b = (int)(pix / ((int64_t)a.W * a.H));
  a.dst[e] = ch < a.C ? (_Float16)a.src[b * a.sb + y * a.sy + x * a.sx + ch * a.sc] : (_Float16)0.f;
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

int check_layer(const sr_cmp_conv& L, int i) {
  if (!L.src || !L.w || !L.bias || (!L.out && !L.out_f32)) SR_FAIL(SR_ERR_INVALID, "sr_cmp_run: layer %d: null src, w, bias or output", i);
  if (L.B < 1 || L.H < 1 || L.W < 1 || L.B > 65535) SR_FAIL(SR_ERR_INVALID, "sr_cmp_run: layer %d: sizes (%d, %d, %d) must be positive (B <= 65535)", i, L.B, L.H, L.W);
  if ((L.Cin != 32 && L.Cin != 64) || (L.Cout != 32 && L.Cout != 64)) SR_FAIL(SR_ERR_INVALID, "sr_cmp_run: layer %d: Cin = %d and Cout = %d must be 32 or 64", i, L.Cin, L.Cout);
  const int64_t pix = (int64_t)L.B * L.H * L.W, lim = (int64_t)1 << 31;
  auto pitch_ok = [&](int ld, int need) { return ld >= need && ld % 8 == 0 && pix * ld < lim; };
  if (!pitch_ok(L.ld_in, L.Cin)) SR_FAIL(SR_ERR_INVALID, "sr_cmp_run: layer %d: ld_in = %d (Cin = %d; a multiple of 8; B H W ld < 2^31)", i, L.ld_in, L.Cin);
  if (!aligned16(L.src) || !aligned16(L.w) || !aligned16(L.bias) || !aligned16(L.slope)) SR_FAIL(SR_ERR_INVALID, "sr_cmp_run: layer %d: src, w, bias and slope must be 16-byte aligned", i);
  if (L.out_f32) {
    if (!L.base) SR_FAIL(SR_ERR_INVALID, "sr_cmp_run: layer %d: the shuffle store needs base", i);
    if (L.s < 1 || L.s > 4 || L.C < 1 || L.C > 4 || L.C * L.s * L.s > L.Cout)
      SR_FAIL(SR_ERR_INVALID, "sr_cmp_run: layer %d: s = %d, C = %d (each 1..4, C s^2 <= Cout = %d)", i, L.s, L.C, L.Cout);
    if (L.ob < 1 || L.oy < 1 || L.ox < 1 || L.oc < 1) SR_FAIL(SR_ERR_INVALID, "sr_cmp_run: layer %d: the strides of out_f32 must be positive", i);
    if (L.bb < 0 || L.by < 0 || L.bx < 0 || L.bc < 0) SR_FAIL(SR_ERR_INVALID, "sr_cmp_run: layer %d: negative stride of base", i);
    if (((uintptr_t)L.out_f32 & 3) != 0 || ((uintptr_t)L.base & 3) != 0) SR_FAIL(SR_ERR_INVALID, "sr_cmp_run: layer %d: out_f32 and base must be 4-byte aligned", i);
  } else {
    if (L.c_off < 0 || L.c_off % 8 || (int64_t)L.c_off + L.Cout > L.ld_out || !pitch_ok(L.ld_out, L.Cout))
      SR_FAIL(SR_ERR_INVALID, "sr_cmp_run: layer %d: c_off = %d, Cout = %d, ld_out = %d (the slice lies inside a row; multiples of 8; B H W ld < 2^31)", i, L.c_off, L.Cout, L.ld_out);
    if (!aligned16(L.out)) SR_FAIL(SR_ERR_INVALID, "sr_cmp_run: layer %d: out must be 16-byte aligned", i);
  }
  return SR_OK;
}

void launch(const sr_cmp_conv& L, hipStream_t st) {
  const dim3 grid((unsigned)(((L.W + PW - 1) / PW) * ((L.H + PH - 1) / PH)), (unsigned)L.B);
  if (L.Cout == 32) hipLaunchKernelGGL((conv3_kernel<1>), grid, dim3(THREADS), 0, st, L);
  else hipLaunchKernelGGL((conv3_kernel<2>), grid, dim3(THREADS), 0, st, L);
}

}  // namespace

extern "C" int64_t sr_cmp_packed_index(int32_t Cout, int32_t Cin, int32_t n, int32_t c, int32_t ky, int32_t kx) {
  return conv3_packed_index(Cout, Cin, n, c, ky, kx);
}

extern "C" int sr_cmp_run(const sr_cmp_conv* layers, int32_t n, void* stream) {
  if (!layers || n < 1 || n > SR_CMP_MAX_LAYERS) SR_FAIL(SR_ERR_INVALID, "sr_cmp_run: null layers or n = %d not in 1..%d", n, (int)SR_CMP_MAX_LAYERS);
  for (int i = 0; i < n; ++i) {
    const int rc = check_layer(layers[i], i);
    if (rc != SR_OK) return rc;
  }
  for (int i = 0; i < n; ++i) {
    launch(layers[i], sr_stream(stream));
    SR_CHECK_LAUNCH("sr_cmp_run");
  }
  return SR_OK;
}

extern "C" int sr_cmp_pack_input(const float* src, int64_t sb, int64_t sy, int64_t sx, int64_t sc, int32_t B, int32_t H, int32_t W,
                                 int32_t C, void* dst, int32_t ld_dst, void* stream) {
  if (!src || !dst) SR_FAIL(SR_ERR_INVALID, "sr_cmp_pack_input: null pointer");
  if (B < 1 || H < 1 || W < 1 || C < 1) SR_FAIL(SR_ERR_INVALID, "sr_cmp_pack_input: sizes (%d, %d, %d, %d) must be positive", B, H, W, C);
  if (sb < 0 || sy < 0 || sx < 0 || sc < 0) SR_FAIL(SR_ERR_INVALID, "sr_cmp_pack_input: negative stride");
  if (ld_dst % 8 || C > ld_dst) SR_FAIL(SR_ERR_INVALID, "sr_cmp_pack_input: ld_dst = %d must be a multiple of 8 and hold %d channels", ld_dst, C);
  if (((uintptr_t)src & 3) != 0 || !aligned16(dst)) SR_FAIL(SR_ERR_INVALID, "sr_cmp_pack_input: src must be 4-byte and dst 16-byte aligned");
  pack_args p;
  p.src = src; p.dst = (_Float16*)dst; p.sb = sb; p.sy = sy; p.sx = sx; p.sc = sc;
  p.H = H; p.W = W; p.C = C; p.ld = ld_dst;
  p.total = (int64_t)B * H * W * ld_dst;
  if (p.total >= ((int64_t)1 << 31)) SR_FAIL(SR_ERR_INVALID, "sr_cmp_pack_input: B H W ld = %lld is not below 2^31", (long long)p.total);
  hipLaunchKernelGGL(pack_input_kernel, dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, sr_stream(stream), p);
  SR_CHECK_LAUNCH("sr_cmp_pack_input");
  return SR_OK;
}
