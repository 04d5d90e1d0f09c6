// libsr_clip.so: the CLIP text encoder (sr_clip.h).  Five launches per transformer layer: LayerNorm + q|k|v, attention, out_proj
// into the stream, LayerNorm + fc1 + activation, fc2 into the stream; around them the embedding, the final LayerNorm, the pooled row
// and the prompt weighting.
//
// The linear kernel.  M = 77 R rows with R small, so the weights are the traffic: N x K halves that must come from HBM once.
//   A workgroup (4 waves) owns 32 output columns n and ALL rows: it loops M in chunks of 96 rows (three 32-row MFMA tiles) inside the
//   workgroup, so its 32 x K weight slice is fetched from HBM by the first chunk and from L2 by the later ones.  N / 32 workgroups.
//   MFMA 32x32x16 f16 with the WEIGHTS as the A operand (rows = n) and the activations as B (columns = m), as csrc/compact/compact.hip
//   does: a lane then holds runs of four consecutive n of one row m, which are 8-byte fp16 stores or 16-byte fp32 updates.
//   Weights are packed on the host so that a wave's fragment is 1 KB contiguous and a lane's part 16 bytes (sr_clip_packed_index).
//   The K range is split over the four waves (K / 4 each, a multiple of 16); the partial tiles meet in LDS and are summed in the
//   order wave 0, 1, 2, 3 by the wave that stores them: no atomics, no partial sums in memory, the same bits every run.
//   The B fragment of a lane is 8 consecutive k of one row, read from global memory (L2: the activations are a few hundred KB):
//   16 bytes of an fp16 source, or 32 bytes of the fp32 stream which are LayerNorm'ed (the row statistics of the chunk are computed
//   by the workgroup first, 16 lanes per row, two passes over registers) or just rounded.  Rows at and above M are zeros and are
//   never stored.  One wave per SIMD and at most N / 32 <= 160 workgroups: the loop is unrolled so that four steps' loads are in flight.
// The attention kernel: one workgroup (8 waves) per (section, head); K (pitch 66 halves: a lane per key reads its row conflict-free)
// and V in LDS, a wave per query row, a lane per key for the scores (only keys j <= t), fp32 softmax, a lane per channel for the sum.
#include <cstdint>
#include "sr_clip.h"
#define SR_SIDE clip
#define SR_SIDE_UC CLIP
#ifndef SR_CLIP_SRC_HASH
#define SR_CLIP_SRC_HASH "unstamped"
#endif
#include "../sr_side.h"

namespace {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int T = SR_CLIP_T, HD = SR_CLIP_HEAD_DIM, THREADS = 256;
constexpr int MT = 3, CH = MT * 32;                     // 32-row tiles and rows per M chunk
constexpr int UB = 4;                                   // k-steps whose loads are issued together
constexpr float EPS = 1e-5f;

__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ inline float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

__device__ inline float group_sum(float v) {             // over the 16 lanes that share lane >> 4
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// mean and 1 / sqrt(var + eps) of one fp32 row of n columns (a multiple of 64) by 16 lanes (l = lane & 15): the four 16-lane groups of a
// wave take four rows at once, and every lane of the wave must call it (`live` = false: a row past the end, nothing is read).  Two
// passes; for n <= 1280 the row is held in registers between them (all its loads in flight at once), wider rows are read twice.
// The same arithmetic in every caller.
__device__ inline void row_stats(const float* row, int n, int l, bool live, float& mean, float& rstd) {
  constexpr int NV = 20;
  float s = 0.f, q = 0.f;
  if (n <= NV * 64) {
    float4 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = (live && i * 64 < n) ? *(const float4*)(row + i * 64 + l * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    mean = group_sum(s) / (float)n;
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (i * 64 < n) {
        const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
        q += (a * a + b * b) + (c * c + d * d);
      }
  } else {
    if (live)
      for (int c = l * 4; c < n; c += 64) {
        const float4 v = *(const float4*)(row + c);
        s += (v.x + v.y) + (v.z + v.w);
      }
    mean = group_sum(s) / (float)n;
    if (live)
      for (int c = l * 4; c < n; c += 64) {
        const float4 v = *(const float4*)(row + c);
        const float a = v.x - mean, b = v.y - mean, cc = v.z - mean, d = v.w - mean;
        q += (a * a + b * b) + (cc * cc + d * d);
      }
  }
  rstd = 1.0f / sqrtf(group_sum(q) / (float)n + EPS);
}

__device__ inline float activate(float a, int act) {
  if (act == SR_CLIP_ACT_QUICK_GELU) return a / (1.0f + expf(-1.702f * a));
  if (act == SR_CLIP_ACT_GELU) return 0.5f * a * (1.0f + erff(a * 0.70710678118654752f));
  return a;
}

template <int SRC>
__global__ __launch_bounds__(THREADS) void linear_kernel(const sr_clip_op p) {
  __shared__ float red[4 * MT * 16 * 64];               // [wave][tile][register][lane], 48 KB
  __shared__ float stat[CH * 2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  const int M = p.M, K = p.K, n0 = (int)blockIdx.x * 32;
  const int kq = K / 4, k0 = wv * kq, steps = kq / 16;
  const _Float16* const wl = (const _Float16*)p.w + ((int64_t)blockIdx.x * (K / 16) + k0 / 16) * 512 + lane * 8;
  const int ld = p.ld_src;

  for (int m0 = 0; m0 < M; m0 += CH) {
    if (SRC == SR_CLIP_SRC_F32_LN) {
      for (int i0 = wv * 4; i0 < CH && m0 + i0 < M; i0 += 16) {          // uniform per wave: four rows at a time
        const int i = i0 + (lane >> 4);
        const bool live = m0 + i < M;
        float mean, rstd;
        row_stats((const float*)p.src + (int64_t)(m0 + i) * ld, K, lane & 15, live, mean, rstd);
        if (live && (lane & 15) == 0) { stat[2 * i] = mean; stat[2 * i + 1] = rstd; }
      }
      __syncthreads();
    }
    f32x16 acc[MT];
    bool ok[MT];
    float mu[MT], rs[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[i][k] = 0.f;
      ok[i] = m0 + i * 32 + r < M;
      mu[i] = rs[i] = 0.f;
      if (SRC == SR_CLIP_SRC_F32_LN && ok[i]) { mu[i] = stat[2 * (i * 32 + r)]; rs[i] = stat[2 * (i * 32 + r) + 1]; }
    }
    // this lane's B fragment of step s and tile i: 8 consecutive k of one row (zeros past M)
    auto fragment = [&](int s, int i, const float (&g)[8], const float (&b)[8]) {
      h16x8 xf;
#pragma unroll
      for (int j = 0; j < 8; ++j) xf[j] = (_Float16)0.f;
      if (ok[i]) {
        const int64_t off = (int64_t)(m0 + i * 32 + r) * ld + (k0 + s * 16 + 8 * h);
        if (SRC == SR_CLIP_SRC_F16) {
          xf = *(const h16x8*)((const _Float16*)p.src + off);
        } else {
          float x[8];
          *(float4*)x = *(const float4*)((const float*)p.src + off);
          *(float4*)(x + 4) = *(const float4*)((const float*)p.src + off + 4);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            xf[j] = SRC == SR_CLIP_SRC_F32_LN ? (_Float16)((x[j] - mu[i]) * rs[i] * g[j] + b[j]) : (_Float16)x[j];
        }
      }
      return xf;
    };
    // one wave per SIMD and at most 160 workgroups: latency, not issue, is the cost, so the loads of UB steps are in flight at once
    for (int s0 = 0; s0 < steps; s0 += UB) {
      h16x8 wf[UB], xf[UB][MT];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int s = s0 + u;
        if (s >= steps) continue;                         // uniform
        wf[u] = *(const h16x8*)(wl + (int64_t)s * 512);
        float g[8] = {}, b[8] = {};
        if (SRC == SR_CLIP_SRC_F32_LN) {
          const int k = k0 + s * 16 + 8 * h;
          *(float4*)g = *(const float4*)(p.gamma + k); *(float4*)(g + 4) = *(const float4*)(p.gamma + k + 4);
          *(float4*)b = *(const float4*)(p.beta + k); *(float4*)(b + 4) = *(const float4*)(p.beta + k + 4);
        }
#pragma unroll
        for (int i = 0; i < MT; ++i)
          if (m0 + i * 32 < M) xf[u][i] = fragment(s, i, g, b);        // else the whole tile lies past M (uniform)
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        if (s0 + u >= steps) continue;
#pragma unroll
        for (int i = 0; i < MT; ++i)
          if (m0 + i * 32 < M) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[u], xf[u][i], acc[i], 0, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int k = 0; k < 16; ++k) red[((wv * MT + i) * 16 + k) * 64 + lane] = acc[i][k];
    __syncthreads();
    // wave g sums and stores the registers 4g .. 4g + 3 of every tile: register 4g + k of a lane is column n0 + 8g + 4h + k of row r
    const int n = n0 + 8 * wv + 4 * h;
    float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias) bb = *(const float4*)(p.bias + n);
    const float bias[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int m = m0 + i * 32 + r;
      if (m >= M) continue;
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = (i * 16 + 4 * wv + k) * 64 + lane;
        v[k] = ((red[e] + red[e + MT * 16 * 64]) + red[e + 2 * MT * 16 * 64]) + red[e + 3 * MT * 16 * 64];
        v[k] = activate(v[k] + bias[k], p.act);
      }
      const int64_t o = (int64_t)m * p.ld_dst + n;
      if (p.dst_kind == SR_CLIP_DST_F16) {
        const h16x4 hv = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
        *(h16x4*)((_Float16*)p.dst + o) = hv;
      } else {
        float4* const q = (float4*)((float*)p.dst + o);
        float4 x = make_float4(v[0], v[1], v[2], v[3]);
        if (p.dst_kind == SR_CLIP_DST_F32_ADD) {
          const float4 c = *q;
          x = make_float4(c.x + v[0], c.y + v[1], c.z + v[2], c.w + v[3]);
        }
        *q = x;
      }
    }
    __syncthreads();                                    // red and stat are written again by the next chunk
  }
}

constexpr int KP = HD + 2;                              // K's LDS pitch in halves: 33 dwords
constexpr int AW = 8, ATHREADS = AW * 64;               // waves of an attention workgroup: a query row each

__global__ __launch_bounds__(ATHREADS) void attn_kernel(const sr_clip_op p) {
  __shared__ __attribute__((aligned(16))) _Float16 Ks[T * KP];
  __shared__ __attribute__((aligned(16))) _Float16 Vs[T * HD];
  __shared__ float qs[AW][HD];
  __shared__ float ps[AW][2 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int head = blockIdx.x, sec = blockIdx.y, D = p.N;
  const _Float16* const base = (const _Float16*)p.src + (int64_t)sec * T * p.ld_src + head * HD;
  for (int u = tid; u < T * 8; u += ATHREADS) {
    const int j = u >> 3, c = (u & 7) * 8;
    const _Float16* const row = base + (int64_t)j * p.ld_src + c;
    const uint4 kv = *(const uint4*)(row + D);
    uint32_t* const kd = (uint32_t*)(Ks + j * KP + c);
    kd[0] = kv.x; kd[1] = kv.y; kd[2] = kv.z; kd[3] = kv.w;
    *(uint4*)(Vs + j * HD + c) = *(const uint4*)(row + 2 * D);
  }
  __syncthreads();
  for (int t0 = 0; t0 < T; t0 += AW) {
    const int t = t0 + wv;                              // this wave's query row; the barriers below are reached by every wave
    const bool live = t < T;
    if (live) qs[wv][lane] = (float)base[(int64_t)t * p.ld_src + lane];
    __syncthreads();
    float s[2], mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int j = lane + 64 * e;
      s[e] = -INFINITY;
      if (live && j <= t) {
        float a = 0.f;
#pragma unroll
        for (int d = 0; d < HD; d += 2) {
          const h16x2 kk = *(const h16x2*)(Ks + j * KP + d);
          a += qs[wv][d] * (float)kk[0];
          a += qs[wv][d + 1] * (float)kk[1];
        }
        s[e] = a * 0.125f;
        mx = fmaxf(mx, s[e]);
      }
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int j = lane + 64 * e;
      const float pe = (live && j <= t) ? expf(s[e] - mx) : 0.f;
      ps[wv][j] = pe;
      sum += pe;
    }
    sum = wave_sum(sum);
    __syncthreads();
    if (live) {
      float a = 0.f;
      for (int j = 0; j <= t; ++j) a += ps[wv][j] * (float)Vs[j * HD + lane];
      ((_Float16*)p.dst)[((int64_t)sec * T + t) * p.ld_dst + head * HD + lane] = (_Float16)(a / sum);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(THREADS) void norm_kernel(const sr_clip_op p) {
  const int l = threadIdx.x & 15, m = (int)blockIdx.x * 16 + (threadIdx.x >> 4);      // 16 lanes per row
  const bool live = m < p.M;
  const float* const row = (const float*)p.src + (int64_t)m * p.ld_src;
  float* const out = (float*)p.dst + (int64_t)m * p.ld_dst;
  if (!p.gamma) {
    if (live)
      for (int c = l * 4; c < p.N; c += 64) *(float4*)(out + c) = *(const float4*)(row + c);
    return;
  }
  float mean, rstd;
  row_stats(row, p.N, l, live, mean, rstd);
  if (!live) return;
  for (int c = l * 4; c < p.N; c += 64) {
    const float4 v = *(const float4*)(row + c), g = *(const float4*)(p.gamma + c), b = *(const float4*)(p.beta + c);
    *(float4*)(out + c) = make_float4((v.x - mean) * rstd * g.x + b.x, (v.y - mean) * rstd * g.y + b.y,
                                      (v.z - mean) * rstd * g.z + b.z, (v.w - mean) * rstd * g.w + b.w);
  }
}

__global__ __launch_bounds__(THREADS) void gather_kernel(const sr_clip_op p) {
  const int r = blockIdx.x;
  const int t = min(max(p.idx[r], 0), T - 1);
  const float* const row = (const float*)p.src + ((int64_t)r * T + t) * p.ld_src;
  float* const out = (float*)p.dst + (int64_t)r * p.ld_dst;
  for (int c = threadIdx.x * 4; c < p.N; c += THREADS * 4) *(float4*)(out + c) = *(const float4*)(row + c);
}

__global__ __launch_bounds__(THREADS) void weigh_kernel(const sr_clip_op p) {
#pragma clang fp contract(off)
  const int m = blockIdx.x;
  const float w = p.aux[m];
  if (w == 1.0f) return;
  float* const z = (float*)p.dst + (int64_t)m * p.ld_dst;
  const float* const e = (const float*)p.w + (int64_t)(m % T) * p.ld_src;
  for (int c = threadIdx.x; c < p.N; c += THREADS) {
    const float ze = e[c];
    const float d = z[c] - ze;
    const float s = d * w;
    z[c] = s + ze;
  }
}

__global__ __launch_bounds__(THREADS) void embed_kernel(const int32_t* ids, const void* tok, int tok_is_f32, const float* extra, const float* pos,
                                                        float* x, int D, int vocab, int n_extra, int ld_x) {
  const int m = blockIdx.x;
  int id = ids[m];
  if (id < 0 || id >= vocab + n_extra) id = 0;
  float* const out = x + (int64_t)m * ld_x;
  const float* const pr = pos + (int64_t)(m % T) * D;
  for (int c = threadIdx.x * 4; c < D; c += THREADS * 4) {
    float4 v;
    if (id < vocab && tok_is_f32) {
      v = *(const float4*)((const float*)tok + (int64_t)id * D + c);
    } else if (id < vocab) {
      const h16x4 hv = *(const h16x4*)((const _Float16*)tok + (int64_t)id * D + c);
      v = make_float4((float)hv[0], (float)hv[1], (float)hv[2], (float)hv[3]);
    } else {
      v = *(const float4*)(extra + (int64_t)(id - vocab) * D + c);
    }
    const float4 q = *(const float4*)(pr + c);
    *(float4*)(out + c) = make_float4(v.x + q.x, v.y + q.y, v.z + q.z, v.w + q.w);
  }
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

int check_op(const sr_clip_op& o, int i) {
  const int64_t lim = (int64_t)1 << 31;
  if (o.op < SR_CLIP_OP_LINEAR || o.op > SR_CLIP_OP_WEIGH) SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: unknown op code %d", i, o.op);
  if (o.M < 1 || o.N < 64 || o.N % 64) SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: M = %d must be positive and N = %d a multiple of 64", i, o.M, o.N);
  if (!o.dst || !aligned16(o.dst)) SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: dst is null or not 16-byte aligned", i);
  if (o.op != SR_CLIP_OP_WEIGH && (!o.src || !aligned16(o.src))) SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: src is null or not 16-byte aligned", i);
  if (o.ld_dst < o.N || o.ld_dst % 8 || (int64_t)o.M * o.ld_dst >= lim)
    SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: ld_dst = %d (holds N = %d columns; a multiple of 8; M ld < 2^31)", i, o.ld_dst, o.N);
  const int width = o.op == SR_CLIP_OP_LINEAR ? o.K : o.op == SR_CLIP_OP_ATTN ? 3 * o.N : o.N;
  const int64_t rows = o.op == SR_CLIP_OP_GATHER ? (int64_t)o.M * T : o.op == SR_CLIP_OP_WEIGH ? T : o.M;
  if (o.op == SR_CLIP_OP_LINEAR && (o.K < 64 || o.K % 64)) SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: K = %d must be a multiple of 64", i, o.K);
  if (o.ld_src < width || o.ld_src % 8 || rows * o.ld_src >= lim)
    SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: ld_src = %d (holds %d columns; a multiple of 8; rows ld < 2^31)", i, o.ld_src, width);
  switch (o.op) {
    case SR_CLIP_OP_LINEAR:
      if (!o.w || !aligned16(o.w) || !aligned16(o.bias)) SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: w is null, or w or bias not 16-byte aligned", i);
      if (o.src_kind < SR_CLIP_SRC_F16 || o.src_kind > SR_CLIP_SRC_F32 || o.dst_kind < SR_CLIP_DST_F16 || o.dst_kind > SR_CLIP_DST_F32 ||
          o.act < SR_CLIP_ACT_NONE || o.act > SR_CLIP_ACT_GELU)
        SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: src_kind = %d, dst_kind = %d or act = %d is unknown", i, o.src_kind, o.dst_kind, o.act);
      if (o.src_kind == SR_CLIP_SRC_F32_LN && (!o.gamma || !o.beta || !aligned16(o.gamma) || !aligned16(o.beta)))
        SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: the LayerNorm source needs 16-byte aligned gamma and beta", i);
      if (o.src == o.dst) SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: dst must not be src (other workgroups read the rows one updates)", i);
      break;
    case SR_CLIP_OP_ATTN:
      if (o.heads < 1 || o.heads > 65535 || (int64_t)o.heads * HD != o.N)
        SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: N = %d over %d heads is not a head dimension of %d", i, o.N, o.heads, (int)HD);
      if (o.M % T || o.M / T > 65535) SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: M = %d is not a number of sections of T = %d tokens", i, o.M, (int)T);
      if (o.aux || o.idx) SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: a key-padding mask (enable_attention_masks) is not supported", i);
      if (o.src == o.dst) SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: dst must not be src", i);
      break;
    case SR_CLIP_OP_NORM:
      if (!o.gamma != !o.beta || !aligned16(o.gamma) || !aligned16(o.beta))
        SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: norm needs 16-byte aligned gamma and beta (or neither: a copy)", i);
      if (o.src == o.dst) SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: dst must not be src", i);
      break;
    case SR_CLIP_OP_GATHER:
      if (!o.idx || ((uintptr_t)o.idx & 3)) SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: gather needs a 4-byte aligned idx", i);
      if (o.src == o.dst) SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: dst must not be src", i);
      break;
    case SR_CLIP_OP_WEIGH:
      if (!o.aux || ((uintptr_t)o.aux & 3) || !o.w || !aligned16(o.w)) SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: weigh needs aux and a 16-byte aligned w (the empty section)", i);
      if (o.M % T) SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: M = %d is not a number of sections of T = %d tokens", i, o.M, (int)T);
      if (o.w == o.dst) SR_FAIL(SR_ERR_INVALID, "sr_clip_run: op %d: the empty section must not be the matrix that is weighted", i);
      break;
  }
  return SR_OK;
}

void launch(const sr_clip_op& o, hipStream_t st) {
  switch (o.op) {
    case SR_CLIP_OP_LINEAR: {
      const dim3 grid((unsigned)(o.N / 32));
      if (o.src_kind == SR_CLIP_SRC_F16) hipLaunchKernelGGL((linear_kernel<SR_CLIP_SRC_F16>), grid, dim3(THREADS), 0, st, o);
      else if (o.src_kind == SR_CLIP_SRC_F32_LN) hipLaunchKernelGGL((linear_kernel<SR_CLIP_SRC_F32_LN>), grid, dim3(THREADS), 0, st, o);
      else hipLaunchKernelGGL((linear_kernel<SR_CLIP_SRC_F32>), grid, dim3(THREADS), 0, st, o);
      break;
    }
    case SR_CLIP_OP_ATTN: hipLaunchKernelGGL(attn_kernel, dim3((unsigned)o.heads, (unsigned)(o.M / T)), dim3(ATHREADS), 0, st, o); break;
    case SR_CLIP_OP_NORM: hipLaunchKernelGGL(norm_kernel, dim3((unsigned)((o.M + 15) / 16)), dim3(THREADS), 0, st, o); break;
    case SR_CLIP_OP_GATHER: hipLaunchKernelGGL(gather_kernel, dim3((unsigned)o.M), dim3(THREADS), 0, st, o); break;
    case SR_CLIP_OP_WEIGH: hipLaunchKernelGGL(weigh_kernel, dim3((unsigned)o.M), dim3(THREADS), 0, st, o); break;
  }
}

}  // namespace

extern "C" int64_t sr_clip_packed_index(int32_t N, int32_t K, int32_t n, int32_t k) {
  if (N < 32 || N % 32 || K < 16 || K % 16 || n < 0 || n >= N || k < 0 || k >= K) return -1;
  return ((int64_t)(n / 32) * (K / 16) + k / 16) * 512 + (((k % 16) / 8) * 32 + n % 32) * 8 + k % 8;
}

extern "C" int sr_clip_embed(const int32_t* ids, const void* tok, const float* extra, const float* pos, float* x, int32_t M, int32_t D,
                             int32_t vocab, int32_t n_extra, int32_t ld_x, int32_t tok_is_f32, void* stream) {
  if (!ids || !tok || !pos || !x) SR_FAIL(SR_ERR_INVALID, "sr_clip_embed: null pointer");
  if (M < 1 || M % T) SR_FAIL(SR_ERR_INVALID, "sr_clip_embed: M = %d is not a number of sections of T = %d tokens", M, (int)T);
  if (D < 64 || D % 64) SR_FAIL(SR_ERR_INVALID, "sr_clip_embed: D = %d must be a multiple of 64", D);
  if (tok_is_f32 != 0 && tok_is_f32 != 1) SR_FAIL(SR_ERR_INVALID, "sr_clip_embed: tok_is_f32 = %d must be 0 or 1", tok_is_f32);
  if (vocab < 1 || n_extra < 0 || (n_extra > 0 && !extra)) SR_FAIL(SR_ERR_INVALID, "sr_clip_embed: vocab = %d, n_extra = %d (extra rows need the extra table)", vocab, n_extra);
  if (ld_x < D || ld_x % 4 || (int64_t)M * ld_x >= ((int64_t)1 << 31)) SR_FAIL(SR_ERR_INVALID, "sr_clip_embed: ld_x = %d (holds D = %d columns; a multiple of 4; M ld < 2^31)", ld_x, D);
  if (((uintptr_t)ids & 3) || !aligned16(tok) || !aligned16(extra) || !aligned16(pos) || !aligned16(x))
    SR_FAIL(SR_ERR_INVALID, "sr_clip_embed: ids must be 4-byte, the tables and x 16-byte aligned");
  hipLaunchKernelGGL(embed_kernel, dim3((unsigned)M), dim3(THREADS), 0, sr_stream(stream), ids, tok, tok_is_f32, extra, pos, x, D, vocab, n_extra, ld_x);
  SR_CHECK_LAUNCH("sr_clip_embed");
  return SR_OK;
}

extern "C" int sr_clip_run(const sr_clip_op* ops, int32_t n, void* stream) {
  if (!ops || n < 1 || n > SR_CLIP_MAX_OPS) SR_FAIL(SR_ERR_INVALID, "sr_clip_run: null ops or n = %d not in 1..%d", n, (int)SR_CLIP_MAX_OPS);
  for (int i = 0; i < n; ++i) {
    const int rc = check_op(ops[i], i);
    if (rc != SR_OK) return rc;
  }
  for (int i = 0; i < n; ++i) {
    launch(ops[i], sr_stream(stream));
    SR_CHECK_LAUNCH("sr_clip_run");
  }
  return SR_OK;
}
