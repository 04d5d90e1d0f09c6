// The k x k box maximum / minimum behind the Morphology node (kornia's dilation / erosion with an all-ones kernel, as sr_morph.h
// states them) and the 18 Porter-Duff modes of comfy_extras/nodes_compositing.py.  libsr_morph.so, private C ABI in sr_morph.h; why
// it is a library of its own and a private one: csrc/sidelib.py.
//
// The box is separable: a pass along x, then a pass along y, one launch each, the same kernel.  Of the two usual O(< k) schemes
// this is the power-of-two doubling in LDS, not van Herk / Gil-Werman: a workgroup stages a tile of R = S + k - 1 positions along
// the axis by T neighbouring lines (taps outside the image staged as -1e4 / +1e4), forms M_2p[i] = max(M_p[i], M_p[i + p]) for
// p = 1, 2, 4, ... while 2p <= k, ping-ponging between two LDS arrays with one barrier per level, and takes each of its S outputs
// from two overlapping windows, max(M_p[i], M_p[i + k - p]).  Per output that is about (R / S) log2 k maxima, never k taps.
// LDS: two arrays of NMAX floats (R T <= NMAX) per extreme that is computed: NMAX = 2048 for k <= 32, 4096 for k <= 64 and 8192
// beyond, that is 16, 32 or 64 KiB for one extreme and twice that for both (of the CU's 160 KiB), chosen so that T = 32 lines (one
// 128-byte line of memory) fit with R >= 2k where they can; T halves for larger k, down to 4 at k = 999.  The flat tile
// index is position * T + line, so lanes run along the lines in LDS (no bank conflicts: every access is to consecutive dwords)
// and in memory: in the pass along y the lines are the contiguous x C axis of the intermediate.
#include <cstdint>
#include "sr_morph.h"
#define SR_SIDE morph
#define SR_SIDE_UC MORPH
#ifndef SR_MORPH_SRC_HASH
#define SR_MORPH_SRC_HASH "unstamped"
#endif
#include "../sr_side.h"

// Bit equality with the reference needs every fp32 operation rounded on its own, and hipcc contracts a * b + c into a fused
// multiply-add by default.  The pragma forbids that for the operators written below it.  HIP's __fadd_rn / __fsub_rn / __fmul_rn do
// not help: they are plain operators defined in a header, above any pragma of ours, and are contracted (seen in this file's ISA).
#pragma clang fp contract(off)

namespace {

constexpr float PAD = 1e4f;                 // kornia's max_val: a tap outside the image is -PAD for the maximum, +PAD for the minimum
constexpr int THREADS = 256;
constexpr int MAX_SEGMENT = 1024;           // outputs along the axis per workgroup, at most

// torch.max / torch.min: a NaN on either side wins
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || a > b) ? a : b; }
__device__ __forceinline__ float nan_min(float a, float b) { return (a != a || a < b) ? a : b; }

// One pass along one axis.  The element (o, p, j) -- outer index o < n_outer, position p < L on the axis, line j < J -- lies at
//   o / O2 * s[0] + o % O2 * s[1] + p * s[2] + j / C * s[3] + j % C * s[4]
// of an input; the outputs are contiguous (n_outer, L, J).  Along x: o = (b, y), p = x, j = c.  Along y: o = b, p = y, j = (x, c).
struct Pass {
  const float* in_max;                      // what the maximum is taken of, and what the minimum is taken of: the same image in
  const float* in_min;                      // the first pass, the two halves of the intermediate in the second
  float* out_max;                           // null: that extreme is not stored (it may still be computed for the gradient)
  float* out_min;
  const float* epi_src;
  int64_t s[5], es[5];
  int n_outer, O2, L, J, C;
  int before;                               // taps before the output's position (k / 2, clipped to L)
  int kk;                                   // the window's length after clipping
  int S, T, R;                              // the tile: S outputs, T lines, R = S + kk - 1 positions
  int nseg, njt;
  int do_max, do_min, epilogue;
};

// BOTH: the maximum and the minimum are computed, each in its own pair of arrays; otherwise one of them, in the only pair
template <int NMAX, bool BOTH>
__global__ void __launch_bounds__(THREADS) box_pass_kernel(Pass a) {
  __shared__ float lds[(BOTH ? 4 : 2) * NMAX];
  float* cmx = lds;
  float* nmx = lds + NMAX;
  float* cmn = BOTH ? lds + 2 * NMAX : lds;
  float* nmn = BOTH ? lds + 3 * NMAX : lds + NMAX;
  const int tid = threadIdx.x;
  const unsigned bid = blockIdx.x;
  const int jt = (int)(bid % (unsigned)a.njt);
  const int seg = (int)((bid / (unsigned)a.njt) % (unsigned)a.nseg);
  const int o = (int)(bid / ((unsigned)a.njt * (unsigned)a.nseg));
  const int j0 = jt * a.T, s0 = seg * a.S;
  const int T = a.T, n = a.R * a.T;
  const int64_t base = (int64_t)(o / a.O2) * a.s[0] + (int64_t)(o % a.O2) * a.s[1];
  const bool same = a.in_max == a.in_min;

  for (int e = tid; e < n; e += THREADS) {
    const int r = e / T, t = e - r * T;
    const int pos = s0 - a.before + r, j = j0 + t;
    float vmax = -PAD, vmin = PAD;
    if (pos >= 0 && pos < a.L && j < a.J) {
      const int64_t off = base + (int64_t)pos * a.s[2] + (int64_t)(j / a.C) * a.s[3] + (int64_t)(j % a.C) * a.s[4];
      if (a.do_max) vmax = a.in_max[off];
      if (a.do_min) vmin = (same && a.do_max) ? vmax : a.in_min[off];
    }
    if (a.do_max) cmx[e] = vmax;
    if (a.do_min) cmn[e] = vmin;
  }
  __syncthreads();

  // M_p[e] covers the positions r ... r + p - 1 of its line wherever r + p <= R; entries beyond that are never read for a result
  int p = 1;
  while (2 * p <= a.kk) {
    const int sh = p * T;
    for (int e = tid; e < n; e += THREADS) {
      const int f = e + sh;
      if (a.do_max) nmx[e] = f < n ? nan_max(cmx[e], cmx[f]) : cmx[e];
      if (a.do_min) nmn[e] = f < n ? nan_min(cmn[e], cmn[f]) : cmn[e];
    }
    __syncthreads();                                         // one per level: the next level reads nmx and writes cmx
    float* q = cmx; cmx = nmx; nmx = q;
    q = cmn; cmn = nmn; nmn = q;
    p *= 2;
  }

  const int sh = (a.kk - p) * T;                             // e + sh <= (S + kk - p) T - 1 <= R T - 1
  const int nout = a.S * T;
  for (int e = tid; e < nout; e += THREADS) {
    const int r = e / T, t = e - r * T;
    const int pos = s0 + r, j = j0 + t;
    if (pos >= a.L || j >= a.J) continue;
    float vmax = 0.f, vmin = 0.f;
    if (a.do_max) vmax = nan_max(cmx[e], cmx[e + sh]);
    if (a.do_min) vmin = nan_min(cmn[e], cmn[e + sh]);
    const int64_t oi = ((int64_t)o * a.L + pos) * a.J + j;
    if (a.epilogue == SR_MORPH_EPI_GRADIENT) {
      a.out_max[oi] = vmax - vmin;
      continue;
    }
    if (a.epilogue != SR_MORPH_EPI_NONE) {
      const float x = a.epi_src[(int64_t)(o / a.O2) * a.es[0] + (int64_t)(o % a.O2) * a.es[1] + (int64_t)pos * a.es[2] +
                                (int64_t)(j / a.C) * a.es[3] + (int64_t)(j % a.C) * a.es[4]];
      const bool top = a.epilogue == SR_MORPH_EPI_TOP_HAT;
      vmax = top ? x - vmax : vmax - x;
      vmin = top ? x - vmin : vmin - x;
    }
    if (a.out_max) a.out_max[oi] = vmax;
    if (a.out_min) a.out_min[oi] = vmin;
  }
}

// the tile of a pass: -> NMAX (0: the window does not fit); fills kk, before, S, T, R, nseg, njt
int plan_tile(Pass& a, int k) {
  const int before = k / 2 < a.L ? k / 2 : a.L;              // a window that reaches past the image sees the same taps when it is
  const int after = k - k / 2 - 1 < a.L ? k - k / 2 - 1 : a.L;   // clipped to one tap outside: the padding is a constant
  a.before = before;
  a.kk = before + after + 1;
  int nmax = 2048;
  while (nmax < 8192 && nmax < 64 * (int64_t)a.kk) nmax *= 2;
  int T = a.J < 32 ? a.J : 32;
  while (T > 1 && nmax / T < 2 * a.kk) T /= 2;
  int S = nmax / T - a.kk + 1;
  if (S < 1) return 0;
  if (S > MAX_SEGMENT) S = MAX_SEGMENT;
  if (S > a.L) S = a.L;
  a.S = S;
  a.T = T;
  a.R = S + a.kk - 1;
  a.nseg = (a.L + S - 1) / S;
  a.njt = (a.J + T - 1) / T;
  return nmax;
}

// -> NMAX of the planned pass, 0 with the error set
int plan_pass(Pass& a, int k, const char* what) {
  const int nmax = plan_tile(a, k);
  if (nmax == 0 || (int64_t)a.n_outer * a.nseg * a.njt > 0x7fffffffLL) {
    set_error("sr_morph_box: %s does not fit a launch (k = %d)", what, k);
    return 0;
  }
  return nmax;
}

int launch_pass(const Pass& a, int nmax, const char* what, hipStream_t st) {
  const int64_t blocks = (int64_t)a.n_outer * a.nseg * a.njt;
  const dim3 grid((unsigned)blocks), block(THREADS);
  if (a.do_max && a.do_min) {
    if (nmax == 2048) hipLaunchKernelGGL((box_pass_kernel<2048, true>), grid, block, 0, st, a);
    else if (nmax == 4096) hipLaunchKernelGGL((box_pass_kernel<4096, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((box_pass_kernel<8192, true>), grid, block, 0, st, a);
  } else {
    if (nmax == 2048) hipLaunchKernelGGL((box_pass_kernel<2048, false>), grid, block, 0, st, a);
    else if (nmax == 4096) hipLaunchKernelGGL((box_pass_kernel<4096, false>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((box_pass_kernel<8192, false>), grid, block, 0, st, a);
  }
  SR_CHECK_LAUNCH(what);
  return SR_OK;
}

// ---- Porter-Duff ---------------------------------------------------------------------------------------------------------------------
// Each line below is the reference's expression, operation by operation, in its order of evaluation, and every operation is rounded
// on its own: nothing may be contracted into a fused multiply-add (the pragma at the top of this file).
#define ADD(x, y) ((x) + (y))
#define SUB(x, y) ((x) - (y))
#define MUL(x, y) ((x) * (y))

__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }   // torch.clamp: NaN stays

__device__ __forceinline__ float pd_alpha(int mode, float sa, float da) {
  switch (mode) {
    case SR_PD_ADD: return clamp01(ADD(sa, da));
    case SR_PD_CLEAR: return 0.f;
    case SR_PD_DARKEN: case SR_PD_LIGHTEN: case SR_PD_OVERLAY: case SR_PD_SCREEN: return SUB(ADD(sa, da), MUL(sa, da));
    case SR_PD_DST: case SR_PD_SRC_ATOP: return da;
    case SR_PD_DST_ATOP: case SR_PD_SRC: return sa;
    case SR_PD_DST_IN: case SR_PD_MULTIPLY: case SR_PD_SRC_IN: return MUL(sa, da);
    case SR_PD_DST_OUT: return MUL(SUB(1.f, sa), da);
    case SR_PD_DST_OVER: return ADD(da, MUL(SUB(1.f, da), sa));
    case SR_PD_SRC_OUT: return MUL(SUB(1.f, da), sa);
    case SR_PD_SRC_OVER: return ADD(sa, MUL(SUB(1.f, sa), da));
    default: return ADD(MUL(SUB(1.f, da), sa), MUL(SUB(1.f, sa), da));                              // XOR
  }
}

__device__ __forceinline__ float pd_image(int mode, float s, float sa, float d, float da) {
  switch (mode) {
    case SR_PD_ADD: return clamp01(ADD(s, d));
    case SR_PD_CLEAR: return 0.f;
    case SR_PD_DARKEN: return ADD(ADD(MUL(SUB(1.f, da), s), MUL(SUB(1.f, sa), d)), nan_min(s, d));
    case SR_PD_DST: return d;
    case SR_PD_DST_ATOP: return ADD(MUL(sa, d), MUL(SUB(1.f, da), s));
    case SR_PD_DST_IN: return MUL(d, sa);
    case SR_PD_DST_OUT: return MUL(SUB(1.f, sa), d);
    case SR_PD_DST_OVER: return ADD(d, MUL(SUB(1.f, da), s));
    case SR_PD_LIGHTEN: return ADD(ADD(MUL(SUB(1.f, da), s), MUL(SUB(1.f, sa), d)), nan_max(s, d));
    case SR_PD_MULTIPLY: return MUL(s, d);
    case SR_PD_OVERLAY:
      return MUL(2.f, d) < da ? MUL(MUL(2.f, s), d) : SUB(MUL(sa, da), MUL(MUL(2.f, SUB(da, s)), SUB(sa, d)));
    case SR_PD_SCREEN: return SUB(ADD(s, d), MUL(s, d));
    case SR_PD_SRC: return s;
    case SR_PD_SRC_ATOP: return ADD(MUL(da, s), MUL(SUB(1.f, sa), d));
    case SR_PD_SRC_IN: return MUL(s, da);
    case SR_PD_SRC_OUT: return MUL(SUB(1.f, da), s);
    case SR_PD_SRC_OVER: return ADD(s, MUL(SUB(1.f, sa), d));
    default: return ADD(MUL(SUB(1.f, da), s), MUL(SUB(1.f, sa), d));                                // XOR
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The image as n = n_pix C floats, then the alpha as n_pix floats, each in groups of four (n4, a4 groups; 0 when a pointer is not
// 16-byte aligned) with single elements behind them.  The element i of the image belongs to the pixel i / C.
__global__ void __launch_bounds__(THREADS) porter_duff_kernel(const float* __restrict__ src, const float* __restrict__ sa,
                                                              const float* __restrict__ dst, const float* __restrict__ da,
                                                              float* __restrict__ out, float* __restrict__ oa, int64_t n_pix, int C,
                                                              int mode, int64_t n4, int64_t a4) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = n_pix * C;
  for (int64_t g = tid; g < n4; g += stride) {
    const float4 s = *reinterpret_cast<const float4*>(src + 4 * g);
    const float4 d = *reinterpret_cast<const float4*>(dst + 4 * g);
    const int64_t p0 = (4 * g) / C;                          // one division per group: the next pixels follow from the remainder
    const int c0 = (int)(4 * g - p0 * C);
    const int64_t p1 = p0 + (c0 + 1) / C, p2 = p0 + (c0 + 2) / C, p3 = p0 + (c0 + 3) / C;
    float4 r;
    r.x = pd_image(mode, s.x, sa[p0], d.x, da[p0]);
    r.y = pd_image(mode, s.y, sa[p1], d.y, da[p1]);
    r.z = pd_image(mode, s.z, sa[p2], d.z, da[p2]);
    r.w = pd_image(mode, s.w, sa[p3], d.w, da[p3]);
    *reinterpret_cast<float4*>(out + 4 * g) = r;
  }
  for (int64_t i = 4 * n4 + tid; i < n; i += stride) {
    const int64_t p = i / C;
    out[i] = pd_image(mode, src[i], sa[p], dst[i], da[p]);
  }
  for (int64_t g = tid; g < a4; g += stride) {
    const float4 s = *reinterpret_cast<const float4*>(sa + 4 * g);
    const float4 d = *reinterpret_cast<const float4*>(da + 4 * g);
    *reinterpret_cast<float4*>(oa + 4 * g) =
        make_float4(pd_alpha(mode, s.x, d.x), pd_alpha(mode, s.y, d.y), pd_alpha(mode, s.z, d.z), pd_alpha(mode, s.w, d.w));
  }
  for (int64_t i = 4 * a4 + tid; i < n_pix; i += stride) oa[i] = pd_alpha(mode, sa[i], da[i]);
}

}  // namespace

extern "C" int sr_morph_box(const float* src, float* out_max, float* out_min, float* scratch, int64_t scratch_elems, int B, int H,
                            int W, int C, const int64_t* strides, int k, int epilogue, const float* epi_src,
                            const int64_t* epi_strides, void* stream) {
  if (!src || !scratch || !strides || (!out_max && !out_min)) SR_FAIL(SR_ERR_INVALID, "sr_morph_box: null src, scratch, strides or outputs");
  if (B < 1 || H < 1 || W < 1 || C < 1) SR_FAIL(SR_ERR_INVALID, "sr_morph_box: sizes (%d, %d, %d, %d) must be positive", B, H, W, C);
  if (k < 1 || k > SR_MORPH_MAX_K) SR_FAIL(SR_ERR_INVALID, "sr_morph_box: k = %d is not in 1..%d", k, (int)SR_MORPH_MAX_K);
  if (epilogue < SR_MORPH_EPI_NONE || epilogue > SR_MORPH_EPI_BOTTOM_HAT) SR_FAIL(SR_ERR_INVALID, "sr_morph_box: unknown epilogue %d", epilogue);
  if (epilogue == SR_MORPH_EPI_GRADIENT && (!out_max || out_min))
    SR_FAIL(SR_ERR_INVALID, "sr_morph_box: the gradient goes to out_max, and out_min is null");
  const bool hat = epilogue == SR_MORPH_EPI_TOP_HAT || epilogue == SR_MORPH_EPI_BOTTOM_HAT;
  if (hat != (epi_src != nullptr) || hat != (epi_strides != nullptr))
    SR_FAIL(SR_ERR_INVALID, "sr_morph_box: epi_src and epi_strides go with the top-hat and bottom-hat epilogues only");
  for (int i = 0; i < 4; ++i)
    if (strides[i] < 0 || (hat && epi_strides[i] < 0)) SR_FAIL(SR_ERR_INVALID, "sr_morph_box: negative stride");
  const int64_t wc = (int64_t)W * C, plane = (int64_t)B * H * wc;
  if (wc > 0x7fffffffLL || (int64_t)B * H > 0x7fffffffLL) SR_FAIL(SR_ERR_INVALID, "sr_morph_box: the image is too large");
  const bool do_max = out_max || epilogue == SR_MORPH_EPI_GRADIENT, do_min = out_min || epilogue == SR_MORPH_EPI_GRADIENT;
  const int64_t need = plane * ((do_max ? 1 : 0) + (do_min ? 1 : 0));
  if (scratch_elems < need)
    SR_FAIL(SR_ERR_INVALID, "sr_morph_box: scratch holds %lld floats, %lld are needed", (long long)scratch_elems, (long long)need);
  float* tmp_max = do_max ? scratch : nullptr;
  float* tmp_min = do_min ? scratch + (do_max ? plane : 0) : nullptr;
  hipStream_t st = sr_stream(stream);

  Pass x = {};                                               // along x: (b, y) outer, c the lines
  x.in_max = x.in_min = src;
  x.out_max = tmp_max;
  x.out_min = tmp_min;
  x.s[0] = strides[0]; x.s[1] = strides[1]; x.s[2] = strides[2]; x.s[3] = 0; x.s[4] = strides[3];
  x.n_outer = B * H; x.O2 = H; x.L = W; x.J = C; x.C = C;
  x.do_max = do_max; x.do_min = do_min; x.epilogue = SR_MORPH_EPI_NONE;

  Pass y = {};                                               // along y: b outer, (x, c) the lines, contiguous in the intermediate
  y.in_max = tmp_max;
  y.in_min = tmp_min;
  y.out_max = out_max;
  y.out_min = out_min;
  y.s[0] = (int64_t)H * wc; y.s[1] = 0; y.s[2] = wc; y.s[3] = C; y.s[4] = 1;
  if (hat) {
    y.epi_src = epi_src;
    y.es[0] = epi_strides[0]; y.es[1] = 0; y.es[2] = epi_strides[1]; y.es[3] = epi_strides[2]; y.es[4] = epi_strides[3];
  }
  y.n_outer = B; y.O2 = 1; y.L = H; y.J = (int)wc; y.C = C;
  y.do_max = do_max; y.do_min = do_min; y.epilogue = epilogue;
  // both passes are planned before the first is launched: nothing runs on arguments that are refused
  const int nx = plan_pass(x, k, "the pass along x"), ny = nx ? plan_pass(y, k, "the pass along y") : 0;
  if (!nx || !ny) return SR_ERR_INVALID;
  const int rc = launch_pass(x, nx, "sr_morph_box: the pass along x", st);
  return rc != SR_OK ? rc : launch_pass(y, ny, "sr_morph_box: the pass along y", st);
}

extern "C" int sr_porter_duff(const float* src, const float* src_alpha, const float* dst, const float* dst_alpha, float* out_image,
                              float* out_alpha, int64_t n_pix, int C, int mode, void* stream) {
  if (!src || !src_alpha || !dst || !dst_alpha || !out_image || !out_alpha) SR_FAIL(SR_ERR_INVALID, "sr_porter_duff: null pointer");
  if (n_pix < 1 || C < 1 || n_pix > (INT64_MAX >> 4) / C) SR_FAIL(SR_ERR_INVALID, "sr_porter_duff: n_pix = %lld, C = %d", (long long)n_pix, C);
  if (mode < 0 || mode >= SR_PD_MODES) SR_FAIL(SR_ERR_INVALID, "sr_porter_duff: unknown mode %d", mode);
  const int64_t n = n_pix * C;
  const int64_t n4 = al16(src) && al16(dst) && al16(out_image) ? n / 4 : 0;
  const int64_t a4 = al16(src_alpha) && al16(dst_alpha) && al16(out_alpha) ? n_pix / 4 : 0;
  // one item per thread up to 2048 workgroups (8 per CU of a 256-CU part), grid-stride beyond
  const int64_t items = n4 > 0 ? n4 : n;
  int64_t blocks = (items + THREADS - 1) / THREADS;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(porter_duff_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, sr_stream(stream), src, src_alpha, dst, dst_alpha,
                     out_image, out_alpha, n_pix, C, mode, n4, a4);
  SR_CHECK_LAUNCH("sr_porter_duff");
  return SR_OK;
}
