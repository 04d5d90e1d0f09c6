// Host-only reader and validator of model bundles ("SRMODEL1" files; layout: model.cpp).  Plain C++17: include/sr_hip.h and the
// standard library, no HIP header and no HIP call -- sr_model_load (model.cpp) runs it BEFORE it allocates anything, and
// tests/native/bundle_check_main.cpp runs it on a machine without a GPU, under the host sanitizers.
//
// The file is not trusted.  read() parses the head of the file (header, tensor table, io windows, plans, relocations; never the
// tensor contents) into host structures and refuses, with SR_ERR_INVALID and a message naming plan, op and field,
//   * counts that a file of this size cannot hold, a truncated head, a foreign sizeof(sr_op), tensor contents outside the file,
//   * a sum of tensor sizes that overflows or exceeds the limit the caller passes (the device's memory),
//   * an op kind outside the 15 known ones, a lane other than 0 / 1,
//   * a relocation that names no op / tensor / pointer field of the op's kind, names a field twice, or points at or past the end
//     of its tensor (offset 0 of a zero-size tensor is what the exporter writes for an empty storage and stays legal),
//   * a pointer field no relocation names that is not NULL in the file (no address from the file ever reaches a kernel),
//   * an io window outside its tensor, an "inject_err" window (the flag sr_unet_forward reads into one int32_t) of other than 4 bytes,
//   * and -- the EXTENTS -- every relocated pointer whose op would touch bytes past the end of the tensor it was relocated into:
//     the byte count of each pointer field is restated below from the contracts of include/sr_hip.h, and from the kernel where it
//     touches more than the contract said (packed weights: Npad = N rounded up to 128 rows; bias / colsum: whole 16-byte chunks, N
//     rounded up to 4 floats; the zero page: one K-row of the wider source, not 16 bytes; attention's output: rows of q_stride
//     elements).  Counts the entry point itself refuses
//     (negative sizes, an unknown dtype, KH / stride outside their sets, ldt below the row length ...) are refused here.
// What it cannot see: the CONTENTS of tensors and every field that is neither a pointer nor a size (scale, act, eps, tile ...):
// the format has no checksum, a corrupted weight or a flipped `act` loads and computes something else.
#ifndef SR_BUNDLE_FILE_H
#define SR_BUNDLE_FILE_H
#include "../../include/sr_hip.h"
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <new>
#include <string>
#include <vector>

namespace sr_bundle {

struct Tensor { uint64_t nbytes, data_offset; };             // data_offset 0 = zero-filled at load
struct Io { char name[32]; uint32_t tensor, is_output; uint64_t offset, nbytes; };
struct Reloc { uint32_t op, field, tensor, pad; uint64_t offset; };
struct Plan { char name[16]; std::vector<sr_op> ops; std::vector<Reloc> relocs; };
struct Extent { uint32_t plan, op; const char* field; uint32_t tensor; uint64_t offset, bytes; };   // one per relocated pointer
struct Field { size_t offset; const char* name; };
struct Bundle {
  std::vector<Tensor> tensors;
  std::vector<Io> io;
  std::vector<Plan> plans;
  std::vector<Extent> extents;
  uint64_t total_bytes = 0;                                  // sum of the tensor sizes
};
static_assert(sizeof(Io) == 56 && sizeof(Reloc) == 24 && sizeof(Tensor) == 16, "record layouts of the file format");

// byte offsets (inside sr_op) and names of every device-pointer field of an op of this kind; the order of the struct definitions
// (stable-renderer_amd/bundle.py:_pointer_fields derives the same table from the ctypes structs; tests/test_bundle_file.py pins them
// to each other)
inline std::vector<Field> pointer_fields(int kind) {
#define F(member, field) Field{offsetof(sr_op, u) + offsetof(decltype(sr_op::u), member) + offsetof(decltype(decltype(sr_op::u)::member), field), #field}
  switch (kind) {
    case SR_OP_IGEMM: return {F(igemm, a), F(igemm, a2), F(igemm, w), F(igemm, bias), F(igemm, rowvec), F(igemm, residual), F(igemm, out),
                              F(igemm, zero_page), F(igemm, workspace), F(igemm, row_stats), F(igemm, colsum), F(igemm, prefetch), F(igemm, split_counters)};
    case SR_OP_GROUPNORM: return {F(gn, x), F(gn, x2), F(gn, gamma), F(gn, beta), F(gn, y), F(gn, partials)};
    case SR_OP_ATTENTION: return {F(attn, q), F(attn, k), F(attn, vt), F(attn, o)};
    case SR_OP_LAYERNORM: case SR_OP_ROW_STATS: case SR_OP_LAYERNORM_GATHER:
      return {F(ln, x), F(ln, gamma), F(ln, beta), F(ln, y), F(ln, sel), F(ln, err_flag)};
    case SR_OP_NCHW_TO_NHWC: case SR_OP_NHWC_TO_NCHW: return {F(cvt, x), F(cvt, y), F(cvt, per_batch_scale)};
    case SR_OP_TIMESTEP_EMBED: return {F(temb, t), F(temb, y)};
    case SR_OP_SILU: case SR_OP_SOFTMAX_ROWS: return {F(ew, x), F(ew, y)};
    case SR_OP_GATHER_ROWS: return {F(gather, x), F(gather, y), F(gather, sel), F(gather, err_flag)};
    case SR_OP_ADD_SCALED: return {F(add, a), F(add, b), F(add, y)};
    default: return {};
  }
#undef F
}

// sr_groupnorm_scratch_floats (norm.hip) restated: the largest need of any batch up to B.  The chunk count of an entry depends on the
// batch only through three classes (b < 4, b < 8, b >= 8) and the need grows with b inside a class, so the largest b of each class
// decides.  (tests/test_gpu_model_bundle.py holds this against the library's function.)
inline int gn_pixels_per_chunk(int64_t HW, int64_t B) {
  const int64_t chunks = B >= 8 ? 64 : B >= 4 ? 128 : 256;
  const int64_t p = (HW + chunks - 1) / chunks;
  return (int)(p < 64 ? 64 : p);
}
inline uint64_t gn_scratch_floats(int64_t B, int64_t HW) {
  uint64_t need = 0;
  const int64_t top[3] = {B < 3 ? B : 3, B < 7 ? B : 7, B};
  for (int64_t b : top) {
    if (b < 1) continue;
    const int ppc = gn_pixels_per_chunk(HW, b);
    const uint64_t n = (uint64_t)b * (uint64_t)((HW + ppc - 1) / ppc) * 128u;
    need = n > need ? n : need;
  }
  return need;
}

namespace detail {
constexpr uint64_t SAT = ~(uint64_t)0;                       // a saturated product / sum: larger than any tensor
inline uint64_t mul(uint64_t a, uint64_t b) { return (a && b > SAT / a) ? SAT : a * b; }
inline uint64_t add(uint64_t a, uint64_t b) { return a > SAT - b ? SAT : a + b; }
// (rows - 1) * stride + width elements: the span of `rows` rows of `width` elements laid out `stride` apart; 0 when empty
inline uint64_t span(uint64_t rows, uint64_t stride, uint64_t width) { return (rows == 0 || width == 0) ? 0 : add(mul(rows - 1, stride), width); }

struct Need { const char* field; uint64_t bytes; };

// bytes every pointer field of this op is touched through -> needs; a non-empty `why` = the op's own counts are refused
inline void op_needs(const sr_op& op, std::vector<Need>& needs, std::string& why) {
  char buf[200];
#define BAD(...) do { snprintf(buf, sizeof(buf), __VA_ARGS__); why = buf; return; } while (0)
#define DTYPE(dt) do { if ((dt) != SR_F16 && (dt) != SR_F32) BAD("dtype %d", (int)(dt)); } while (0)
  switch (op.kind) {
    case SR_OP_IGEMM: {
      const sr_igemm_args& a = op.u.igemm;
      DTYPE(a.dtype);
      const uint64_t es = a.dtype == SR_F16 ? 2 : 4;
      if (a.B <= 0 || a.H <= 0 || a.W <= 0 || a.N <= 0) BAD("B=%d H=%d W=%d N=%d must be positive", a.B, a.H, a.W, a.N);
      if (a.C1 <= 0 || a.C2 < 0) BAD("C1=%d C2=%d", a.C1, a.C2);
      if (a.KH != 1 && a.KH != 3) BAD("KH=%d", a.KH);
      if (a.stride != 1 && a.stride != 2) BAD("stride=%d", a.stride);
      if (a.upsample && a.stride != 1) BAD("upsample with stride");
      if (a.pad_br && (a.KH != 3 || a.upsample)) BAD("pad_br is for 3x3 convs without upsample");
      if (a.up_h < 0 || a.up_w < 0 || (a.upsample && ((a.up_h > 0) != (a.up_w > 0))) || (!a.upsample && (a.up_h || a.up_w))) BAD("up_h=%d up_w=%d", a.up_h, a.up_w);
      if (a.act == 2 && (a.N % 4 || a.transpose_out)) BAD("GEGLU needs N %% 4 == 0 and a row-major output");
      if (a.rowvec_ld < 0 || a.workspace_bytes < 0 || a.prefetch_bytes < 0) BAD("rowvec_ld=%d workspace_bytes=%lld prefetch_bytes=%lld", a.rowvec_ld, (long long)a.workspace_bytes, (long long)a.prefetch_bytes);
      int64_t Ho, Wo;                                        // the rule of igemm_check (igemm.hip)
      if (a.upsample) { Ho = a.up_h > 0 ? a.up_h : 2 * (int64_t)a.H; Wo = a.up_w > 0 ? a.up_w : 2 * (int64_t)a.W; }
      else if (a.stride == 2) {
        const int ptot = a.pad_br ? a.KH / 2 : 2 * (a.KH / 2);
        Ho = ((int64_t)a.H + ptot - a.KH) / 2 + 1; Wo = ((int64_t)a.W + ptot - a.KH) / 2 + 1;
      } else { Ho = a.H; Wo = a.W; }
      if (Ho <= 0 || Wo <= 0) BAD("empty output %lld x %lld", (long long)Ho, (long long)Wo);
      const uint64_t rpb = mul((uint64_t)Ho, (uint64_t)Wo), M = mul((uint64_t)a.B, rpb);
      if (M > 0x7fffffffULL / 2) BAD("M too large");
      if (a.transpose_out && (a.ldt < 0 || (uint64_t)a.ldt < rpb)) BAD("ldt=%d < pixels per batch", a.ldt);
      const uint64_t pix = mul(mul((uint64_t)a.B, (uint64_t)a.H), (uint64_t)a.W);
      const uint64_t K = mul((uint64_t)(a.KH * a.KH), (uint64_t)a.C1 + (uint64_t)a.C2);
      const uint64_t Npad = ((uint64_t)a.N + 127) / 128 * 128;   // the kernels stage whole tiles of weight rows: rows N..Npad-1 are read
      const uint64_t ldo = a.act == 2 ? (uint64_t)a.N / 2 : (uint64_t)a.N, oes = a.out_f32 ? 4 : es;
      needs.push_back({"a", mul(mul(pix, (uint64_t)a.C1), es)});
      needs.push_back({"a2", mul(mul(pix, (uint64_t)a.C2), es)});
      needs.push_back({"w", mul(mul(Npad, K), es)});
      // bias / colsum: the fp16 unsplit tile kernels fetch the tile's rows in 16-byte chunks, one at every n = n0 + 4c < N (igemm.hip,
      // igemm_kernel: "[bias n0..n0+BN) | colsum n0..n0+BN)] -> LDS"), the other epilogues read a float4 at n < N (epilogue_rows_h,
      // splitk_reduce_kernel): the last chunk ends at N rounded up to 4 floats (ops.pack_bias pads to that)
      const uint64_t vec4 = ((uint64_t)a.N + 3) / 4 * 16;
      needs.push_back({"bias", vec4});
      needs.push_back({"rowvec", mul(span((uint64_t)a.B, a.rowvec_ld ? (uint64_t)a.rowvec_ld : (uint64_t)a.N, (uint64_t)a.N), 4)});
      needs.push_back({"residual", a.transpose_out ? 0 : mul(mul(M, ldo), es)});
      needs.push_back({"out", a.transpose_out ? mul(mul(mul((uint64_t)a.B, (uint64_t)a.N), (uint64_t)a.ldt), oes) : mul(mul(M, ldo), oes)});
      // padding taps and rows >= M read the zero page at the K offset of the source row they stand in for: one row of the wider source
      const uint64_t zrow = mul((uint64_t)(a.C1 > a.C2 ? a.C1 : a.C2), es);
      needs.push_back({"zero_page", zrow < 16 ? 16 : zrow});
      needs.push_back({"workspace", (uint64_t)a.workspace_bytes});
      needs.push_back({"row_stats", mul(M, 8)});
      needs.push_back({"colsum", vec4});
      needs.push_back({"prefetch", (uint64_t)a.prefetch_bytes});
      needs.push_back({"split_counters", (uint64_t)SR_IGEMM_SPLIT_COUNTERS * 4});
      return;
    }
    case SR_OP_GROUPNORM: {
      const sr_groupnorm_args& a = op.u.gn;
      DTYPE(a.dtype);
      const uint64_t es = a.dtype == SR_F16 ? 2 : 4;
      if (a.B < 0 || a.HW < 0 || a.C1 < 0 || a.C2 < 0) BAD("B=%d HW=%d C1=%d C2=%d", a.B, a.HW, a.C1, a.C2);
      const uint64_t pix = mul((uint64_t)a.B, (uint64_t)a.HW), C = (uint64_t)a.C1 + (uint64_t)a.C2;
      if (a.groups <= 0 || a.groups > 32 || C % (uint64_t)a.groups) BAD("C=%llu groups=%d", (unsigned long long)C, a.groups);
      needs.push_back({"x", mul(mul(pix, (uint64_t)a.C1), es)});
      needs.push_back({"x2", mul(mul(pix, (uint64_t)a.C2), es)});
      needs.push_back({"gamma", C * 4});
      needs.push_back({"beta", C * 4});
      needs.push_back({"y", mul(mul(pix, C), es)});
      needs.push_back({"partials", mul(gn_scratch_floats(a.B, a.HW), 4)});
      return;
    }
    case SR_OP_ATTENTION: {
      const sr_attention_args& a = op.u.attn;
      DTYPE(a.dtype);
      const uint64_t es = a.dtype == SR_F16 ? 2 : 4;
      if (a.B < 0 || a.Tq < 0 || a.Tk < 0 || a.heads < 0 || a.d < 0 || a.q_stride < 0 || a.k_stride < 0) BAD("negative count");
      if (a.Bk != 1 && a.Bk != a.B) BAD("Bk=%d must be 1 or B=%d", a.Bk, a.B);
      if (a.ldt < a.Tk) BAD("ldt=%d < Tk=%d", a.ldt, a.Tk);
      const uint64_t row = mul((uint64_t)a.heads, (uint64_t)a.d);
      const uint64_t qspan = mul(span(mul((uint64_t)a.B, (uint64_t)a.Tq), (uint64_t)a.q_stride, row), es);
      needs.push_back({"q", qspan});
      needs.push_back({"k", mul(span(mul((uint64_t)a.Bk, (uint64_t)a.Tk), (uint64_t)a.k_stride, row), es)});
      needs.push_back({"vt", mul(mul(mul((uint64_t)a.Bk, row), (uint64_t)a.ldt), es)});
      needs.push_back({"o", qspan});                         // the kernels write o in rows of q_stride elements
      return;
    }
    case SR_OP_LAYERNORM: case SR_OP_ROW_STATS: case SR_OP_LAYERNORM_GATHER: {
      const auto& a = op.u.ln;
      DTYPE(a.dtype);
      const uint64_t es = a.dtype == SR_F16 ? 2 : 4;
      if (a.rows < 0 || a.C < 0) BAD("rows=%d C=%d", a.rows, a.C);
      const uint64_t body = mul(mul((uint64_t)a.rows, (uint64_t)a.C), es);
      if (op.kind == SR_OP_LAYERNORM_GATHER) {
        if (a.frame_rows < 1 || a.n_frames < 1 || a.rows % a.frame_rows || a.rows / a.frame_rows < 1) BAD("rows=%d frame_rows=%d n_frames=%d", a.rows, a.frame_rows, a.n_frames);
        needs.push_back({"x", mul(mul(mul((uint64_t)a.n_frames, (uint64_t)a.frame_rows), (uint64_t)a.C), es)});
        needs.push_back({"sel", (uint64_t)(a.rows / a.frame_rows) * 4});
        needs.push_back({"err_flag", 4});
      } else {
        needs.push_back({"x", body});
        needs.push_back({"sel", 0});
        needs.push_back({"err_flag", 0});
      }
      const bool stats = op.kind == SR_OP_ROW_STATS;         // y = [rows, 2] fp32, no gamma / beta
      needs.push_back({"gamma", stats ? 0 : (uint64_t)a.C * 4});
      needs.push_back({"beta", stats ? 0 : (uint64_t)a.C * 4});
      needs.push_back({"y", stats ? mul((uint64_t)a.rows, 8) : body});
      return;
    }
    case SR_OP_NCHW_TO_NHWC: case SR_OP_NHWC_TO_NCHW: {
      const auto& a = op.u.cvt;
      DTYPE(a.dtype);
      const uint64_t es = a.dtype == SR_F16 ? 2 : 4;
      if (a.B < 0 || a.C < 0 || a.HW < 0) BAD("B=%d C=%d HW=%d", a.B, a.C, a.HW);
      const uint64_t pix = mul((uint64_t)a.B, (uint64_t)a.HW), planar = mul(mul(pix, (uint64_t)a.C), 4);
      if (op.kind == SR_OP_NCHW_TO_NHWC) {
        if (a.Cpad < a.C) BAD("Cpad=%d < C=%d", a.Cpad, a.C);
        needs.push_back({"x", planar});
        needs.push_back({"y", mul(mul(pix, (uint64_t)a.Cpad), es)});
        needs.push_back({"per_batch_scale", (uint64_t)a.B * 4});
      } else {
        if (a.ldc < a.C) BAD("ldc=%d < C=%d", a.ldc, a.C);
        needs.push_back({"x", mul(span(pix, (uint64_t)a.ldc, (uint64_t)a.C), es)});
        needs.push_back({"y", planar});
        needs.push_back({"per_batch_scale", 0});
      }
      return;
    }
    case SR_OP_TIMESTEP_EMBED: {
      const auto& a = op.u.temb;
      DTYPE(a.dtype);
      if (a.B < 0 || a.dim < 0 || a.dim % 2 || (int64_t)a.B * a.dim > 0x7fffffff) BAD("B=%d dim=%d", a.B, a.dim);
      needs.push_back({"t", (uint64_t)a.B * 4});
      needs.push_back({"y", mul(mul((uint64_t)a.B, (uint64_t)a.dim), a.dtype == SR_F16 ? 2 : 4)});
      return;
    }
    case SR_OP_SILU: case SR_OP_SOFTMAX_ROWS: {
      const auto& a = op.u.ew;
      DTYPE(a.dtype);
      const uint64_t es = a.dtype == SR_F16 ? 2 : 4;
      if (op.kind == SR_OP_SILU) {
        if (a.n < 0) BAD("n=%lld", (long long)a.n);
        needs.push_back({"x", mul((uint64_t)a.n, es)});
        needs.push_back({"y", mul((uint64_t)a.n, es)});
      } else {                                               // in place on y; x is not read
        if (a.rows < 0 || a.cols < 0) BAD("rows=%d cols=%d", a.rows, a.cols);
        needs.push_back({"x", 0});
        needs.push_back({"y", mul(mul((uint64_t)a.rows, (uint64_t)a.cols), es)});
      }
      return;
    }
    case SR_OP_GATHER_ROWS: {
      const auto& a = op.u.gather;
      if (a.row_bytes <= 0 || a.row_bytes % 16 || a.nsel < 0 || a.n_rows < 1) BAD("row_bytes=%lld nsel=%d n_rows=%d", (long long)a.row_bytes, a.nsel, a.n_rows);
      needs.push_back({"x", mul((uint64_t)a.n_rows, (uint64_t)a.row_bytes)});
      needs.push_back({"y", mul((uint64_t)a.nsel, (uint64_t)a.row_bytes)});
      needs.push_back({"sel", (uint64_t)a.nsel * 4});
      needs.push_back({"err_flag", 4});
      return;
    }
    case SR_OP_ADD_SCALED: {
      const auto& a = op.u.add;
      DTYPE(a.dtype);
      if (a.n < 0) BAD("n=%lld", (long long)a.n);
      const uint64_t nb = mul((uint64_t)a.n, a.dtype == SR_F16 ? 2 : 4);
      needs.push_back({"a", nb});
      needs.push_back({"b", nb});
      needs.push_back({"y", nb});
      return;
    }
    default: return;                                         // FORK / JOIN: no pointers
  }
#undef DTYPE
#undef BAD
}

inline bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
struct Closer { FILE* f; ~Closer() { if (f) fclose(f); } };
}  // namespace detail

// Parse and validate the bundle at `path`.  max_total_bytes: upper limit of the sum of the tensor sizes (0 = none).  Returns SR_OK
// with *out filled (out->extents: what was checked, one record per relocated pointer) or SR_ERR_INVALID with *err set.
inline int read(const char* path, uint64_t max_total_bytes, Bundle* out, std::string* err) {
  using namespace detail;
  char msg[512];
#define REFUSE(...) do { snprintf(msg, sizeof(msg), __VA_ARGS__); *err = msg; return SR_ERR_INVALID; } while (0)
  if (!path || !out || !err) { if (err) *err = "sr_model_load: null argument"; return SR_ERR_INVALID; }
  *out = Bundle();
  Closer file{fopen(path, "rb")};
  FILE* f = file.f;
  if (!f) REFUSE("sr_model_load: cannot open %s", path);
  try {
    char magic[8];
    uint32_t hdr[4];
    if (!rd(f, magic, 8) || memcmp(magic, "SRMODEL1", 8) != 0 || !rd(f, hdr, sizeof(hdr)) || hdr[0] != 1)
      REFUSE("sr_model_load: %s is not a version-1 model bundle", path);
    const uint32_t nt = hdr[1], nio = hdr[2], np = hdr[3];
    // every count is bounded by what a file of this size can hold before anything is allocated for it
    long fsize_l = 0;
    if (fseek(f, 0, SEEK_END) != 0 || (fsize_l = ftell(f)) < 24 || fseek(f, 24, SEEK_SET) != 0 ||
        (uint64_t)nt * sizeof(Tensor) + (uint64_t)nio * sizeof(Io) + (uint64_t)np * 32 > (uint64_t)fsize_l)
      REFUSE("sr_model_load: %s: header counts (%u tensors, %u io, %u plans) do not fit the file", path, nt, nio, np);
    const uint64_t fsize = (uint64_t)fsize_l;
    out->tensors.resize(nt);
    out->io.resize(nio);
    out->plans.resize(np);
    if (!rd(f, out->tensors.data(), (size_t)nt * sizeof(Tensor)) || !rd(f, out->io.data(), (size_t)nio * sizeof(Io)))
      REFUSE("sr_model_load: %s is truncated", path);
    for (uint32_t i = 0; i < np; ++i) {
      Plan& p = out->plans[i];
      uint32_t ph[4];
      if (!rd(f, p.name, 16) || !rd(f, ph, sizeof(ph))) REFUSE("sr_model_load: %s is truncated", path);
      if (ph[2] != sizeof(sr_op))
        REFUSE("sr_model_load: bundle built for sizeof(sr_op) = %u, this library has %zu (re-export it)", ph[2], sizeof(sr_op));
      if ((uint64_t)ph[0] * sizeof(sr_op) + (uint64_t)ph[1] * sizeof(Reloc) > fsize || ph[0] > 0x7fffffffu)
        REFUSE("sr_model_load: %s is truncated (plan %u: %u ops, %u relocations)", path, i, ph[0], ph[1]);
      p.ops.resize(ph[0]);
      p.relocs.resize(ph[1]);
      if (!rd(f, p.ops.data(), (size_t)ph[0] * sizeof(sr_op)) || !rd(f, p.relocs.data(), (size_t)ph[1] * sizeof(Reloc)))
        REFUSE("sr_model_load: %s is truncated", path);
    }
    // ---- tensors: contents inside the file, sizes that add up to something a device can hold
    uint64_t total = 0;
    for (uint32_t i = 0; i < nt; ++i) {
      const Tensor& t = out->tensors[i];
      if (t.data_offset != 0 && (t.data_offset > fsize || t.nbytes > fsize - t.data_offset))
        REFUSE("sr_model_load: tensor %u of %s lies outside the file", i, path);
      const uint64_t nb = t.nbytes ? t.nbytes : 16;            // (what the loader allocates for an empty tensor)
      if (total > SAT - nb) REFUSE("sr_model_load: %s: the tensor sizes overflow (tensor %u: %llu bytes)", path, i, (unsigned long long)t.nbytes);
      total += nb;
    }
    if (max_total_bytes && total > max_total_bytes)
      REFUSE("sr_model_load: %s: the tensor sizes add up to %llu bytes, above the limit of %llu bytes", path, (unsigned long long)total, (unsigned long long)max_total_bytes);
    out->total_bytes = total;
    // ---- plans: kinds and lanes; relocations name a pointer field of their op once and stay inside their tensor; every other
    // pointer field is NULL; every relocated pointer's extent stays inside its tensor
    std::vector<Need> needs;
    for (uint32_t i = 0; i < np; ++i) {
      Plan& p = out->plans[i];
      const size_t n_ops = p.ops.size();
      for (size_t o = 0; o < n_ops; ++o) {
        if (p.ops[o].kind < SR_OP_IGEMM || p.ops[o].kind > SR_OP_LAYERNORM_GATHER) REFUSE("sr_model_load: plan %u op %zu: unknown op kind %d", i, o, p.ops[o].kind);
        if (p.ops[o].lane != 0 && p.ops[o].lane != 1) REFUSE("sr_model_load: plan %u op %zu: lane %d is neither 0 nor 1", i, o, p.ops[o].lane);
      }
      std::vector<std::vector<const Reloc*>> hit(n_ops);       // per op: the relocation of each pointer field, in table order
      for (const Reloc& r : p.relocs) {
        if (r.op >= n_ops || r.tensor >= nt || (uint64_t)r.field + sizeof(void*) > sizeof(sr_op))
          REFUSE("sr_model_load: bad relocation in plan %u (op %u, field offset %u, tensor %u)", i, r.op, r.field, r.tensor);
        const uint64_t size = out->tensors[r.tensor].nbytes;
        if (r.offset >= size && !(r.offset == 0 && size == 0))
          REFUSE("sr_model_load: bad relocation in plan %u op %u: offset %llu is not inside tensor %u (%llu bytes)", i, r.op,
                 (unsigned long long)r.offset, r.tensor, (unsigned long long)size);
        const std::vector<Field> pf = pointer_fields(p.ops[r.op].kind);
        size_t which = pf.size();
        for (size_t k = 0; k < pf.size(); ++k) if (pf[k].offset == r.field) which = k;
        if (which == pf.size()) REFUSE("sr_model_load: plan %u op %u: relocation of a non-pointer field (offset %u)", i, r.op, r.field);
        if (hit[r.op].empty()) hit[r.op].assign(pf.size(), nullptr);
        if (hit[r.op][which]) REFUSE("sr_model_load: bad relocation in plan %u op %u: field %s is named twice", i, r.op, pf[which].name);
        hit[r.op][which] = &r;
      }
      for (size_t o = 0; o < n_ops; ++o) {
        const sr_op& op = p.ops[o];
        const std::vector<Field> pf = pointer_fields(op.kind);
        for (size_t k = 0; k < pf.size(); ++k) {
          if (!hit[o].empty() && hit[o][k]) continue;
          uint64_t v = 0;
          memcpy(&v, (const char*)&op + pf[k].offset, sizeof(v));
          if (v) REFUSE("sr_model_load: plan %u op %zu carries a raw address in an unrelocated pointer field (%s)", i, o, pf[k].name);
        }
        needs.clear();
        std::string why;
        op_needs(op, needs, why);                                // (an op no relocation names has its counts checked all the same)
        if (!why.empty()) REFUSE("sr_model_load: plan %u op %zu (kind %d): %s", i, o, op.kind, why.c_str());
        for (size_t k = 0; k < pf.size(); ++k) {
          const Reloc* r = hit[o].empty() ? nullptr : hit[o][k];
          if (!r) continue;
          uint64_t bytes = SAT;
          for (const Need& n : needs) if (strcmp(n.field, pf[k].name) == 0) bytes = n.bytes;
          const uint64_t size = out->tensors[r->tensor].nbytes;
          if (bytes > size - r->offset)
            REFUSE("sr_model_load: plan %u op %zu (kind %d) field %s: the op touches %llu bytes from offset %llu of tensor %u, which has %llu",
                   i, o, op.kind, pf[k].name, (unsigned long long)bytes, (unsigned long long)r->offset, r->tensor, (unsigned long long)size);
          out->extents.push_back(Extent{i, (uint32_t)o, pf[k].name, r->tensor, r->offset, bytes});
        }
      }
    }
    for (size_t k = 0; k < out->io.size(); ++k) {
      const Io& e = out->io[k];
      if (e.tensor >= nt || e.offset > out->tensors[e.tensor].nbytes || e.nbytes > out->tensors[e.tensor].nbytes - e.offset)
        REFUSE("sr_model_load: bad io window %zu (tensor %u, offset %llu, %llu bytes)", k, e.tensor, (unsigned long long)e.offset, (unsigned long long)e.nbytes);
      // sr_unet_forward reads and clears this window through one int32_t on the host
      if (strncmp(e.name, "inject_err", sizeof(e.name)) == 0 && e.nbytes != 4)
        REFUSE("sr_model_load: bad io window %zu ('inject_err' is one 4-byte flag, the file gives it %llu bytes)", k, (unsigned long long)e.nbytes);
    }
  } catch (const std::bad_alloc&) {
    REFUSE("sr_model_load: %s: out of host memory for its tables", path);
  }
#undef REFUSE
  return SR_OK;
}

}  // namespace sr_bundle
#endif
