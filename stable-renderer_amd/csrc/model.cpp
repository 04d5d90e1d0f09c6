// Operator-level entry points of the C ABI (include/sr_hip.h: sr_model_*, sr_unet_forward, sr_vae_decode).
//
// A *model bundle* is a launch plan made relocatable: the flat sr_op arrays a Python host lowered a UNet / VAE to (unet.py,
// vae.py, plan.py -- once per (weights, batch, resolution), tiles already chosen by the tuner), every device pointer in them
// replaced by (tensor id, byte offset), plus the tensor table (size, initial contents: packed weights, norm parameters, zero
// pages; activations are zero-filled) and the named input / output windows.  sr_model_load allocates the tensors on the current
// device, uploads their contents and patches the pointers back in; from then on a host written in any language runs
//     sr_unet_forward(m, x, t, ctx, out, stream)          = UNetModel.forward       (openaimodel.py:841-946)
//     sr_vae_decode(m, z, img, stream)                    = VAE.decode              (comfy/sd.py:329-346)
// through this library alone -- no Python, no torch in the process (tests/test_gpu_model_bundle.py does exactly that from a
// child process that imports neither).  The file is produced by stable-renderer_amd/bundle.py:export_bundle.
//
// File layout (little endian):  "SRMODEL1" | u32 version=1 | u32 n_tensors | u32 n_io | u32 n_plans
//   tensors[n_tensors] : u64 nbytes, u64 data_offset (0 = zero-filled, else absolute file offset of nbytes bytes)
//   io[n_io]           : char name[32], u32 tensor, u32 is_output, u64 offset, u64 nbytes
//   plans[n_plans]     : char name[16], u32 n_ops, u32 n_reloc, u32 sizeof_op, u32 pad,
//                        ops[n_ops * sizeof_op], reloc[n_reloc] = { u32 op, u32 field_offset, u32 tensor, u32 pad, u64 offset }
#include "sr_common.h"
#include "bundle_file.h"
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <new>
#include <string>
#include <vector>

namespace {
using sr_bundle::Io;
struct PlanRec { char name[16]; std::vector<sr_op> ops; };
}  // namespace

struct sr_model {
  std::vector<void*> tensors;
  std::vector<uint64_t> sizes;
  std::vector<Io> io;
  std::vector<PlanRec> plans;
  int device = -1;
  bool prologue_ran = false;                                 // sr_unet_forward(ctx = NULL) needs a projected prompt
};

static void free_model(sr_model* m) {
  if (!m) return;
  for (void* p : m->tensors) if (p) (void)hipFree(p);
  delete m;
}

// The file is not trusted, and nothing of it reaches the device before ALL of it has been judged: sr_bundle::read (bundle_file.h,
// host only) parses the head and checks every count, relocation, unrelocated pointer field, io window and -- through the sizes each
// op carries -- every byte an op would touch through a relocated pointer against the tensor it points into, and the sum of the
// tensor sizes against this device's memory.  Only then: allocate, zero or upload, patch the pointers in.  No address from the file
// ever reaches a kernel, and no count from it lets a kernel leave the tensor its pointer was relocated into.
extern "C" int sr_model_load(const char* path, sr_model** out) {
  if (!path || !out) SR_FAIL(SR_ERR_INVALID, "sr_model_load: null argument");
  *out = nullptr;
  size_t mem_free = 0, mem_total = 0;
  if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess || mem_total == 0) SR_FAIL(SR_ERR_LAUNCH, "sr_model_load: hipMemGetInfo failed");
  sr_model* m = nullptr;
  FILE* f = nullptr;
  try {
  sr_bundle::Bundle b;
  std::string err;
  if (sr_bundle::read(path, (uint64_t)mem_total, &b, &err) != SR_OK) SR_FAIL(SR_ERR_INVALID, "%s", err.c_str());
  const size_t nt = b.tensors.size();
  m = new sr_model();
  (void)hipGetDevice(&m->device);
  m->tensors.assign(nt, nullptr);
  m->sizes.resize(nt);
  for (size_t i = 0; i < nt; ++i) m->sizes[i] = b.tensors[i].nbytes;
  m->io = b.io;
  // ---- tensors: allocate, zero or upload
  f = fopen(path, "rb");
  if (!f) { free_model(m); SR_FAIL(SR_ERR_INVALID, "sr_model_load: cannot open %s", path); }
  std::vector<char> stage;
  for (size_t i = 0; i < nt; ++i) {
    const uint64_t nb = m->sizes[i] ? m->sizes[i] : 16;
    if (hipMalloc(&m->tensors[i], nb) != hipSuccess) { fclose(f); free_model(m); SR_FAIL(SR_ERR_LAUNCH, "sr_model_load: hipMalloc of %llu bytes failed", (unsigned long long)nb); }
    if (b.tensors[i].data_offset == 0) {
      if (hipMemset(m->tensors[i], 0, nb) != hipSuccess) { fclose(f); free_model(m); SR_FAIL(SR_ERR_LAUNCH, "sr_model_load: hipMemset failed"); }
    } else {
      stage.resize(m->sizes[i]);
      if (fseek(f, (long)b.tensors[i].data_offset, SEEK_SET) != 0 || fread(stage.data(), 1, m->sizes[i], f) != m->sizes[i] ||
          hipMemcpy(m->tensors[i], stage.data(), m->sizes[i], hipMemcpyHostToDevice) != hipSuccess) {
        fclose(f); free_model(m);
        SR_FAIL(SR_ERR_INVALID, "sr_model_load: cannot read / upload tensor %zu of %s", i, path);
      }
    }
  }
  fclose(f);
  f = nullptr;
  // ---- relocations (all validated above): (tensor, offset) -> device pointer, written into the pointer field of the op
  m->plans.resize(b.plans.size());
  for (size_t i = 0; i < b.plans.size(); ++i) {
    memcpy(m->plans[i].name, b.plans[i].name, sizeof(m->plans[i].name));
    m->plans[i].ops.swap(b.plans[i].ops);
    for (const sr_bundle::Reloc& r : b.plans[i].relocs) {
      void* ptr = (char*)m->tensors[r.tensor] + r.offset;
      memcpy((char*)&m->plans[i].ops[r.op] + r.field, &ptr, sizeof(void*));
    }
  }
  } catch (const std::bad_alloc&) {                          // (never through the extern "C" frame)
    if (f) fclose(f);
    free_model(m);
    SR_FAIL(SR_ERR_INVALID, "sr_model_load: %s: out of host memory for its tables", path);
  }
  *out = m;
  return SR_OK;
}

// the handle belongs to the device it was loaded on: its tensors live there
static int on_device(const sr_model* m, const char* who) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != m->device)
    SR_FAIL(SR_ERR_INVALID, "%s: the model was loaded on device %d, the current device is %d", who, m->device, dev);
  return SR_OK;
}

extern "C" int sr_model_free(sr_model* m) {
  free_model(m);
  return SR_OK;
}

static const Io* find_io(const sr_model* m, const char* name) {
  for (const Io& e : m->io)
    if (strncmp(e.name, name, sizeof(e.name)) == 0) return &e;
  return nullptr;
}

extern "C" int sr_model_io(sr_model* m, const char* name, void** dev_ptr, int64_t* nbytes) {
  if (!m || !name) SR_FAIL(SR_ERR_INVALID, "sr_model_io: null argument");
  const Io* e = find_io(m, name);
  if (!e) SR_FAIL(SR_ERR_INVALID, "sr_model_io: the bundle has no input / output named '%s'", name);
  if (dev_ptr) *dev_ptr = (char*)m->tensors[e->tensor] + e->offset;
  if (nbytes) *nbytes = (int64_t)e->nbytes;
  return SR_OK;
}

extern "C" int sr_model_run(sr_model* m, const char* plan, void* stream) {
  if (!m || !plan) SR_FAIL(SR_ERR_INVALID, "sr_model_run: null argument");
  if (on_device(m, "sr_model_run") != SR_OK) return SR_ERR_INVALID;
  for (const PlanRec& p : m->plans)
    if (strncmp(p.name, plan, sizeof(p.name)) == 0) {
      const int rc = sr_plan_run(p.ops.data(), (int32_t)p.ops.size(), stream);
      if (rc == SR_OK && strncmp(plan, "prologue", 9) == 0) m->prologue_ran = true;
      return rc;
    }
  SR_FAIL(SR_ERR_INVALID, "sr_model_run: the bundle has no plan named '%s'", plan);
}

// src / dst may be host or device memory (hipMemcpyDefault resolves it): a host without any HIP binding feeds host buffers
static int io_copy(sr_model* m, const char* name, const void* src, void* dst, bool write, void* stream, const char* who) {
  const Io* e = find_io(m, name);
  if (!e) SR_FAIL(SR_ERR_INVALID, "%s: the bundle has no input / output named '%s'", who, name);
  if (on_device(m, who) != SR_OK) return SR_ERR_INVALID;
  void* dev = (char*)m->tensors[e->tensor] + e->offset;
  const hipError_t rc = write ? hipMemcpyAsync(dev, src, e->nbytes, hipMemcpyDefault, sr_stream(stream))
                              : hipMemcpyAsync(dst, dev, e->nbytes, hipMemcpyDefault, sr_stream(stream));
  if (rc != hipSuccess) SR_FAIL(SR_ERR_LAUNCH, "%s: copy of '%s' failed: %s", who, name, hipGetErrorString(rc));
  return SR_OK;
}

extern "C" int sr_model_write(sr_model* m, const char* name, const void* src, void* stream) {
  if (!m || !name || !src) SR_FAIL(SR_ERR_INVALID, "sr_model_write: null argument");
  return io_copy(m, name, src, nullptr, true, stream, "sr_model_write");
}

extern "C" int sr_model_read(sr_model* m, const char* name, void* dst, void* stream) {
  if (!m || !name || !dst) SR_FAIL(SR_ERR_INVALID, "sr_model_read: null argument");
  const int rc = io_copy(m, name, nullptr, dst, false, stream, "sr_model_read");
  if (rc != SR_OK) return rc;
  if (hipStreamSynchronize(sr_stream(stream)) != hipSuccess) SR_FAIL(SR_ERR_LAUNCH, "sr_model_read: stream synchronisation failed");
  return SR_OK;
}

extern "C" int sr_unet_forward(sr_model* m, const float* x, const float* t, const void* ctx, float* out, void* stream) {
  if (!m || !x || !t || !out) SR_FAIL(SR_ERR_INVALID, "sr_unet_forward: null argument");
  int rc;
  if (ctx) {                                                 // a new prompt: cross-attention K / V are projected once (prologue plan)
    if ((rc = io_copy(m, "ctx", ctx, nullptr, true, stream, "sr_unet_forward")) != SR_OK) return rc;
    if ((rc = sr_model_run(m, "prologue", stream)) != SR_OK) return rc;
  } else if (!m->prologue_ran)
    SR_FAIL(SR_ERR_INVALID, "sr_unet_forward: ctx == NULL keeps the previous call's prompt, and there has been none (the cross-attention K / V are not projected yet)");
  if ((rc = io_copy(m, "x", x, nullptr, true, stream, "sr_unet_forward")) != SR_OK) return rc;
  if ((rc = io_copy(m, "t", t, nullptr, true, stream, "sr_unet_forward")) != SR_OK) return rc;
  if ((rc = sr_model_run(m, "step", stream)) != SR_OK) return rc;
  if ((rc = io_copy(m, "out", nullptr, out, false, stream, "sr_unet_forward")) != SR_OK) return rc;
  // a bundled plan with K/V injection carries the device flag sr_gather_rows raises on an out-of-range injected index (io window
  // "inject_err"): surfaced here, at the cost of one 4-byte read behind the evaluation
  if (find_io(m, "inject_err")) {
    int32_t flag = 0;
    if ((rc = sr_model_read(m, "inject_err", &flag, stream)) != SR_OK) return rc;
    if (flag != 0) {
      const int32_t zero = 0;
      (void)sr_model_write(m, "inject_err", &zero, stream);
      SR_FAIL(SR_ERR_INVALID, "sr_unet_forward: an injected frame index ('inject') lies outside the batch");
    }
  }
  return SR_OK;
}

extern "C" int sr_vae_decode(sr_model* m, const float* z, float* img, void* stream) {
  if (!m || !z || !img) SR_FAIL(SR_ERR_INVALID, "sr_vae_decode: null argument");
  int rc;
  if ((rc = io_copy(m, "z", z, nullptr, true, stream, "sr_vae_decode")) != SR_OK) return rc;
  if ((rc = sr_model_run(m, "step", stream)) != SR_OK) return rc;
  return io_copy(m, "img", nullptr, img, false, stream, "sr_vae_decode");
}
