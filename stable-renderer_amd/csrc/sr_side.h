// The prologue every side library (csrc/sidelib.py's registry) shares: the thread-local error text and its accessor, the source
// hash the loader compares, the failure macros and the stream cast.  A translation unit includes it after its public header,
// having named its prefix in both cases and given the hash macro of its registry entry a default:
//   #define SR_SIDE tiled
//   #define SR_SIDE_UC TILED
// This is not sr_common.h: that one declares sr_set_error of errors.cpp and belongs to the hash of libsr_hip.so.
#ifndef SR_SIDE_H
#define SR_SIDE_H
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>

#if !defined(SR_SIDE) || !defined(SR_SIDE_UC)
#error "define SR_SIDE and SR_SIDE_UC before including sr_side.h"
#endif
#define SR_SIDE_CAT_(a, b, c) a##b##c
#define SR_SIDE_CAT(a, b, c) SR_SIDE_CAT_(a, b, c)
#define SR_SIDE_FN(suffix) SR_SIDE_CAT(sr_, SR_SIDE, suffix)       // sr_tiled_last_error
#define SR_SIDE_ID(suffix) SR_SIDE_CAT(SR_, SR_SIDE_UC, suffix)    // SR_TILED_OK

static thread_local char g_err[512] = "";
static void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
extern "C" const char* SR_SIDE_FN(_last_error)(void) { return g_err; }
extern "C" const char* SR_SIDE_FN(_source_hash)(void) { return SR_SIDE_ID(_SRC_HASH); }
#define SR_FAIL(code, ...) do { set_error(__VA_ARGS__); return (code); } while (0)
#define SR_CHECK_LAUNCH(name) do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) { \
    set_error("%s: %s", name, hipGetErrorString(e_)); return SR_SIDE_ID(_ERR_LAUNCH); } } while (0)
#define SR_ERR_INVALID SR_SIDE_ID(_ERR_INVALID)
#define SR_OK SR_SIDE_ID(_OK)

namespace {
inline hipStream_t sr_stream(void* s) { return (hipStream_t)s; }
}  // namespace
#endif
