// The packed weight layout of the patch-stationary 3x3 convolutions of libsr_esrgan.so, libsr_taesd.so and libsr_compact.so (it is
// listed as `shared` for exactly those three in csrc/sidelib.py): a lane's MFMA A fragment is 16 contiguous bytes.  Host code only.
#ifndef SR_CONV3_PACK_H
#define SR_CONV3_PACK_H
#include <cstdint>

// where weight (n, c, ky, kx) of a Cout x Cin x 3 x 3 layer lies in the packed layout, in elements; -1 for a bad argument
static inline int64_t conv3_packed_index(int32_t Cout, int32_t Cin, int32_t n, int32_t c, int32_t ky, int32_t kx) {
  if (Cout < 32 || Cout % 32 || Cin < 32 || Cin % 32 || n < 0 || n >= Cout || c < 0 || c >= Cin || ky < 0 || ky > 2 || kx < 0 || kx > 2) return -1;
  const int64_t frag = ((int64_t)((c / 32) * 9 + ky * 3 + kx) * 2 + (c % 32) / 16) * (Cout / 32) + n / 32;
  return frag * 512 + (((c % 16) / 8) * 32 + n % 32) * 8 + c % 8;
}
#endif
