// The row copy of the best-shot kernels (track_best_body, track_exit_copy_kernel, the two copies of flm_track_views.hip),
// stated once: `bytes` bytes from src to dst, cut into pieces of 16 bytes at the 16-byte lines of the SOURCE address.  A
// piece that lies wholly inside the row is one 16-byte access where the two addresses are congruent modulo 16; the
// pieces at the row's two ends, and every piece of a row whose addresses are not congruent, go byte by byte.  No byte
// outside [src, src + bytes) is read and none outside [dst, dst + bytes) written.  The threads that share a row pass
// their own `first` piece and the common `stride`.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace flm {

typedef unsigned copy4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void copy_row_bytes(const unsigned char* src, unsigned char* dst, size_t bytes, size_t first,
                                               size_t stride) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(src), a1 = a0 + bytes;
  const uintptr_t base = a0 & ~(uintptr_t)15;
  const bool congruent = ((a0 ^ reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
  const size_t pieces = (size_t)((a1 - base + 15) >> 4);
  for (size_t j = first; j < pieces; j += stride) {
    const uintptr_t lo = base + 16 * j, hi = lo + 16;
    if (congruent && lo >= a0 && hi <= a1) {
      const copy4v v = *reinterpret_cast<const copy4v*>(lo);
      *reinterpret_cast<copy4v*>(dst + (lo - a0)) = v;
    } else {
      const uintptr_t s = lo > a0 ? lo : a0, e = hi < a1 ? hi : a1;
      for (uintptr_t q = s; q < e; ++q) dst[q - a0] = *reinterpret_cast<const unsigned char*>(q);
    }
  }
}

}  // namespace flm
