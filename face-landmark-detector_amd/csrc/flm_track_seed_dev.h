// The arithmetic of flm_track_seed for one box, stated once: track_seed_kernel (flm_track.hip) writes it for every box it
// is given, track_assoc_kernel (flm_track_assoc.hip) for the slots it restarts or fills from a detection.
// include/flm.h states the contract; float64, one IEEE operation per written operator (-ffp-contract=off).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flm.h"

namespace flm {

struct TrackSeed {
  float a, d, tx, ty;  // M = [[a, 0, tx], [0, d, ty]]
  int32_t status;
};
// `dead`: the box, clipped to the frame, is empty.
__host__ __device__ __forceinline__ TrackSeed track_seed_one(int x0, int y0, int x1, int y1, bool dead, int in_h, int in_w) {
  TrackSeed s;
  s.a = 1.f; s.d = 1.f; s.tx = 0.f; s.ty = 0.f;
  if (!dead) {  // (a box with pixels has x1 > x0 and y1 > y0)
    const double sx = (double)in_w / (double)(x1 - x0), sy = (double)in_h / (double)(y1 - y0);
    s.a = (float)sx;
    s.d = (float)sy;
    s.tx = (float)((0.5 - (double)x0) * sx - 0.5);
    s.ty = (float)((0.5 - (double)y0) * sy - 0.5);
  }
  s.status = dead ? FLM_TRACK_DEAD : 0;
  return s;
}
__host__ __device__ __forceinline__ void track_seed_store(const TrackSeed& s, float* o) {
  o[0] = s.a;  o[1] = 0.f; o[2] = s.tx;
  o[3] = 0.f;  o[4] = s.d; o[5] = s.ty;
}

}  // namespace flm
