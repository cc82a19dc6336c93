// The source taps and 11-bit weights of the crop front-end's resize (cv2's INTER_LINEAR on uint8, restated: flm_misc.hip
// states the whole algorithm above crop_resize_kernel), shared by that kernel and by its NV12 form in
// flm_frames_nv12.hip.
#pragma once

#include "flm_common.h"

namespace flm {

__device__ __forceinline__ void resize_coef(int d, double scale, int n_src, int& s0, int& s1, int& w0, int& w1) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= n_src - 1) { s = n_src - 1; f = 0.f; }
  s0 = s;
  s1 = min(s + 1, n_src - 1);
  w0 = (int)rintf((1.f - f) * 2048.f);
  w1 = (int)rintf(f * 2048.f);
}

// Along y OpenCV clamps only the ROW INDICES (clip(sy + k, 0, h)) and keeps the split weights of the unclamped
// position: on the first / last output rows of an upscale both rows are the border row, weighted b0 and b1 separately
// -- floor(b0*v >> 16) + floor(b1*v >> 16) is not always (2048*v) >> 16, so folding the weights there is off by one LSB.
__device__ __forceinline__ void resize_coef_y(int d, double scale, int n_src, int& s0, int& s1, int& w0, int& w1) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  const int s = (int)floorf(f);
  f -= (float)s;
  s0 = min(max(s, 0), n_src - 1);
  s1 = min(max(s + 1, 0), n_src - 1);
  w0 = (int)rintf((1.f - f) * 2048.f);
  w1 = (int)rintf(f * 2048.f);
}

}  // namespace flm
