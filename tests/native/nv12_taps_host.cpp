// Host sweep of csrc/flm_nv12_dev.h, the tap addressing, conversion and blend that the NV12 kernels run: every clamped
// source position of small frames, inside a heap buffer of exactly the slot's bytes (so that a sanitizer build reports
// any load outside [slot, slot + flm_frame_format_bytes)), against a restatement that converts the whole frame pixel by
// pixel first and then indexes it as the BGR kernels index a BGR frame.  No GPU call is made.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "flm_nv12_dev.h"

static int failures = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (++failures <= 20) { std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                      \
  } while (0)

// include/flm.h, section by section, written out again
static void convert_ref(int Y, int U, int V, int matrix, int bgr[3]) {
  static const int K[2][5] = {{1220542, 2116026, -409993, -852492, 1673527}, {1220945, 2215014, -223607, -558796, 1879825}};
  const int* k = K[matrix];
  const int yy = (Y - 16 > 0 ? Y - 16 : 0) * k[0];
  const int u = U - 128, v = V - 128;
  const int acc[3] = {yy + k[1] * u + (1 << 19), yy + k[3] * v + k[2] * u + (1 << 19), yy + k[4] * v + (1 << 19)};
  for (int c = 0; c < 3; ++c) {
    const int s = acc[c] >> 20;
    bgr[c] = s < 0 ? 0 : s > 255 ? 255 : s;
  }
}

static unsigned bits(float f) {
  unsigned b;
  std::memcpy(&b, &f, 4);
  return b;
}

static long long sweep(int fh, int fw, unsigned y_pitch, unsigned uv_pitch, unsigned uv_off, int matrix, unsigned seed) {
  flm::Nv12Geom g;
  g.fh = fh; g.fw = fw; g.y_pitch = y_pitch; g.uv_pitch = uv_pitch; g.uv_off = uv_off;
  const size_t bytes = (size_t)flm::nv12_slot_bytes(g);
  CHECK(bytes == (size_t)uv_off + (size_t)(fh / 2 - 1) * uv_pitch + fw, "slot bytes");
  uint8_t* slot = static_cast<uint8_t*>(std::malloc(bytes));  // exactly the bytes a kernel may read
  unsigned r = seed * 2654435761u + 12345u;
  for (size_t i = 0; i < bytes; ++i) {
    r = r * 1664525u + 1013904223u;
    const unsigned v = r >> 24;
    slot[i] = (uint8_t)((r >> 8) % 5 == 0 ? (v & 1 ? 255 : 0) : v);  // a fifth of the bytes at the extremes: the clamps
  }
  const flm::Nv12Coef kc = flm::nv12_coef(matrix);
  // the converted frame, pixel by pixel
  std::vector<int> bgr((size_t)fh * fw * 3);
  for (int y = 0; y < fh; ++y)
    for (int x = 0; x < fw; ++x) {
      const uint8_t* c = slot + uv_off + (size_t)(y >> 1) * uv_pitch + (x & ~1);
      convert_ref(slot[(size_t)y * y_pitch + x], c[0], c[1], matrix, &bgr[((size_t)y * fw + x) * 3]);
    }
  long long n = 0;
  // a single tap anywhere (the crop / resize and the converter's ragged edge)
  for (int y = 0; y < fh; ++y)
    for (int x = 0; x < fw; ++x) {
      int p[3];
      flm::nv12_tap_bgr(slot, g, kc, x, y, p);
      const int* e = &bgr[((size_t)y * fw + x) * 3];
      CHECK(p[0] == e[0] && p[1] == e[1] && p[2] == e[2], "tap %dx%d (%d,%d): %d %d %d != %d %d %d", fh, fw, x, y, p[0],
            p[1], p[2], e[0], e[1], e[2]);
      int q[3];
      flm::nv12_to_bgr(slot[(size_t)y * y_pitch + x], 128, 128, kc, q);
      CHECK(q[0] == q[1] && q[1] == q[2], "grey is not grey");
      ++n;
    }
  // the four taps of a warp sample: every (x0, y0) warp_position can return, a few weights each
  const float W[5] = {0.f, 0.25f, 0.5f, 0.8125f, 0.99999994f};
  for (int y0 = 0; y0 < fh; ++y0)
    for (int x0 = 0; x0 < fw; ++x0)
      for (int a = 0; a < 5; ++a)
        for (int b = 0; b < 5; ++b) {
          // (xs = fw-1 and ys = fh-1 are reached only exactly: the fraction is 0 there)
          const float fx = x0 == fw - 1 ? 0.f : W[a], fy = y0 == fh - 1 ? 0.f : W[b];
          flm::Nv12Taps t;
          flm::nv12_gather(slot, g, x0, y0, fx, fy, t);
          float out[3];
          flm::nv12_blend(t, kc, out);
          // warp_sample_any's indexing on the converted frame, warp_blend_u8's three fmafs
          const int x1 = x0 + 1 < fw ? x0 + 1 : fw - 1, y1 = y0 + 1 < fh ? y0 + 1 : fh - 1;
          for (int c = 0; c < 3; ++c) {
            const float p00 = (float)bgr[((size_t)y0 * fw + x0) * 3 + c], p01 = (float)bgr[((size_t)y0 * fw + x1) * 3 + c];
            const float p10 = (float)bgr[((size_t)y1 * fw + x0) * 3 + c], p11 = (float)bgr[((size_t)y1 * fw + x1) * 3 + c];
            const float top = std::fmaf(fx, p01 - p00, p00);
            const float bot = std::fmaf(fx, p11 - p10, p10);
            const float e = std::fmaf(fy, bot - top, top);
            CHECK(bits(out[c]) == bits(e), "blend %dx%d pitch %u/%u off %u (%d,%d) fx %g fy %g c %d: %.9g != %.9g", fh, fw,
                  y_pitch, uv_pitch, uv_off, x0, y0, (double)fx, (double)fy, c, (double)out[c], (double)e);
          }
          ++n;
        }
  std::free(slot);
  return n;
}

int main() {
  const int sizes[][2] = {{2, 2}, {4, 2}, {2, 4}, {6, 4}, {4, 6}, {4, 8}};
  long long n = 0;
  unsigned seed = 1;
  for (const auto& s : sizes) {
    const int fh = s[0], fw = s[1];
    for (int matrix = 0; matrix < 2; ++matrix) {
      n += sweep(fh, fw, fw, fw, fw * fh, matrix, seed++);                         // dense
      n += sweep(fh, fw, fw + 3, fw + 1, (fw + 3) * fh + 5, matrix, seed++);       // padded pitches, odd U,V offset
      n += sweep(fh, fw, fw + 2, fw + 6, (fw + 2) * (fh + 2), matrix, seed++);     // U,V plane at a later row
    }
  }
  // the grey points of include/flm.h
  for (int matrix = 0; matrix < 2; ++matrix) {
    const flm::Nv12Coef kc = flm::nv12_coef(matrix);
    int p[3];
    flm::nv12_to_bgr(16, 128, 128, kc, p);
    CHECK(p[0] == 0 && p[1] == 0 && p[2] == 0, "Y=16 is not black");
    flm::nv12_to_bgr(235, 128, 128, kc, p);
    CHECK(p[0] == 255 && p[1] == 255 && p[2] == 255, "Y=235 is not white");
    for (int Y = 0; Y < 256; Y += 5)
      for (int U = 0; U < 256; U += 3)
        for (int V = 0; V < 256; V += 3) {
          int e[3];
          flm::nv12_to_bgr(Y, U, V, kc, p);
          convert_ref(Y, U, V, matrix, e);
          CHECK(p[0] == e[0] && p[1] == e[1] && p[2] == e[2], "convert %d %d %d", Y, U, V);
        }
  }
  std::printf("nv12 taps: %lld positions checked, %d failures\n", n, failures);
  return failures ? 1 : 0;
}
