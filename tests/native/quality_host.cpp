// Host sweep of csrc/flm_quality_dev.h, the per-pixel pieces flm_face_quality's kernel is built from.
//   1. Every uint8 (B, G, R) triple, 2^24 of them, through the element conversion, the quantise step under the identity
//      format and the luma: p must be 16 * x, Y must lie in [0, 4080] and equal a restatement in __int128.
//   2. Every 16-bit pattern, as binary16 and as bfloat16, through the element conversion (against a decoder written from
//      the bit fields) and the de-normalise and quantise step, with the matcher's scale and bias and with the identity:
//      a NaN gives 0, the infinities clamp, and every result equals a long-double restatement with one rounding to
//      float32 per operation.  The restatement is exact before each rounding: a difference of a 16-bit value and +-1
//      either fits the 64-bit significand of long double or has a term below 2^-56 of the other, which cannot bring the
//      long-double result to a float32 midpoint; a product of two float32 values has 48 significant bits.
// Built with the host's address and undefined-behaviour sanitizers.  No GPU call is made.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "flm_quality_dev.h"

typedef __int128 i128;

static long long failures = 0, checks = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    ++checks;                                              \
    if (!(cond)) {                                         \
      if (++failures <= 20) { std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                      \
  } while (0)

static uint32_t bits_of(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}

// binary16 from its fields: (-1)^s * 2^(e-15) * (1 + m/1024), subnormals 2^-14 * m/1024
static long double half_ref(uint16_t b, bool* nan) {
  const int s = b >> 15, e = (b >> 10) & 31, m = b & 1023;
  *nan = e == 31 && m != 0;
  long double v;
  if (e == 31) v = INFINITY;
  else if (e == 0) v = std::ldexp((long double)m, -24);
  else v = std::ldexp((long double)(1024 + m), e - 25);
  return s ? -v : v;
}
// bfloat16 from its fields: 8 exponent bits (bias 127), 7 fraction bits
static long double bf16_ref(uint16_t b, bool* nan) {
  const int s = b >> 15, e = (b >> 7) & 255, m = b & 127;
  *nan = e == 255 && m != 0;
  long double v;
  if (e == 255) v = INFINITY;
  else if (e == 0) v = std::ldexp((long double)m, -133);
  else v = std::ldexp((long double)(128 + m), e - 134);
  return s ? -v : v;
}

// include/flm.h: t = xf - bias, v = t * inv, p = clamp(rint(v * 16), 0, 4080), a NaN giving 0
static int quant_ref(long double xf, bool nan, float bias, float inv) {
  if (nan) return 0;
  const float t = (float)(xf - (long double)bias);
  const float v = (float)((long double)t * (long double)inv);
  const float v16 = (float)((long double)v * 16.0L);
  if (std::isnan(v16)) return 0;  // (0 * inf, inf - inf)
  const long double r = std::rint((long double)v16);  // to nearest, ties to even: the default rounding mode
  return r < 0.0L ? 0 : r > 4080.0L ? 4080 : (int)r;
}

template <int TYPE>
static void sweep16(const char* name, long double (*decode)(uint16_t, bool*), float scale, float bias) {
  const float inv = 1.0f / scale;
  for (uint32_t b = 0; b < 65536; ++b) {
    bool nan;
    const long double x = decode((uint16_t)b, &nan);
    const float xf = flm::QPix<TYPE>::load((uint16_t)b);
    if (nan) CHECK(std::isnan(xf), "%s 0x%04x: a NaN decodes to %g", name, b, (double)xf);
    else CHECK((long double)xf == x, "%s 0x%04x: decodes to %g, expected %Lg", name, b, (double)xf, x);
    const int p = flm::quality_quant(xf, bias, inv), e = quant_ref(x, nan, bias, inv);
    CHECK(p == e, "%s 0x%04x (%g) scale %g bias %g: p = %d, expected %d", name, b, (double)xf, (double)scale, (double)bias,
          p, e);
    CHECK(p >= 0 && p <= flm::kQualityMaxP, "%s 0x%04x: p = %d outside [0, 4080]", name, b, p);
    if (nan) CHECK(p == 0, "%s 0x%04x: a NaN gives %d", name, b, p);
    if (!nan && std::isinf(x) && inv > 0) CHECK(p == (x > 0 ? 4080 : 0), "%s 0x%04x: an infinity gives %d", name, b, p);
  }
}

int main() {
  // ---- 1. every uint8 triple ----
  int p8[256];
  for (int x = 0; x < 256; ++x) {
    p8[x] = flm::quality_quant(flm::QPix<FLM_PIX_U8>::load((uint8_t)x), 0.0f, 1.0f);
    CHECK(p8[x] == 16 * x, "uint8 %d quantises to %d", x, p8[x]);
  }
  int ymin = 1 << 30, ymax = -1;
  for (int b = 0; b < 256; ++b)
    for (int g = 0; g < 256; ++g)
      for (int r = 0; r < 256; ++r) {
        const int y = flm::quality_luma(p8[b], p8[g], p8[r]);
        const i128 wide = ((i128)1868 * (16 * b) + (i128)9617 * (16 * g) + (i128)4899 * (16 * r) + 8192) / 16384;
        CHECK(y >= 0 && y <= 4080 && (i128)y == wide, "luma(%d,%d,%d) = %d, expected %lld", b, g, r, y, (long long)wide);
        ymin = y < ymin ? y : ymin;
        ymax = y > ymax ? y : ymax;
      }
  CHECK(ymin == 0 && ymax == 4080, "luma range [%d, %d]", ymin, ymax);
  CHECK(1868 + 9617 + 4899 == 16384, "the weights do not sum to 2^14");
  for (int x = 0; x < 256; ++x)  // a grey pixel keeps its level
    CHECK(flm::quality_luma(16 * x, 16 * x, 16 * x) == 16 * x, "grey %d", x);

  // ---- 2. every 16-bit pattern, both types, the matcher's format and the identity ----
  const float sc = (float)(1.0 / 127.5), bi = -1.0f;  // alignment.AlignedFormat.matcher(): x * (1/127.5) - 1
  sweep16<FLM_PIX_F16>("binary16", half_ref, sc, bi);
  sweep16<FLM_PIX_F16>("binary16", half_ref, 1.0f, 0.0f);
  sweep16<FLM_PIX_BF16>("bfloat16", bf16_ref, sc, bi);
  sweep16<FLM_PIX_BF16>("bfloat16", bf16_ref, 1.0f, 0.0f);
  // float32 passes through with its bits
  const float probe[] = {0.0f, -0.0f, 1.5f, 255.0f, 1e-40f, INFINITY};
  for (float f : probe) CHECK(bits_of(flm::QPix<FLM_PIX_F32>::load(f)) == bits_of(f), "float32 %g changed", (double)f);
  // ties go to even: 0.5 and 1.5 sixteenths
  CHECK(flm::quality_quant(0.03125f, 0.0f, 1.0f) == 0 && flm::quality_quant(0.09375f, 0.0f, 1.0f) == 2, "ties to even");

  std::printf("quality_host: %lld checks, %lld failures\n", checks, failures);
  return failures ? 1 : 0;
}
