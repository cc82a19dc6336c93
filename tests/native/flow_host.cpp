// The __host__ __device__ arithmetic of csrc/flm_flow_dev.h -- luma, pyramid pixel, sample, solve, gates, the whole flow of
// a point -- run on the host over cases a test writes (tests/test_flow_native_host.py), which compares every byte of the
// answer with tests/flow_ref.py.  Built without contraction, as the library is; this is also the program to build with
// the host's address and undefined-behaviour sanitizers.
//
//   flow_host IN OUT
// IN:  int32 n_cases; per case: int32 {h, w, ch, levels, radius, max_iter, c, 0}, double {eps, min_eig, max_err, max_move},
//      float m[6], double lm[c*2], uint8 prev[h*w*ch], uint8 cur[h*w*ch]
// OUT: per case: uint8 pyr_prev[bytes], uint8 pyr_cur[bytes], then per point double {x, y}, int32 {err, flags}
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "flm_flow_dev.h"

using namespace flm;

static void must(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "flow_host: %s\n", what);
    std::exit(2);
  }
}

template <class T>
static void rd(FILE* f, T* p, size_t n) { must(std::fread(p, sizeof(T), n, f) == n, "short read"); }
template <class T>
static void wr(FILE* f, const T* p, size_t n) { must(std::fwrite(p, sizeof(T), n, f) == n, "short write"); }

static std::vector<uint8_t> pyramid(const std::vector<uint8_t>& src, int h, int w, int ch, int levels) {
  std::vector<uint8_t> p(flow_level_offset(h, w, levels));
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const uint8_t* q = &src[((size_t)y * w + x) * ch];
      p[(size_t)y * w + x] = (uint8_t)(ch == 1 ? q[0] : flow_luma(q[0], q[1], q[2]));
    }
  for (int l = 1; l < levels; ++l) {
    const uint8_t* a = p.data() + flow_level_offset(h, w, l - 1);
    uint8_t* b = p.data() + flow_level_offset(h, w, l);
    const int wa = w >> (l - 1), hb = h >> l, wb = w >> l;
    for (int y = 0; y < hb; ++y)
      for (int x = 0; x < wb; ++x) {
        const uint8_t* q = a + (size_t)(2 * y) * wa + 2 * x;
        b[(size_t)y * wb + x] = (uint8_t)flow_down(q[0], q[1], q[wa], q[wa + 1]);
      }
  }
  return p;
}

int main(int argc, char** argv) {
  must(argc == 3, "usage: flow_host IN OUT");
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  must(in && out, "cannot open the files");
  int32_t n_cases = 0;
  rd(in, &n_cases, 1);
  long points = 0;
  for (int t = 0; t < n_cases; ++t) {
    int32_t hd[8];
    double od[4];
    float m[6];
    rd(in, hd, 8);
    rd(in, od, 4);
    rd(in, m, 6);
    const int h = hd[0], w = hd[1], ch = hd[2], c = hd[6];
    FlowParams o;
    o.levels = hd[3]; o.radius = hd[4]; o.max_iter = hd[5];
    o.eps = od[0]; o.min_eig = od[1]; o.max_err = od[2]; o.max_move = od[3];
    must(h >= 1 && w >= 1 && (ch == 1 || ch == 3) && o.levels >= 1 && o.levels <= kFlowMaxLevels && o.radius >= 1 &&
             o.radius <= kFlowMaxRadius && c >= 0, "bad case header");
    std::vector<double> lm((size_t)c * 2);
    std::vector<uint8_t> prev((size_t)h * w * ch), cur((size_t)h * w * ch);
    rd(in, lm.data(), lm.size());
    rd(in, prev.data(), prev.size());
    rd(in, cur.data(), cur.size());
    const std::vector<uint8_t> pp = pyramid(prev, h, w, ch, o.levels), pc = pyramid(cur, h, w, ch, o.levels);
    wr(out, pp.data(), pp.size());
    wr(out, pc.data(), pc.size());
    for (int i = 0; i < c; ++i) {
      double q[2];
      int32_t ef[2];
      ef[1] = flow_point(pp.data(), pc.data(), h, w, m, lm[2 * i], lm[2 * i + 1], o, &q[0], &q[1], &ef[0]);
      if (ef[1] != 0) q[0] = q[1] = -1.0;
      wr(out, q, 2);
      wr(out, ef, 2);
      ++points;
    }
  }
  std::fclose(in);
  must(std::fclose(out) == 0, "close failed");
  std::printf("flow_host: %d cases, %ld points, 0 failures\n", n_cases, points);
  return 0;
}
