// csrc/flm_parts_dev.h on the host: the fit of a part, the openness record of a measure and the step of its blink state,
// run over the cases tests/test_parts_native_host.py writes.  Every buffer is a heap allocation of exactly the bytes the
// case has, so the host's address sanitizer sees any read past a landmark, weight, index or template array.
//
//   parts_host IN OUT
// IN:  int32 n_fit, then per fit   { int32 c, n, has_w, 0; int32 idx[n]; double tmpl[2n]; double lm[2c]; double w[c] if has_w }
//      int32 n_rec, then per record { int32 c, has_w, wa, wb, v, 0, 0, 0; int32 up[4], lo[4]; double min_width;
//                                     double lm[2c]; double w[c] if has_w }
//      int32 n_seq, then per sequence { int32 ticks, 0; double th[4]; double st[8];
//                                       per tick { int32 ok, status, reset, 0; double o, dt; int64 frame_id } }
// OUT: per fit 6 floats and int32 ok; per record 4 doubles; per sequence and tick 8 doubles.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "flm_parts_dev.h"

using namespace flm;

template <class T>
static T* take(FILE* f, size_t n) {  // an exact heap copy of the next n elements
  T* p = static_cast<T*>(malloc(n ? n * sizeof(T) : 1));
  if (n && fread(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "short input\n");
    exit(2);
  }
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int failures = 0;
  int32_t* cnt = take<int32_t>(in, 1);
  const int n_fit = cnt[0];
  free(cnt);
  for (int t = 0; t < n_fit; ++t) {
    int32_t* h = take<int32_t>(in, 4);
    const int c = h[0], n = h[1], has_w = h[2];
    int32_t* idx = take<int32_t>(in, n);
    double* tmpl = take<double>(in, 2 * (size_t)n);
    double* lm = take<double>(in, 2 * (size_t)c);
    double* w = has_w ? take<double>(in, c) : nullptr;
    double* pt = static_cast<double*>(malloc(sizeof(double) * kPartPt * n));
    for (int i = 0; i < n; ++i) part_stage(pt + kPartPt * i, lm, 2, w, 1, 0, c, idx[i], tmpl + 2 * i);
    float m[6];
    const int32_t ok = part_fit(pt, n, m) ? 1 : 0;
    if (!ok && !(m[0] == 1.f && m[1] == 0.f && m[2] == 0.f && m[3] == 0.f && m[4] == 1.f && m[5] == 0.f)) ++failures;
    fwrite(m, sizeof(float), 6, out);
    fwrite(&ok, sizeof(ok), 1, out);
    free(h); free(idx); free(tmpl); free(lm); free(w); free(pt);
  }
  cnt = take<int32_t>(in, 1);
  const int n_rec = cnt[0];
  free(cnt);
  for (int t = 0; t < n_rec; ++t) {
    int32_t* h = take<int32_t>(in, 8);
    const int c = h[0], has_w = h[1];
    int32_t* ul = take<int32_t>(in, 8);
    double* mw = take<double>(in, 1);
    double* lm = take<double>(in, 2 * (size_t)c);
    double* w = has_w ? take<double>(in, c) : nullptr;
    double rec[FLM_OPEN_REC];
    const bool ok = open_record(lm, 2, w, 1, 0, c, h[2], h[3], h[4], ul, ul + 4, mw[0], rec);
    if (ok != (rec[2] == 1.0) || (!ok && rec[0] != -1.0)) ++failures;
    fwrite(rec, sizeof(double), FLM_OPEN_REC, out);
    free(h); free(ul); free(mw); free(lm); free(w);
  }
  cnt = take<int32_t>(in, 1);
  const int n_seq = cnt[0];
  free(cnt);
  for (int t = 0; t < n_seq; ++t) {
    int32_t* h = take<int32_t>(in, 2);
    double* th = take<double>(in, 4);
    double* st = take<double>(in, FLM_OPEN_STATE);
    const OpenThresholds thr{th[0], th[1], th[2], th[3]};
    for (int i = 0; i < h[0]; ++i) {
      int32_t* k = take<int32_t>(in, 4);
      double* od = take<double>(in, 2);
      int64_t* fid = take<int64_t>(in, 1);
      if (k[2]) open_state_reset(st);
      open_state_step(st, k[0] != 0, od[0], k[1], od[1], thr, fid[0]);
      fwrite(st, sizeof(double), FLM_OPEN_STATE, out);
      free(k); free(od); free(fid);
    }
    free(h); free(th); free(st);
  }
  fclose(in);
  fclose(out);
  printf("parts_host: %d fits, %d records, %d sequences, %d failures\n", n_fit, n_rec, n_seq, failures);
  return failures ? 1 : 0;
}
