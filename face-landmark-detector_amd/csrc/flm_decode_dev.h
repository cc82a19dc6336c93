// Device pieces shared by the heatmap decode (flm_decode.hip) and its landmark-record form (flm_decode_stats.hip): the
// argument block, the two tile streams, the merge of the chunk lists and the all-pixel lane sums.  flm_decode.hip's
// header comment describes the two passes they serve.
#pragma once
#include "flm_common.h"
#include "flm_topn_dev.h"

namespace flm {

constexpr int PT = 64;  // pixels per tile

// One argument block for every kernel of this file.  flm_decode in top-n mode is the sweep with one mode (n_max = n,
// n_modes = 1); flm_decode in all-pixel mode uses `sums` and `out` only.
struct DecodeArgs {
  const float* hm;
  int n, h, w, l;
  int chunks, chunk_px;  // decode_plan's; chunk_px multiple of 64
  int vec;               // face stride is a multiple of 16 bytes: 16-byte loads allowed
  int n_max;             // largest top-n mode (0: all-pixel modes only)
  int has_all;           // some mode is 0
  float thresh;
  unsigned long long* keys;  // [n][chunks][l][n_max]
  double* sums;              // [n][chunks][l][3]
  double* out;               // [n_modes][n][l][2]
  const unsigned* gate;      // non-null: the launch does nothing unless *gate != 0
  int n_modes;
  int modes[FLM_SWEEP_MAX_MODES];
  // compact batch (top-n kernels; the per-face fallback of the forward): hm holds n rows, of which those at index
  // *rows_cnt and beyond are skipped; row r's result goes to out[rows[r]].  Both null: row = face.
  const int* rows;
  const unsigned* rows_cnt;
};

// nothing to do for map row `row`: the launch is gated off, or the row lies beyond the compact batch's live rows
__device__ __forceinline__ bool decode_row_off(const DecodeArgs& a, int row) {
  if (a.gate && *a.gate == 0) return true;
  return a.rows_cnt && (unsigned)row >= *a.rows_cnt;
}
// the face whose result map row `row` holds
__device__ __forceinline__ int decode_out_face(const DecodeArgs& a, int row) { return a.rows ? a.rows[row] : row; }

// the pixel range [p_begin, p_end) of workgroup (chunk, face)
struct Chunk {
  int face, chunk, p_begin, p_end;
};
__device__ __forceinline__ Chunk chunk_of(const DecodeArgs& a) {
  Chunk k;
  k.face = blockIdx.y;
  k.chunk = blockIdx.x;
  k.p_begin = k.chunk * a.chunk_px;
  k.p_end = min(k.p_begin + a.chunk_px, a.h * a.w);
  return k;
}

// 16 bytes of a map that is read exactly once: the non-temporal hint keeps the stream from displacing everything else in
// the L2 (standalone top-4 decode of 68-landmark maps, LDS-DMA form: 0.253 -> 0.234 ms at batch 64, 1.63 -> 1.49 ms at 512)
__device__ __forceinline__ float4 load_stream16(const float* p) {
  typedef float f4v __attribute__((ext_vector_type(4)));
  const f4v v = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}

// ---- the tile stream, register-prefetch form --------------------------------------------------------------------------
// A tile of 64 pixels x L channels on its way from HBM to LDS: up to 6 x 16 bytes per thread cover L <= 96.  (Every
// loop over r[] is fully unrolled, so the array lives in registers; tests/test_build_hygiene.py fails on scratch.)
struct PrefetchTile {
  float4 r[6];
  __device__ __forceinline__ void load(const float* nsrc, int tid, int tile_f) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int e4 = tid * 4 + 1024 * i;
      if (e4 < tile_f) r[i] = load_stream16(nsrc + e4);
    }
  }
  __device__ __forceinline__ void store(float* tile, int tid, int tile_f, int L, int LS) const {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int e4 = tid * 4 + 1024 * i;
      if (e4 < tile_f) {
        int p = e4 / L, c = e4 - p * L;
        tile[p * LS + c] = r[i].x; if (++c == L) { c = 0; ++p; }
        tile[p * LS + c] = r[i].y; if (++c == L) { c = 0; ++p; }
        tile[p * LS + c] = r[i].z; if (++c == L) { c = 0; ++p; }
        tile[p * LS + c] = r[i].w;
      }
    }
  }
};

// The pixels [p_begin, p_end) of one face (`src`) on their way through `tile` ([PT][L | 1] floats of LDS), a tile of 64
// pixels per stage().  The NEXT tile is prefetched into registers before the current one is processed, so the HBM
// latency hides behind the selection work; a partial tile, or a face whose stride is not a multiple of 16 bytes (!vec),
// takes plain loads with zero fill.
struct TileStream {
  float* tile;
  const float* src;
  int L, p_end, vec, tid;
  PrefetchTile pf;
  bool pf_valid;
  __device__ __forceinline__ TileStream(float* tile_, const float* src_, int L_, int p_begin, int p_end_, int vec_, int tid_)
      : tile(tile_), src(src_), L(L_), p_end(p_end_), vec(vec_), tid(tid_) {
#pragma unroll
    for (int i = 0; i < 6; ++i) pf.r[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    pf_valid = false;
    if (vec && p_begin + PT <= p_end) {
      pf.load(src + (size_t)p_begin * L, tid, PT * L);
      pf_valid = true;
    }
  }
  // tile p0 .. p0 + PT - 1 into LDS, between two barriers; returns its number of pixels
  __device__ __forceinline__ int stage(int p0) {
    const int LS = L | 1;
    const int tile_f = PT * L;  // floats per full tile (multiple of 4 because PT is)
    const int npx = min(PT, p_end - p0);
    const int nf = npx * L;
    __syncthreads();
    if (pf_valid) {
      pf.store(tile, tid, tile_f, L, LS);
    } else {
      const float* tsrc = src + (size_t)p0 * L;
      for (int e = tid; e < tile_f; e += 256) {
        const int p = e / L, c = e - p * L;
        tile[p * LS + c] = (e < nf) ? tsrc[e] : 0.f;
      }
    }
    pf_valid = vec && p0 + 2 * PT <= p_end;
    if (pf_valid) pf.load(src + (size_t)(p0 + PT) * L, tid, tile_f);
    __syncthreads();
    return npx;
  }
};

// ---- the tile stream for 68-landmark maps, tiles brought in by LDS-DMA (round 3) ---------------------------------------
// What bounded the form above at batch 64 (0.31 ms, 0.49 of 8 TB/s) is bytes in flight: one 17 KiB tile of register
// prefetch per workgroup, three workgroups per CU, 51 KiB per CU against ~3 us of loaded HBM latency.  Here a tile goes
// from HBM to LDS by buffer_load ... lds (17 requests of 1 KiB; inline assembly as in flm_igemm_args.h, so that
// hipcc does not order the tile's ds_reads behind every pending request) into a ring of three slots: while tile t is
// processed, tiles t+1 and t+2 are in flight -- twice the bytes, no prefetch registers.  The image of a tile is then the
// plain [pixel][68] array (rows of 272 bytes: an odd row stride is not available to a DMA): a wave owns channels
// 16w .. 16w+15 and 64+w and reads its pixel's values as four ds_read_b128 + one b32 -- lanes 272 bytes apart cover all
// 32 banks once per 8 lanes, conflict-free.  The tail of a chunk is zero-filled by the buffer bounds check
// (num_records = the chunk's bytes; the tile offset rides in the VECTOR offset, the one the check looks at).
// The requests carry `nt`: the map is read once (0.253 -> 0.234 ms at batch 64, 1.63 -> 1.49 ms at 512).
// One barrier per tile: a wave waits for its own requests of tile t (vmcnt), the barrier makes every wave's pieces
// visible and proves that tile t-1 has been read by all, then tile t+2 is requested into t-1's slot.
constexpr int DL = 68, D_TILE_B = PT * DL * 4, D_PIECES = D_TILE_B / 1024, D_RING = 3, D_PPW = (D_PIECES + 3) / 4;
constexpr int D_CPW = 17;
static_assert(D_TILE_B % 1024 == 0 && D_PPW == 5, "17 pieces of 1 KiB: five per wave, the missing ones repeat piece w");

// i-th channel of wave `wave`, and the wave's 17 values of pixel `lane` of a ring slot
__device__ __forceinline__ int dma_channel(int i, int wave) { return i < 16 ? 16 * wave + i : 64 + wave; }
__device__ __forceinline__ void dma_read_pixel(const char* slot, int lane, int wave, float v[D_CPW]) {
  const char* tile = slot + lane * (DL * 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float4 q = *reinterpret_cast<const float4*>(tile + (16 * wave + 4 * j) * 4);
    v[4 * j] = q.x; v[4 * j + 1] = q.y; v[4 * j + 2] = q.z; v[4 * j + 3] = q.w;
  }
  v[16] = *reinterpret_cast<const float*>(tile + (64 + wave) * 4);
}

// The pixels [p_begin, p_end) (not empty) of one face on their way through `ring` ([D_RING][PT][DL] floats of LDS).
// `wave` is uniform (an SGPR).
struct DmaRing {
  typedef int dsrd_t __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) char lds_char;
  const char* ring;
  unsigned ring_lds;
  dsrd_t srd;
  int ntiles, lane, wave;
  __device__ __forceinline__ DmaRing(char* ring_, const float* src, int p_begin, int p_end, int lane_, int wave_)
      : ring(ring_), ntiles((p_end - p_begin + PT - 1) / PT), lane(lane_), wave(wave_) {
    ring_lds = (unsigned)(size_t)((lds_char*)ring_);
    const unsigned long long cb = reinterpret_cast<unsigned long long>(src + (size_t)p_begin * DL);
    srd = (dsrd_t){(int)(unsigned)cb, (int)(unsigned)((cb >> 32) & 0xffffu), (p_end - p_begin) * DL * 4, 0x00020000};
    issue(0);
    if (ntiles > 1) issue(1);
  }
  // piece k of a tile: bytes [1024 k, 1024 k + 1024); this wave's pieces wave, wave + 4, ... (five requests per tile and
  // wave so that the vmcnt arithmetic is the same in every wave: a piece past the 17th repeats piece `wave`)
  __device__ __forceinline__ void issue(int t) const {
    const unsigned slot = ring_lds + (unsigned)(t % D_RING) * D_TILE_B;
#pragma unroll
    for (int j = 0; j < D_PPW; ++j) {
      const int k = wave + 4 * j < D_PIECES ? wave + 4 * j : wave;
      asm volatile("s_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen nt lds"
                   :
                   : "v"((unsigned)t * D_TILE_B + (unsigned)k * 1024u + (unsigned)lane * 16u), "s"(srd), "{m0}"(slot + k * 1024)
                   : "memory");
    }
  }
  // tile t complete in its slot (returned), tile t + 2 requested
  __device__ __forceinline__ const char* stage(int t) const {
    if (t + 1 < ntiles) __builtin_amdgcn_s_waitcnt(0x0f75);  // vmcnt(5): tile t's five requests done, tile t+1's may fly
    else __builtin_amdgcn_s_waitcnt(0x0f70);
    __syncthreads();
    if (t + 2 < ntiles) issue(t + 2);
    return ring + (size_t)(t % D_RING) * D_TILE_B;
  }
};

// the chunk lists of (face, c) merged to the face's top n_max
template <bool WIDE>
__device__ __forceinline__ void merge_chunk_lists(const DecodeArgs& a, int face, int c, int lane, unsigned long long& list,
                                                  unsigned long long& list_hi, unsigned long long& tau) {
  const int L = a.l, n_max = a.n_max;
  const unsigned long long* part = a.keys + (size_t)face * a.chunks * L * n_max;
  if constexpr (WIDE) {  // 64 < n <= 128: a chunk's list arrives in two batches of up to 64 keys
    for (int s = 0; s < a.chunks; ++s)
      for (int r0 = 0; r0 < n_max; r0 += 64) {
        const unsigned long long cand = r0 + lane < n_max ? part[((size_t)s * L + c) * n_max + r0 + lane] : 0ull;
        if (__any(cand > tau)) insert_candidates_wide(list, list_hi, tau, cand, n_max, lane);
      }
  } else {
    // 64 / n_max chunk lists are merged per pass (lane -> (chunk offset, rank))
    const int per = 64 / n_max;
    for (int s0 = 0; s0 < a.chunks; s0 += per) {
      const int s = s0 + lane / n_max, rk = lane % n_max;
      const unsigned long long cand =
          (lane < per * n_max && s < a.chunks) ? part[((size_t)s * L + c) * n_max + rk] : 0ull;
      if (__any(cand > tau)) insert_candidates(list, tau, cand, n_max, lane);
    }
  }
}

// flm_decode's all-pixel mode: every lane keeps float64 sums of its pixel column per channel, reduced over the wave by
// a fixed-order butterfly (deterministic) at the end of the chunk.
__device__ __forceinline__ void lane_sums_add(double hv, double dx, double dy, double& s0, double& sx, double& sy) {
  s0 += hv;
  sx = fma(hv, dx, sx);
  sy = fma(hv, dy, sy);
}
__device__ __forceinline__ void lane_sums_write(double* part, int lane, double v0, double v1, double v2) {
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) {
    v0 += __shfl_xor(v0, sh);
    v1 += __shfl_xor(v1, sh);
    v2 += __shfl_xor(v2, sh);
  }
  if (lane == 0) {
    part[0] = v0;
    part[1] = v1;
    part[2] = v2;
  }
}

// flm_decode_stats.hip: the launches of flm_decode_stats that differ from flm_decode's (decode_run, flm_decode.hip, plans
// them and fills the arguments; there `out` takes the records [n][l][FLM_LANDMARK_REC] and `sums` six entries per
// (chunk, landmark)).  Top-n: pass 1 is flm_decode's own launch, this is the merge.  All-pixel: both passes.
int launch_decode_merge_stats(hipStream_t s, dim3 mgrid, const DecodeArgs& a, bool wide);
int launch_decode_all_stats(hipStream_t s, dim3 grid, dim3 mgrid, const DecodeArgs& a, bool dma, bool big, size_t tile_lds,
                            size_t ring_lds);

}  // namespace flm
