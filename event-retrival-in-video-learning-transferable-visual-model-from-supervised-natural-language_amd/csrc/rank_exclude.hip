// Exclusion mask (gfx950): one streaming pass over the corpus that clears, in a row bitmask, every
// visible row similar to one of up to 32 hits, and counts the cleared rows per hit.  It is the
// step that lets distinct top-k (rank_collapse.hip) refill a pool that held fewer than k distinct
// frames: rank a pool, collapse it, mask out everything similar to the accepted hits, rank again
// (tests/exclude_ref.py states the pass in NumPy).
//
// Reference call sites this serves: the `top_k * 3` over-fetch, then filter, of the strategies
// (query_strategies.py:55, 141), which returns fewer than top_k frames on static footage.
//
// Semantics (include/miclip.h mi_rank_exclude):
//   sim(a, b) is rank_collapse.hip's: dot / (|a| |b|) of the stored rows widened exactly to f32, all
//   three sums in f32 on the exact-f32 MFMA; a row or hit whose sum of squares is zero or not finite
//   is similar to nothing; NaN >= theta is false.  Row r is removed when it is visible in mask_in
//   and (similar to some hit, or named by some hit_index[m] - index_base); it is attributed to the
//   lowest similar slot, else to the lowest slot that names it.  mask_out = mask_in and not removed,
//   bits of rows >= N written 0; out_count[m] = removed rows attributed to slot m.
//
// Kernel: the hits are the "queries" of rank_pass.hpp's tile geometry (col = hit = lane & 31),
// staged in LDS once per workgroup with their sums of squares (the row sums' fmaf order, so a hit
// that is a stored row has that row's norm bit for bit).  A workgroup's row range is a multiple of
// 384 rows, so a wave's 32-row tile is one mask word.  At entry lane t of a wave reads the word of
// the wave's tile t; tiles whose word is 0 get their 0 written there and are neither loaded nor
// scored (rank_filter.hip's entry scan).  The live tiles run as one stream of 32-k chunks through
// three register buffers (rank_pass.hpp's stream_pass ring); a finished tile gives, per
// accumulator register, one __ballot of `sim >= theta` = 2 rows x 32 hits (rank_collapse.hip's
// idiom): a non-zero half removes the row, its lowest set bit is the slot.  Lane 0 stores the
// tile's word with an ordinary store; lane m counts slot m in a register.  The waves' counts are
// summed through LDS into one [32] int32 line per workgroup, and rank_exclude_sum adds the lines
// into out_count: no atomics, the counts are deterministic.  Nothing synchronises or allocates.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "internal.hpp"
#include "rank_pass.hpp"

namespace miclip {
namespace {
using namespace rankk;

constexpr int NW = 12;                 // waves per workgroup: one tile round = 384 rows
constexpr int MAX_WAVE_TILES = 64;     // one live bit per tile of a wave
constexpr int64_t MAX_ROWS = (int64_t)NW * MAX_WAVE_TILES * 32;   // rows per workgroup: 24576 = 64 x 384
static_assert(MAX_ROWS % 384 == 0, "row ranges are multiples of 384");

// workgroups of a pass over N rows (monotone in N): one per 384 rows up to 512 (one per CU-slot
// pair), more only when a workgroup's rows would exceed the live bitmap
int64_t exclude_chunks(int64_t N) {
  const int64_t tiles = (N + 383) / 384;
  const int64_t a = tiles < 512 ? tiles : 512;
  const int64_t b = (N + MAX_ROWS - 1) / MAX_ROWS;
  const int64_t m = a > b ? a : b;
  return m > 1 ? m : 1;
}

// LDS: hits [32][D+4] f32, row sums of squares [NW][32], hit sums of squares [32], counts [NW][32]
size_t exclude_lds(int64_t D) { return (size_t)FQ * (D + 4) * 4 + (size_t)NW * 32 * 4 + FQ * 4 + (size_t)NW * 32 * 4; }

template <int DT>
__global__ __launch_bounds__(64 * NW) void rank_exclude_kernel(
    const void* __restrict__ corpus, int64_t N, int64_t D, const float* __restrict__ hits,
    const int64_t* __restrict__ hit_index, int H, int64_t index_base, float theta, const uint32_t* mask_in,
    uint32_t* mask_out, int64_t rows_per_wg, int32_t* __restrict__ lines) {
  constexpr int NT = 64 * NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ts_stride = (int)D + 4;
  float* Ts = (float*)smem;
  float* nrm_all = Ts + FQ * ts_stride;
  float* hss = nrm_all + NW * 32;
  int32_t* cnts = (int32_t*)(hss + FQ);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int64_t r_begin = (int64_t)blockIdx.x * rows_per_wg;   // a multiple of 32
  const int64_t r_end = min(N, r_begin + rows_per_wg);
  const int nrows = (int)(r_end - r_begin);

  // entry scan: lane t owns tile t of this wave (rows r_begin + (wave + NW t) 32 ..)
  const int ntw = (nrows + 31) / 32;
  const int my_tiles = ntw > wave ? (ntw - 1 - wave) / NW + 1 : 0;   // <= MAX_WAVE_TILES
  uint32_t word = 0u;
  if (lane < my_tiles) {
    const int64_t row0 = r_begin + (int64_t)(wave + NW * lane) * 32;   // < r_end <= N
    const int64_t left = N - row0;
    word = mask_in ? mask_in[row0 >> 5] : 0xFFFFFFFFu;
    if (left < 32) word &= (1u << (int)left) - 1u;
    if (word == 0u) mask_out[row0 >> 5] = 0u;   // a dead tile: nothing to remove
  }
  const uint64_t live = __ballot(word != 0u);
  if (!__syncthreads_or(live != 0ull)) {   // no live tile in the workgroup: nothing staged
    if (tid < FQ) lines[(int64_t)blockIdx.x * FQ + tid] = 0;
    return;
  }

  stage_queries(Ts, ts_stride, hits, D, 0, H, NT);
  __syncthreads();
  // hit sums of squares: lane (r, h) of wave 0 sums its half of every 32-k chunk, as score_chunk does
  if (wave == 0) {
    float ss = 0.f;
    const float* tq = Ts + r * ts_stride + 16 * h;
    for (int j = 0; j < (int)(D / 32); ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) ss = fmaf(tq[32 * j + i], tq[32 * j + i], ss);
    ss += __shfl_xor(ss, 32, 64);
    if (h == 0) hss[r] = ss;
  }
  __syncthreads();

  // this lane's hit (column r): its norm, and the row it names relative to r_begin (-1: none here)
  const float hs = hss[r];
  const bool vj = r < H && hs > 0.f && __builtin_isfinite(hs);
  const float sj = sqrtf(hs);
  int own = -1;
  if (lane < H && hit_index) {
    const int64_t idx = hit_index[lane];
    if (idx >= index_base) {
      const uint64_t rel = (uint64_t)idx - (uint64_t)index_base;   // exact: idx >= index_base
      if (rel >= (uint64_t)r_begin && rel < (uint64_t)r_end) own = (int)(rel - (uint64_t)r_begin);
    }
  }

  float* nrm = nrm_all + wave * 32;
  const int nch = (int)(D / 32);
  const int64_t total = (int64_t)__builtin_popcountll(live) * nch;
  const float* tq = Ts + r * ts_stride + 16 * h;
  uint64_t lm = live, cm = live;   // live tiles still to load / to score
  int cnt = 0;                     // lane m: rows removed into slot m

  int lj = 0;   // load cursor's chunk; loads past the end re-read a valid row of the wave's range
  auto next_load = [&](float (&buf)[16]) {
    const int t = lm ? __builtin_ctzll(lm) : __builtin_ctzll(live);
    const int64_t row = min(r_begin + (int64_t)(wave + NW * t) * 32 + r, N - 1);
    load_chunk<DT>(corpus, row, D, 32 * lj + 16 * h, buf);
    if (++lj == nch) { lj = 0; lm &= lm - 1ull; }
  };
  int cj = 0;   // compute cursor's chunk
  f32x16 acc = f32x16{};
  float ss = 0.f;
  auto finalize = [&]() {
    ss += __shfl_xor(ss, 32, 64);
    if (h == 0) nrm[r] = ss;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    const int t = __builtin_amdgcn_readfirstlane(__builtin_ctzll(cm));
    const int tr0 = (wave + NW * t) * 32;   // tile's first row, relative to r_begin
    const uint32_t vis = (uint32_t)__builtin_amdgcn_readlane((int)word, t);
    uint32_t removed = 0u;
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
      const float ni = nrm[c_row(rg, h)];
      const bool vi = ni > 0.f && __builtin_isfinite(ni);
      const float sim = acc[rg] / (sqrtf(ni) * sj);
      const uint64_t b = __ballot(vi && vj && sim >= theta);   // lanes 0..31: row c_row(rg, 0); 32..63: c_row(rg, 1)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const uint32_t sims = (uint32_t)(b >> (32 * hh));
        const int row = c_row(rg, hh);
        if (sims != 0u && ((vis >> row) & 1u)) {   // wave-uniform
          removed |= 1u << row;
          cnt += lane == __builtin_ctz(sims) ? 1 : 0;
        }
      }
    }
    // rows a hit names (a zero-norm hit removes its own row): lowest slot first
    uint32_t named = (uint32_t)__ballot(own >= tr0 && own < tr0 + 32);
    while (named) {
      const int m = __builtin_ctz(named);
      const int row = __builtin_amdgcn_readlane(own, m) - tr0;
      if (((vis & ~removed) >> row) & 1u) {
        removed |= 1u << row;
        cnt += lane == m ? 1 : 0;
      }
      named &= named - 1u;
    }
    if (lane == 0) mask_out[(r_begin + tr0) >> 5] = vis & ~removed;
    __builtin_amdgcn_wave_barrier();   // the norms are read before the next tile overwrites them
    acc = f32x16{};
    ss = 0.f;
    cm &= cm - 1ull;
    cj = 0;
  };
  auto consume = [&](const float (&buf)[16]) {
    score_chunk(buf, tq + 32 * cj, acc, ss);
    if (++cj == nch) finalize();
  };

  // stream_pass's ring (rank_pass.hpp): three register buffers used in place, loaded two chunks
  // ahead, with hipcc's own counted waits
  if (total > 0) {
    float b0[16], b1[16], b2[16];
    next_load(b0);
    next_load(b1);
    for (int64_t c = 0; c < total; c += 3) {
      next_load(b2);
      consume(b0);
      if (c + 1 >= total) break;
      next_load(b0);
      consume(b1);
      if (c + 2 >= total) break;
      next_load(b1);
      consume(b2);
    }
  }

  if (lane < 32) cnts[wave * 32 + lane] = cnt;
  __syncthreads();
  if (tid < FQ) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += cnts[w * 32 + tid];
    lines[(int64_t)blockIdx.x * FQ + tid] = s;
  }
}

// out_count[m] = the sum of the workgroups' lines; one workgroup, 8 threads per slot
__global__ __launch_bounds__(256) void rank_exclude_sum(const int32_t* __restrict__ lines, int64_t nwg, int H,
                                                        int32_t* __restrict__ out_count) {
  __shared__ int32_t part[8][FQ];
  const int m = threadIdx.x & 31, p = threadIdx.x >> 5;
  int s = 0;
  for (int64_t w = p; w < nwg; w += 8) s += lines[w * FQ + m];
  part[p][m] = s;
  __syncthreads();
  if (p == 0 && m < H) {
#pragma unroll
    for (int i = 1; i < 8; ++i) s += part[i][m];
    out_count[m] = s;
  }
}

}  // namespace

// (the split's workgroups are at most exclude_chunks, which is monotone in N)
size_t rank_exclude_workspace_bytes(int64_t N) { return al128((size_t)exclude_chunks(N) * FQ * sizeof(int32_t)); }

hipError_t rank_exclude(const void* corpus, int64_t N, int64_t D, int dt, const float* hits, const int64_t* hit_index,
                        int H, int64_t base, float theta, const uint32_t* mask_in, uint32_t* mask_out,
                        int32_t* out_count, void* ws, hipStream_t s) {
  if (N < 1 || H < 1 || H > FQ || D < 32 || D % 32 || D > RANK_MAX_D) return hipErrorInvalidValue;
  const RowSplit split = row_split(N, exclude_chunks(N));   // rows <= MAX_ROWS: a multiple of 384 itself
  if (split.rpw > MAX_ROWS || split.nwg > 0x7fffffffll) return hipErrorInvalidValue;
  int32_t* lines = (int32_t*)ws;
  const hipError_t e = dispatch_dt(dt, [&](auto DT) {
    return launch_lds(rank_exclude_kernel<DT()>, dim3((unsigned)split.nwg), 64 * NW, exclude_lds(D), s, corpus, N, D,
                      hits, hit_index, H, base, theta, mask_in, mask_out, split.rpw, lines);
  });
  if (e != hipSuccess || !out_count) return e;
  return launch_kernel(rank_exclude_sum, dim3(1), 256, s, (const int32_t*)lines, split.nwg, H, out_count);
}

}  // namespace miclip
