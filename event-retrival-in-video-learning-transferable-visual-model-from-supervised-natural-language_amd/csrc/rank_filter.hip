// Filtered ranking (gfx950): the fused normalise + cosine + top-k pass of rank.hip over the rows
// a request may see, given as a row bitmask and / or a per-query row range; indices stay global.
//
// Reference call sites this serves:
//   the UI's video filter, whose default is "all videos"          Backend/app.py:402-429, 567-588, 605
//       (one resident library of videos, a row range per video / per query: miclip/library.py)
//   the hybrid strategies' "CLIP top_k*3, then intersect with the frames a keyword / object
//       filter allows"                                  query_strategies.py:253-361, 466-599, 601-775
//       (exact form: top-k among the allowed frames, the row mask)
//
// Visibility: row r is visible to query q iff (row_mask == NULL or bit r & 31 of word r >> 5 is
// set) and begin_q <= r < end_q, ranges clipped to [0, N).  Only visible rows enter a list, raise
// a threshold or are returned (a hidden NaN row under MI_NAN_FIRST included).
//
// Arithmetic: rank_stream's / rank_stage1's (the k-ordered v_mfma_f32_32x32x2_f32 chain, the fmaf
// sum of squares, inv_norm, score_key), so a visible row's score is bit for bit the one
// mi_rank_topk / mi_score_matrix give that row.
//
// Work skipping: a workgroup's row range is a multiple of 32 rows, so a wave's 32-row tile is one
// mask word.  A tile is live for a query block iff its word (rows < N) is non-zero and it
// intersects the hull [lo, hi) of the block's 32 query ranges.  At entry lane t of a wave decides
// tile t of that wave (at most 64: the launcher bounds the rows per workgroup) and keeps the
// tile's word; the ballot is the wave's live-tile bitmap.  Dead tiles are neither loaded nor
// scored: the load cursor and the compute cursor both walk the bitmap's set bits.  A workgroup
// without a live tile writes its empty candidate slots and exits before the queries are staged.
//
// k <= 16 (rank_filter_stream): rank_stream's three-buffer chunk stream (hipcc's own counted
// waits), packed-u64 register lists and tau; k <= 64 (rank_filter_tiles): rank_stage1<64>'s
// tile-at-a-time loop and (key, index) lists.  Both emit rank_stage1's candidate format,
// [Q][nwg * k] scores and int64 indices (-1 = empty), which rank_merge reduces.
#include <hip/hip_runtime.h>

#include <climits>

#include "common.hpp"
#include "internal.hpp"
#include "rank_keys.hpp"

namespace miclip {
namespace {
using namespace rankk;

constexpr int RQ = 32;            // queries per workgroup (MFMA N)
constexpr int MAX_WAVE_TILES = 64;   // one live bit per tile of a wave

// What a wave knows about its tiles and its lane's query after the entry scan.
struct FilterView {
  uint64_t live;     // bit t: tile t of this wave is live for the query block (wave-uniform)
  uint32_t word;     // lane t: tile t's mask word, rows >= N cleared (all ones without a mask)
  int qlo, qhi;      // this lane's query range relative to the workgroup's first row, in [0, nrows]
};

// r_begin % 32 == 0; tile t of wave `wave` starts at r_begin + (wave + NW * t) * 32
template <int NW>
__device__ __forceinline__ FilterView filter_scan(const uint32_t* __restrict__ row_mask,
                                                  const int64_t* __restrict__ query_range, int64_t N, int64_t Q,
                                                  int64_t q0, int64_t r_begin, int64_t r_end, int wave, int lane) {
  FilterView v;
  // the lane's query range, clipped; empty (or no query) -> [N, 0), which leaves the hull alone
  const int64_t q = q0 + (lane & 31);
  int64_t b = N, e = 0;
  if (q < Q) {
    b = query_range ? query_range[2 * q] : 0;
    e = query_range ? query_range[2 * q + 1] : N;
    b = b < 0 ? 0 : b;
    e = e > N ? N : e;
    if (b >= e) { b = N; e = 0; }
  }
  int64_t lo = b, hi = e;
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1) {
    const int64_t ol = __shfl_xor(lo, o, 64), oh = __shfl_xor(hi, o, 64);
    lo = ol < lo ? ol : lo;
    hi = oh > hi ? oh : hi;
  }
  const int64_t nrows = r_end - r_begin;
  const int64_t rb = b - r_begin, re = e - r_begin;
  v.qlo = (int)(rb < 0 ? 0 : (rb > nrows ? nrows : rb));
  v.qhi = (int)(re < 0 ? 0 : (re > nrows ? nrows : re));
  const int64_t ntw = (nrows + 31) / 32;
  const int my_tiles = ntw > wave ? (int)((ntw - 1 - wave) / NW + 1) : 0;   // <= MAX_WAVE_TILES
  uint32_t w = 0u;
  bool alive = false;
  if (lane < my_tiles) {
    const int64_t row0 = r_begin + (int64_t)(wave + NW * lane) * 32;   // < r_end <= N
    const int64_t left = N - row0;
    w = row_mask ? row_mask[row0 >> 5] : 0xFFFFFFFFu;
    if (left < 32) w &= (1u << (int)left) - 1u;
    alive = w != 0u && row0 < hi && row0 + 32 > lo;
  }
  v.word = w;
  v.live = __ballot(alive);
  return v;
}

// The 32 rows of the tile starting at tr0 (relative to the workgroup's first row) that this lane's
// query may see: the tile's mask word cut to the query's range, one bit per row.
__device__ __forceinline__ uint32_t tile_visible(uint32_t word, int qlo, int qhi, int tr0, bool qvalid) {
  const int lo = min(max(qlo - tr0, 0), 32), hi = min(max(qhi - tr0, 0), 32);
  const uint32_t below_hi = (uint32_t)((1ull << hi) - 1ull), below_lo = (uint32_t)((1ull << lo) - 1ull);
  return qvalid && hi > lo ? word & below_hi & ~below_lo : 0u;
}

// this workgroup holds no candidate for its query block: k empty slots per query
__device__ __forceinline__ void write_empty(int64_t q0, int64_t Q, int k, int64_t C, float* __restrict__ ws_s,
                                            int64_t* __restrict__ ws_i) {
  const int tid = threadIdx.x;
  if (tid < RQ && q0 + tid < Q) {
    float* os = ws_s + (q0 + tid) * C + (int64_t)RB * k;
    int64_t* oi = ws_i + (q0 + tid) * C + (int64_t)RB * k;
    for (int o = 0; o < k; ++o) {
      os[o] = -INFINITY;
      oi[o] = -1;
    }
  }
}

__device__ __forceinline__ void stage_queries(float* Ts, int ts_stride, const float* __restrict__ queries, int64_t D,
                                              int64_t q0, int64_t Q, int NT) {
  for (int64_t e = threadIdx.x; e < RQ * D; e += NT) {
    const int qq = (int)(e / D);
    const int64_t d = e % D;
    Ts[qq * ts_stride + d] = (q0 + qq < Q) ? queries[(q0 + qq) * D + d] : 0.f;
  }
}

// k <= 16.  LDS: queries [32][D+4] f32, row norms [NW][32], tau [32]; the waves' merged lists
// [NW][32][16] u64 reuse the query area after a barrier.
template <int DT, int NW>
__global__ __launch_bounds__(64 * NW) void rank_filter_stream(
    const void* __restrict__ corpus, int64_t N, int64_t D, const float* __restrict__ queries, int64_t Q, int k,
    int64_t rows_per_wg, int norm_mode, int nan_first, int64_t index_base, const uint32_t* __restrict__ row_mask,
    const int64_t* __restrict__ query_range, float* __restrict__ ws_s, int64_t* __restrict__ ws_i, int64_t C) {
  constexpr int NT = 64 * NW, KC = 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ts_stride = (int)D + 4;
  float* Ts = (float*)smem;
  float* nrm_all = Ts + RQ * ts_stride;
  uint32_t* tau = (uint32_t*)(nrm_all + NW * 32);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int64_t q0 = (int64_t)QB * RQ;
  const int64_t r_begin = (int64_t)RB * rows_per_wg;
  const int64_t r_end = min(N, r_begin + rows_per_wg);

  const FilterView fv = filter_scan<NW>(row_mask, query_range, N, Q, q0, r_begin, r_end, wave, lane);
  if (!__syncthreads_or(fv.live != 0ull)) {   // no live tile in the workgroup: nothing staged
    write_empty(q0, Q, k, C, ws_s, ws_i);
    return;
  }
  stage_queries(Ts, ts_stride, queries, D, q0, Q, NT);
  if (tid < RQ) tau[tid] = 0u;
  __syncthreads();

  float* nrm = nrm_all + wave * 32;
  const int nch = (int)(D / 32);
  const int64_t total = (int64_t)__builtin_popcountll(fv.live) * nch;

  uint64_t L[KC];
#pragma unroll
  for (int p = 0; p < KC; ++p) L[p] = 0ull;      // (key 0, row ~0): below every real candidate
  const bool qvalid = q0 + r < Q;
  const float* tq = Ts + r * ts_stride + 16 * h;

  // load cursor: the live tiles still to load, chunk; loads past the end re-read a valid row
  uint64_t lm = fv.live;
  int lj = 0;
  auto next_load = [&](float (&buf)[16]) {
    const int t = lm ? __builtin_ctzll(lm) : 0;
    const int64_t row = min(r_begin + (int64_t)(wave + NW * t) * 32 + r, N - 1);
    load_chunk<DT>(corpus, row, D, 32 * lj + 16 * h, buf);
    if (++lj == nch) { lj = 0; lm &= lm - 1ull; }
  };
  uint64_t cm = fv.live;   // compute cursor: the same sequence of live tiles
  int cj = 0;
  f32x16 acc = f32x16{};
  float ss = 0.f;
  auto finalize = [&]() {
    ss += __shfl_xor(ss, 32, 64);
    if (h == 0) nrm[r] = inv_norm(ss, norm_mode);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    const int t = __builtin_amdgcn_readfirstlane(__builtin_ctzll(cm));
    const int tr0 = (wave + NW * t) * 32;            // tile's first row, relative to r_begin
    // this lane's 16 rows are rr = 4 h + (rg & 3) + 8 (rg >> 2): their visibility bits at fixed positions
    const uint32_t vis = tile_visible((uint32_t)__builtin_amdgcn_readlane((int)fv.word, t), fv.qlo, fv.qhi, tr0,
                                      qvalid) >> (4 * h);
    const uint32_t tq_thr = tau[r];
    const uint32_t own = (uint32_t)(L[KC - 1] >> 32);
    const uint32_t thr = own > tq_thr ? own : tq_thr;
    uint64_t c[16];
    bool any = false;
    uint32_t okm = 0u;
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
      const int rr = (rg & 3) + 8 * (rg >> 2) + 4 * h;
      const int lr = tr0 + rr;
      const float sc = norm_mode == 2 ? acc[rg] : acc[rg] * nrm[rr];
      const uint32_t key = score_key(sc, nan_first);
      const bool ok = (vis & (1u << ((rg & 3) + 8 * (rg >> 2)))) != 0u && key >= thr;   // (visible rows are < nrows)
      c[rg] = ok ? (((uint64_t)key << 32) | (uint32_t)~(uint32_t)lr) : 0ull;
      any |= ok;
      okm |= ok ? 1u << rg : 0u;
    }
    if (__any(any)) {
      list_update16(L, c, okm);
      // publish this list's k-th key (a lower bound of the query's k-th best visible row)
      uint32_t kth = (uint32_t)(L[0] >> 32);
#pragma unroll
      for (int p = 1; p < KC; ++p) kth = (p == k - 1) ? (uint32_t)(L[p] >> 32) : kth;
      const uint32_t other = (uint32_t)__shfl_xor((int)kth, 32, 64);
      kth = kth > other ? kth : other;
      if (h == 0 && qvalid && kth > tq_thr) tau_max(&tau[r], kth);
    }
    __builtin_amdgcn_wave_barrier();
    acc = f32x16{};
    ss = 0.f;
    cm &= cm - 1ull;
    cj = 0;
  };
  auto consume = [&](const float (&buf)[16]) {
    float tb[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 t = *(const float4*)(tq + 32 * cj + 4 * i);
      tb[4 * i] = t.x; tb[4 * i + 1] = t.y; tb[4 * i + 2] = t.z; tb[4 * i + 3] = t.w;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(buf[i], tb[i], acc, 0, 0, 0);
      ss = fmaf(buf[i], buf[i], ss);
    }
    if (++cj == nch) finalize();
  };

  // rank_stream's ring: three register buffers used in place, loaded two chunks ahead
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

  // the workgroup's top-k per query: the wave's two half-lists by shuffles, then wave 0 folds the
  // other waves' lists from LDS (lines_publish's tree), written in rank_stage1's candidate format
  merge16_xor(L, 32);
  uint64_t* wl = (uint64_t*)smem;  // [NW][32][16]
  __syncthreads();                 // query area free -> lists
  if (wave > 0 && lane < 32) {
#pragma unroll
    for (int p = 0; p < 16; ++p) wl[((wave * 32) + r) * 16 + p] = L[p];
  }
  __syncthreads();
  if (wave == 0 && lane < 32) {
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      uint64_t c[16];
#pragma unroll
      for (int p = 0; p < 16; ++p) c[p] = wl[((w * 32) + r) * 16 + p];
      merge16_desc(L, c);
    }
    if (qvalid) {
      float* os = ws_s + (q0 + r) * C + (int64_t)RB * k;
      int64_t* oi = ws_i + (q0 + r) * C + (int64_t)RB * k;
#pragma unroll
      for (int p = 0; p < 16; ++p) {
        if (p < k) {
          const uint64_t e = L[p];
          os[p] = e ? decode_key((uint32_t)(e >> 32), nan_first) : -INFINITY;
          oi[p] = e ? index_base + r_begin + (int64_t)(uint32_t)~(uint32_t)e : (int64_t)-1;
        }
      }
    }
  }
}

// k <= 64: rank_stage1<64>'s loop over the wave's live tiles.  LDS: queries [32][D+4] f32, per-wave
// norms [4][32]; the lists [256 lanes][KC] (key u32, idx i32) reuse the query area after a barrier.
template <int KC, int DT>
__global__ __launch_bounds__(256) void rank_filter_tiles(
    const void* __restrict__ corpus, int64_t N, int64_t D, const float* __restrict__ queries, int64_t Q, int k,
    int64_t rows_per_wg, int norm_mode, int nan_first, int64_t index_base, const uint32_t* __restrict__ row_mask,
    const int64_t* __restrict__ query_range, float* __restrict__ ws_s, int64_t* __restrict__ ws_i, int64_t C) {
  constexpr int NW = 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ts_stride = (int)D + 4;
  float* Ts = (float*)smem;
  float* nrm_all = Ts + RQ * ts_stride;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t q0 = (int64_t)QB * RQ;
  const int64_t r_begin = (int64_t)RB * rows_per_wg;
  const int64_t r_end = min(N, r_begin + rows_per_wg);

  const FilterView fv = filter_scan<NW>(row_mask, query_range, N, Q, q0, r_begin, r_end, wave, lane);
  if (!__syncthreads_or(fv.live != 0ull)) {
    write_empty(q0, Q, k, C, ws_s, ws_i);
    return;
  }
  stage_queries(Ts, ts_stride, queries, D, q0, Q, 256);
  __syncthreads();

  float* nrm = nrm_all + wave * 32;
  uint32_t lk[KC];
  int32_t li[KC];
#pragma unroll
  for (int p = 0; p < KC; ++p) { lk[p] = 0u; li[p] = INT_MAX; }

  const int qcol = lane & 31, h = lane >> 5;
  const bool qvalid = q0 + qcol < Q;
  for (uint64_t m = fv.live; m != 0ull; m &= m - 1ull) {
    const int t = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
    const int tr0 = (wave + NW * t) * 32;
    const uint32_t vis = tile_visible((uint32_t)__builtin_amdgcn_readlane((int)fv.word, t), fv.qlo, fv.qhi, tr0,
                                      qvalid) >> (4 * h);
    f32x16 acc;
    // (rank.hip's score_tile: one tile, its chunks prefetched one ahead)
    {
      const int64_t row = min(r_begin + tr0 + qcol, N - 1);
      acc = f32x16{};
      float ss = 0.f;
      float cur[16], nxt[16];
      load_chunk<DT>(corpus, row, D, 16 * h, cur);
      const int nch = (int)(D / 32);
      const float* tq = Ts + qcol * ts_stride + 16 * h;
      for (int j = 0; j < nch; ++j) {
        if (j + 1 < nch) load_chunk<DT>(corpus, row, D, 32 * (j + 1) + 16 * h, nxt);
        float tb[16];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float4 tv = *(const float4*)(tq + 32 * j + 4 * i);
          tb[4 * i] = tv.x; tb[4 * i + 1] = tv.y; tb[4 * i + 2] = tv.z; tb[4 * i + 3] = tv.w;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[i], tb[i], acc, 0, 0, 0);
          ss = fmaf(cur[i], cur[i], ss);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) cur[i] = nxt[i];
      }
      ss += __shfl_xor(ss, 32, 64);
      if (h == 0) nrm[qcol] = ss;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
      const int rr = (rg & 3) + 8 * (rg >> 2) + 4 * h;
      const int32_t li_row = tr0 + rr;
      const float sc = apply_norm(acc[rg], nrm[rr], norm_mode);
      const uint32_t key = score_key(sc, nan_first);
      const bool ok = (vis & (1u << ((rg & 3) + 8 * (rg >> 2)))) != 0u && better(key, li_row, lk[KC - 1], li[KC - 1]);
      if (__builtin_expect(__any(ok), 0)) {
        if (ok) list_insert<KC, int32_t>(lk, li, key, li_row);
      }
    }
    __builtin_amdgcn_wave_barrier();   // the norms are read before the next tile overwrites them
  }
  __syncthreads();  // query area free -> lists
  uint32_t* Lk = (uint32_t*)smem;
  int32_t* Li = (int32_t*)(smem + 256 * KC * 4);
#pragma unroll
  for (int p = 0; p < KC; ++p) {
    Lk[tid * KC + p] = lk[p];
    Li[tid * KC + p] = li[p];
  }
  __syncthreads();
  if (tid < RQ && q0 + tid < Q) {
    // 8 sorted lists: lanes {w*64 + tid, w*64 + 32 + tid}
    int pos[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) pos[l] = 0;
    float* os = ws_s + (q0 + tid) * C + (int64_t)RB * k;
    int64_t* oi = ws_i + (q0 + tid) * C + (int64_t)RB * k;
    for (int o = 0; o < k; ++o) {
      uint32_t bk = 0u;
      int32_t bi = INT_MAX;
      int bl = 0;
#pragma unroll
      for (int l = 0; l < 8; ++l) {
        const int src = (l >> 1) * 64 + (l & 1) * 32 + tid;
        if (pos[l] < KC) {
          const uint32_t kk = Lk[src * KC + pos[l]];
          const int32_t ii = Li[src * KC + pos[l]];
          if (better(kk, ii, bk, bi)) { bk = kk; bi = ii; bl = l; }
        }
      }
#pragma unroll
      for (int l = 0; l < 8; ++l) pos[l] += (l == bl) ? 1 : 0;
      os[o] = bi == INT_MAX ? -INFINITY : decode_key(bk, nan_first);
      oi[o] = bi == INT_MAX ? (int64_t)-1 : index_base + r_begin + bi;
    }
  }
}

constexpr int STREAM_NW = 12;
// rows per workgroup: multiples of 384 (one tile round of 12 waves, three of 4) with at most
// MAX_WAVE_TILES tiles per wave
constexpr int64_t STREAM_MAX_ROWS = (int64_t)STREAM_NW * MAX_WAVE_TILES * 32;   // 24576 = 64 x 384
constexpr int64_t TILES_MAX_ROWS = 7680;                                        // 20 x 384: 60 tiles per wave
static_assert(STREAM_MAX_ROWS % 384 == 0 && TILES_MAX_ROWS % 384 == 0, "row ranges are multiples of 384");
static_assert(TILES_MAX_ROWS <= (int64_t)4 * MAX_WAVE_TILES * 32, "rank_filter_tiles: one live bit per tile");

// upper bound of the workgroups of a pass (monotone in N): rank.hip's rank_chunks (<= 512, one
// per CU-slot pair) until the rows per workgroup would exceed the live bitmap
int64_t filter_chunks(int64_t N, int k) {
  const int64_t cap = k <= 16 ? STREAM_MAX_ROWS : TILES_MAX_ROWS;
  const int64_t tiles = (N + 383) / 384;
  const int64_t a = tiles < 512 ? tiles : 512;
  const int64_t b = (N + cap - 1) / cap;
  const int64_t m = a > b ? a : b;
  return m > 1 ? m : 1;
}

size_t lists_scores_bytes(int64_t N, int64_t Q, int k) {
  return al128((size_t)(Q * filter_chunks(N, k) * k) * sizeof(float));
}

}  // namespace

// grid.y carries the row blocks
int64_t rank_filtered_max_rows(int k) { return (int64_t)65535 * (k <= 16 ? STREAM_MAX_ROWS : TILES_MAX_ROWS); }

size_t rank_filtered_workspace_bytes(int64_t N, int64_t Q, int k) {
  return lists_scores_bytes(N, Q, k) + al128((size_t)(Q * filter_chunks(N, k) * k) * sizeof(int64_t));
}

template <int DT>
static hipError_t launch_filter_stream(dim3 grid, size_t lds, hipStream_t s, const void* corpus, int64_t N, int64_t D,
                                       const float* q, int64_t Q, int k, int64_t rpw, int nm, int nf, int64_t base,
                                       const uint32_t* mask, const int64_t* range, float* ws_s, int64_t* ws_i,
                                       int64_t C) {
  auto fn = rank_filter_stream<DT, STREAM_NW>;
  hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fn, grid, dim3(64 * STREAM_NW), lds, s, corpus, N, D, q, Q, k, rpw, nm, nf, base, mask, range,
                     ws_s, ws_i, C);
  return hipGetLastError();
}

template <int DT>
static hipError_t launch_filter_tiles(dim3 grid, size_t lds, hipStream_t s, const void* corpus, int64_t N, int64_t D,
                                      const float* q, int64_t Q, int k, int64_t rpw, int nm, int nf, int64_t base,
                                      const uint32_t* mask, const int64_t* range, float* ws_s, int64_t* ws_i,
                                      int64_t C) {
  auto fn = rank_filter_tiles<64, DT>;
  hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fn, grid, dim3(256), lds, s, corpus, N, D, q, Q, k, rpw, nm, nf, base, mask, range, ws_s, ws_i,
                     C);
  return hipGetLastError();
}

hipError_t rank_topk_filtered(const void* corpus, int64_t N, int64_t D, int dt, const float* q, int64_t Q, int k,
                              int64_t base, int norm_mode, int nan_first, const uint32_t* row_mask,
                              const int64_t* query_range, float* out_s, int64_t* out_i, void* ws, hipStream_t s) {
  if (k < 1 || k > RANK_REG_K || N < 1 || Q < 1 || N > rank_filtered_max_rows(k)) return hipErrorInvalidValue;
  const int64_t nch = filter_chunks(N, k);
  const int64_t rpw = ((N + nch - 1) / nch + 383) / 384 * 384;   // <= the cap: a multiple of 384 itself
  const int64_t nwg = (N + rpw - 1) / rpw;                       // <= nch
  const int64_t C = nwg * k;
  float* ws_s = (float*)ws;
  int64_t* ws_i = (int64_t*)((char*)ws + lists_scores_bytes(N, Q, k));
  const dim3 grid((unsigned)((Q + RQ - 1) / RQ), (unsigned)nwg);   // (query blocks, row blocks): RB / QB
  hipError_t e;
  if (k <= 16) {
    const size_t qa = (size_t)RQ * (D + 4) * 4 + (size_t)STREAM_NW * 32 * 4 + RQ * 4;
    const size_t la = (size_t)STREAM_NW * 32 * 16 * 8;
    const size_t lds = qa > la ? qa : la;
    e = dt == 0   ? launch_filter_stream<0>(grid, lds, s, corpus, N, D, q, Q, k, rpw, norm_mode, nan_first, base,
                                            row_mask, query_range, ws_s, ws_i, C)
        : dt == 1 ? launch_filter_stream<1>(grid, lds, s, corpus, N, D, q, Q, k, rpw, norm_mode, nan_first, base,
                                            row_mask, query_range, ws_s, ws_i, C)
                  : launch_filter_stream<2>(grid, lds, s, corpus, N, D, q, Q, k, rpw, norm_mode, nan_first, base,
                                            row_mask, query_range, ws_s, ws_i, C);
  } else {
    const size_t qa = (size_t)RQ * (D + 4) * 4 + 4 * 32 * 4;
    const size_t la = (size_t)256 * 64 * 8;
    const size_t lds = qa > la ? qa : la;
    e = dt == 0   ? launch_filter_tiles<0>(grid, lds, s, corpus, N, D, q, Q, k, rpw, norm_mode, nan_first, base,
                                           row_mask, query_range, ws_s, ws_i, C)
        : dt == 1 ? launch_filter_tiles<1>(grid, lds, s, corpus, N, D, q, Q, k, rpw, norm_mode, nan_first, base,
                                           row_mask, query_range, ws_s, ws_i, C)
                  : launch_filter_tiles<2>(grid, lds, s, corpus, N, D, q, Q, k, rpw, norm_mode, nan_first, base,
                                           row_mask, query_range, ws_s, ws_i, C);
  }
  if (e != hipSuccess) return e;
  return rank_merge(ws_s, ws_i, Q, C, k, nan_first, out_s, out_i, s);
}

}  // namespace miclip
