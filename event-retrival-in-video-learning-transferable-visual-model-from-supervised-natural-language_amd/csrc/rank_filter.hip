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
// Shared with the unfiltered pass: everything that scores a row or keeps a list.  The kernels
// here are rank_pass.hpp's stream_pass (k <= 16: rank_stream's body) and tiles_pass (k <= 64:
// rank_stage1's body) run under the FilteredRows policy below where rank.hip runs them under
// AllRows, so a visible row's score is bit for bit the one mi_rank_topk / mi_score_matrix give
// that row.  This file holds only what the filter adds: the entry scan, the policy, the two
// kernel wrappers with their early exit, and the launcher.
//
// Work skipping: a workgroup's row range is a multiple of 32 rows, so a wave's 32-row tile is one
// mask word.  A tile is live for a query block iff its word (rows < N) is non-zero and it
// intersects the hull [lo, hi) of the block's 32 query ranges.  At entry lane t of a wave decides
// tile t of that wave (at most 64: the launcher bounds the rows per workgroup) and keeps the
// tile's word; the ballot is the wave's live-tile bitmap.  Dead tiles are neither loaded nor
// scored: the load cursor and the compute cursor both walk the bitmap's set bits.  A workgroup
// without a live tile writes its empty candidate slots and exits before the queries are staged.
//
// Both kernels emit rank_stage1's candidate format, [Q][nwg * k] scores and int64 indices
// (-1 = empty), which rank_merge reduces.
#include <hip/hip_runtime.h>

#include <climits>

#include "common.hpp"
#include "internal.hpp"
#include "rank_pass.hpp"

namespace miclip {
namespace {
using namespace rankk;

constexpr int RQ = FQ;            // queries per workgroup (MFMA N)
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

// The row policy (rank_pass.hpp) over a FilterView: both cursors walk the set bits of `live`.
struct FilteredRows {
  const FilterView fv;
  bool qvalid;
  int h;             // lane >> 5
  uint64_t lm, cm;   // live tiles still to load / to score
  __device__ __forceinline__ FilteredRows(const FilterView& v, bool qv, int hh)
      : fv(v), qvalid(qv), h(hh), lm(v.live), cm(v.live) {}
  __device__ __forceinline__ int tiles() const { return __builtin_popcountll(fv.live); }
  __device__ __forceinline__ int load_tile() const { return lm ? __builtin_ctzll(lm) : 0; }
  __device__ __forceinline__ void load_next() { lm &= lm - 1ull; }
  __device__ __forceinline__ int tile() const { return __builtin_amdgcn_readfirstlane(__builtin_ctzll(cm)); }
  __device__ __forceinline__ void next() { cm &= cm - 1ull; }
  // this lane's 16 rows of the tile are c_row(rg, h) = 4 h + c_row(rg, 0): their visibility bits
  // shifted to fixed positions
  __device__ __forceinline__ uint32_t rows(int t, int tr0) const {
    return tile_visible((uint32_t)__builtin_amdgcn_readlane((int)fv.word, t), fv.qlo, fv.qhi, tr0, qvalid) >> (4 * h);
  }
  __device__ __forceinline__ bool sees(uint32_t vis, int rg, int) const {   // (visible rows are < nrows)
    return (vis & (1u << c_row(rg, 0))) != 0u;
  }
};

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

  const bool qvalid = q0 + r < Q;
  FilteredRows rows(fv, qvalid, h);
  const int64_t row_base = index_base + r_begin;
  stream_pass<DT, NW>(corpus, N, D, Ts, ts_stride, nrm_all + wave * 32, tau, wave, lane, r_begin, qvalid, k, norm_mode,
                      nan_first, rows, [&](uint64_t (&L)[KC]) {
    // the workgroup's top-k per query (lines_publish's wave tree), written in rank_stage1's
    // candidate format
    if (workgroup_merge16<NW>(L, smem, wave, lane) && qvalid) {
      float* os = ws_s + (q0 + r) * C + (int64_t)RB * k;
      int64_t* oi = ws_i + (q0 + r) * C + (int64_t)RB * k;
#pragma unroll
      for (int p = 0; p < 16; ++p) {
        if (p < k) {
          const uint64_t e = L[p];
          os[p] = e ? decode_key((uint32_t)(e >> 32), nan_first) : -INFINITY;
          oi[p] = e ? row_base + (int64_t)(uint32_t)~(uint32_t)e : (int64_t)-1;
        }
      }
    }
  });
}

// k <= 64.  LDS: queries [32][D+4] f32, per-wave norms [4][32]; the lists [256 lanes][KC]
// (key u32, idx i32) reuse the query area after a barrier.
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

  tiles_pass<KC, DT>(corpus, N, D, smem, Ts, ts_stride, nrm_all + wave * 32, wave, r_begin, q0, Q, k, norm_mode,
                     nan_first, index_base, FilteredRows(fv, q0 + (lane & 31) < Q, lane >> 5), ws_s, ws_i, C);
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

hipError_t rank_topk_filtered(const void* corpus, int64_t N, int64_t D, int dt, const float* q, int64_t Q, int k,
                              int64_t base, int norm_mode, int nan_first, const uint32_t* row_mask,
                              const int64_t* query_range, float* out_s, int64_t* out_i, void* ws, hipStream_t s) {
  if (k < 1 || k > RANK_REG_K || N < 1 || Q < 1 || N > rank_filtered_max_rows(k)) return hipErrorInvalidValue;
  const RowSplit split = row_split(N, filter_chunks(N, k));   // rows <= the cap: a multiple of 384 itself
  const int64_t rpw = split.rpw, nwg = split.nwg;               // nwg <= filter_chunks
  const int64_t C = nwg * k;
  float* ws_s = (float*)ws;
  int64_t* ws_i = (int64_t*)((char*)ws + lists_scores_bytes(N, Q, k));
  const dim3 grid((unsigned)((Q + RQ - 1) / RQ), (unsigned)nwg);   // (query blocks, row blocks): RB / QB
  const hipError_t e = dispatch_dt(dt, [&](auto DT) {
    auto pass = [&](auto fn, int nt, size_t lds) {
      return launch_lds(fn, grid, nt, lds, s, corpus, N, D, q, Q, k, rpw, norm_mode, nan_first, base, row_mask,
                        query_range, ws_s, ws_i, C);
    };
    // (the stream's tail: the waves' merged lists [NW][32][16] u64)
    return k <= 16 ? pass(rank_filter_stream<DT(), STREAM_NW>, 64 * STREAM_NW,
                          stream_lds(D, STREAM_NW, (size_t)STREAM_NW * 32 * 16 * 8))
                   : pass(rank_filter_tiles<64, DT()>, 256, stage1_lds(D, 64));
  });
  if (e != hipSuccess) return e;
  return rank_merge(ws_s, ws_i, Q, C, k, nan_first, out_s, out_i, s);
}

}  // namespace miclip
