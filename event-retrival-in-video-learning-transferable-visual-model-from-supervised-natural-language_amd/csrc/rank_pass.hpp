// The exact-f32 passes over LDS-staged queries, each written once and parameterised by a row
// policy: stream_pass (rank_stream, rank_filter_stream: k <= 16) and tiles_pass (rank_stage1,
// rank_filter_tiles: k <= 64), with the blocks they are made of (query staging, the 32-k chunk,
// score_tile).  A visible row's score is the same instruction sequence under every policy, which
// is what makes filtered and unfiltered results bit-identical.  Host side: the workgroup split of
// the rows and the LDS sizes the launchers of both files share (dispatch_dt / launch_lds: internal.hpp).
//
// A row policy answers, for one wave of a workgroup whose tile t (ordinal) starts at row
// (wave + NW t) * 32 of the workgroup's range:
//   tiles()                     how many tiles the wave scores;
//   load_tile() / load_next()   the tile the load cursor is on (any valid ordinal once past the
//                               end: the ring loads ahead), and its advance;
//   tile() / next()             the same for the compute cursor;
//   rows(t, tr0) / sees(v, rg, lr)   whether this lane's query sees the row of fragment register
//                               rg, row lr of the workgroup's range, in tile t (first row tr0).
// AllRows is below; FilteredRows (a row mask and per-query ranges) is in rank_filter.hip.
#pragma once
#include <type_traits>

#include "rank_keys.hpp"

namespace miclip {
namespace rankk {

constexpr int ROWS_WAVE = 32;   // corpus rows per wave tile (MFMA M)

// Every row of the workgroup's range, for every valid query: tile ordinals 0 .. my_tiles - 1.
struct AllRows {
  int my_tiles, nrows;   // this wave's tiles; rows of the workgroup's range
  bool qvalid;           // this lane's query exists
  int lt = 0, ct = 0;
  __device__ __forceinline__ AllRows(int64_t r_begin, int64_t r_end, int wave, int nw, bool qv) {
    const int64_t ntw = (r_end - r_begin + 31) / 32;
    my_tiles = ntw > wave ? (int)((ntw - 1 - wave) / nw + 1) : 0;
    nrows = (int)(r_end - r_begin);
    qvalid = qv;
  }
  __device__ __forceinline__ int tiles() const { return my_tiles; }
  __device__ __forceinline__ int load_tile() const { return lt; }
  __device__ __forceinline__ void load_next() { ++lt; }
  __device__ __forceinline__ int tile() const { return ct; }
  __device__ __forceinline__ void next() { ++ct; }
  __device__ __forceinline__ int rows(int, int) const { return 0; }
  __device__ __forceinline__ bool sees(int, int, int lr) const { return qvalid && lr < nrows; }
};

// The block's 32 queries into LDS as [32][ts_stride] f32 (zeros past Q); NT threads, then a barrier.
__device__ __forceinline__ void stage_queries(float* Ts, int ts_stride, const float* __restrict__ queries, int64_t D,
                                              int64_t q0, int64_t Q, int NT) {
  for (int64_t e = threadIdx.x; e < FQ * D; e += NT) {
    const int qq = (int)(e / D);
    const int64_t d = e % D;
    Ts[qq * ts_stride + d] = (q0 + qq < Q) ? queries[(q0 + qq) * D + d] : 0.f;
  }
}

// One 32-k chunk of a 32-row x 32-query tile: this lane's 16 row elements a against its query's 16
// (tq: LDS), a k-ordered chain on the exact-f32 MFMA, the row's sum of squares riding along.
__device__ __forceinline__ void score_chunk(const float (&a)[16], const float* tq, f32x16& acc, float& ss) {
  float tb[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 t = *(const float4*)(tq + 4 * i);
    tb[4 * i] = t.x; tb[4 * i + 1] = t.y; tb[4 * i + 2] = t.z; tb[4 * i + 3] = t.w;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], tb[i], acc, 0, 0, 0);
    ss = fmaf(a[i], a[i], ss);
  }
}

// Computes the 32x32 f32 score tile of (rows row0.., queries of this block)
// for one wave.  Returns acc (C layout: col = query = lane&31, row = c_row(r, lane>>5))
// and the per-row sum of squares in nrm (LDS, 32 floats for this wave).
template <int DT>
__device__ __forceinline__ void score_tile(const void* corpus, int64_t N, int64_t D, int64_t row0,
                                           const float* Ts, int ts_stride, float* nrm, f32x16& acc) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int64_t row = min(row0 + r, N - 1);
  acc = f32x16{};
  float ss = 0.f;
  float cur[16], nxt[16];
  load_chunk<DT>(corpus, row, D, 16 * h, cur);
  const int nch = (int)(D / 32);
  const float* tq = Ts + r * ts_stride + 16 * h;
  for (int j = 0; j < nch; ++j) {
    if (j + 1 < nch) load_chunk<DT>(corpus, row, D, 32 * (j + 1) + 16 * h, nxt);
    score_chunk(cur, tq + 32 * j, acc, ss);
#pragma unroll
    for (int i = 0; i < 16; ++i) cur[i] = nxt[i];
  }
  ss += __shfl_xor(ss, 32, 64);
  if (h == 0) nrm[r] = ss;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// The streaming pass of one wave (rank.hip's rank_stream comment): the policy's tiles as one
// stream of 32-k chunks through three register buffers, each finished tile's visible rows
// above the threshold into the lane's sorted packed list L (key << 32 | ~row, row relative to
// r_begin), then tail(L): the kernel's merge of the workgroup's lists.  Ts: the staged queries;
// nrm: this wave's 32 floats; tau: [32] u32, zeroed.
// The list is declared here and handed to the tail, the policy comes by value and wave / lane
// from the kernel: with the list declared in the kernel and passed in by reference hipcc kept it
// as one <16 x i64> vector instead of 16 scalars and spilled 140-190 B per lane.
template <int DT, int NW, class Rows, class Tail>
__device__ __forceinline__ void stream_pass(const void* corpus, int64_t N, int64_t D, const float* Ts, int ts_stride,
                                            float* nrm, uint32_t* tau, int wave, int lane, int64_t r_begin,
                                            bool qvalid, int k, int norm_mode, int nan_first, Rows rows, Tail tail) {
  constexpr int KC = 16;
  uint64_t L[KC];
  const int r = lane & 31, h = lane >> 5;
  const int nch = (int)(D / 32);
  const int64_t total = (int64_t)rows.tiles() * nch;
#pragma unroll
  for (int p = 0; p < KC; ++p) L[p] = 0ull;      // (key 0, row ~0): below every real candidate
  const float* tq = Ts + r * ts_stride + 16 * h;

  int lj = 0;  // load cursor's chunk; loads past the end re-read a valid row
  auto next_load = [&](float (&buf)[16]) {
    const int64_t row = min(r_begin + (int64_t)(wave + NW * rows.load_tile()) * 32 + r, N - 1);
    load_chunk<DT>(corpus, row, D, 32 * lj + 16 * h, buf);
    if (++lj == nch) { lj = 0; rows.load_next(); }
  };
  int cj = 0;  // compute cursor's chunk
  f32x16 acc = f32x16{};
  float ss = 0.f;
  auto finalize = [&]() {
    ss += __shfl_xor(ss, 32, 64);
    if (h == 0) nrm[r] = inv_norm(ss, norm_mode);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    const int t = rows.tile();
    const int tr0 = (wave + NW * t) * 32;           // tile's first row, relative to r_begin
    const auto vis = rows.rows(t, tr0);
    const uint32_t tq_thr = tau[r];
    const uint32_t own = (uint32_t)(L[KC - 1] >> 32);
    const uint32_t thr = own > tq_thr ? own : tq_thr;
    uint64_t c[16];
    bool any = false;
    uint32_t okm = 0u;
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
      const int rr = c_row(rg, h);
      const int lr = tr0 + rr;
      const float sc = norm_mode == 2 ? acc[rg] : acc[rg] * nrm[rr];
      const uint32_t key = score_key(sc, nan_first);
      const bool ok = rows.sees(vis, rg, lr) && key >= thr;
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
    rows.next();
    cj = 0;
  };
  auto consume = [&](const float (&buf)[16]) {
    score_chunk(buf, tq + 32 * cj, acc, ss);
    if (++cj == nch) finalize();
  };

  // Three register buffers used in place, loaded two chunks ahead (hipcc's
  // own counted waits; measured 3.8-4.0 TB/s at 1M rows).  Tried and
  // rejected: a padded exit-free body with sched_barriers (hipcc then drained
  // the ring at the back-edge) and inline-asm loads with hand-counted waits
  // (hipcc copies the in-flight registers).
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
  tail(L);
}

// The tile-at-a-time pass of one workgroup of 4 waves (k <= 64: KC-deep (key, idx) lists that
// would spill in the stream): each wave scores the policy's tiles with score_tile and inserts the
// visible rows candidate by candidate under a wave vote; the workgroup's 8 lists per query then
// merge through LDS (over the query area) into the candidate format, k (score, int64 index) slots
// per (query, workgroup) at ws[q C + RB k], index -1 = empty, which rank_merge reduces.
template <int KC, int DT, class Rows>
__device__ __forceinline__ void tiles_pass(const void* corpus, int64_t N, int64_t D, char* smem,
                                           const float* Ts, int ts_stride, float* nrm, int wave, int64_t r_begin,
                                           int64_t q0, int64_t Q, int k, int norm_mode, int nan_first,
                                           int64_t index_base, Rows rows, float* __restrict__ ws_s,
                                           int64_t* __restrict__ ws_i, int64_t C) {
  constexpr int NW = 4;
  const int tid = threadIdx.x, h = (tid & 63) >> 5;
  uint32_t lk[KC];
  int32_t li[KC];
#pragma unroll
  for (int p = 0; p < KC; ++p) { lk[p] = 0u; li[p] = INT_MAX; }

  for (int n = rows.tiles(); n > 0; --n, rows.next()) {
    const int t = rows.tile();
    const int tr0 = (wave + NW * t) * 32;
    const auto vis = rows.rows(t, tr0);
    f32x16 acc;
    score_tile<DT>(corpus, N, D, r_begin + tr0, Ts, ts_stride, nrm, acc);
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
      const int rr = c_row(rg, h);
      const int32_t li_row = tr0 + rr;
      const float sc = apply_norm(acc[rg], nrm[rr], norm_mode);
      const uint32_t key = score_key(sc, nan_first);
      const bool ok = rows.sees(vis, rg, li_row) && better(key, li_row, lk[KC - 1], li[KC - 1]);
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
  if (tid < FQ && q0 + tid < Q) {
    int pos[2 * NW];
#pragma unroll
    for (int l = 0; l < 2 * NW; ++l) pos[l] = 0;
    float* os = ws_s + (q0 + tid) * C + (int64_t)RB * k;
    int64_t* oi = ws_i + (q0 + tid) * C + (int64_t)RB * k;
    for (int o = 0; o < k; ++o) {
      uint32_t bk;
      int32_t bi;
      lists_pop<2 * NW>(Lk, Li, KC, tid, pos, bk, bi);
      os[o] = bi == INT_MAX ? -INFINITY : decode_key(bk, nan_first);
      oi[o] = bi == INT_MAX ? (int64_t)-1 : index_base + r_begin + bi;
    }
  }
}

// ------------------------------------------------------------ host side
// Rows per workgroup (a multiple of 384: one tile round of 12 waves, three of 4) and workgroups
// of a pass over N rows with at most `chunks` workgroups.
struct RowSplit {
  int64_t rpw, nwg;
};
static inline RowSplit row_split(int64_t N, int64_t chunks) {
  const int64_t rpw = ((N + chunks - 1) / chunks + 383) / 384 * 384;
  return {rpw, (N + rpw - 1) / rpw};
}

// LDS of a stream kernel: queries [32][D+4] f32, row norms [NW][32], tau [32]; its merge tail
// (tail bytes) reuses the area.  Of a stage-1 / tiles kernel: queries, norms [4][32]; the lists
// [256 lanes][KC] (key u32, idx i32) reuse the area.
static inline size_t stream_lds(int64_t D, int NW, size_t tail) {
  const size_t qa = (size_t)FQ * (D + 4) * 4 + (size_t)NW * 32 * 4 + FQ * 4;
  return qa > tail ? qa : tail;
}
static inline size_t stage1_lds(int64_t D, int KC) {
  const size_t qa = (size_t)FQ * (D + 4) * 4 + 4 * 32 * 4;
  const size_t la = (size_t)256 * KC * 8;
  return qa > la ? qa : la;
}

}  // namespace rankk
}  // namespace miclip
