// Event search (gfx950): the top-k temporal runs of matching frames per query, from the [Q, N]
// score matrix mi_score_matrix wrote, columns in time order (tests/event_ref.py
// states the result as a serial NumPy loop).
//
// Reference call sites this serves: the confidence threshold of the strategies
// (query_strategies.py:121-186, `confidence >= adaptive_threshold`, default 0.5 at app.py:391) and
// their `top_k * 3` over-fetch, which answer with frames and have no notion of time; the time axis
// is the frame number in the file name (query_strategies.py:74).
//
// Semantics (include/miclip.h mi_event_topk):
//   Column t is HOT for query q iff it is visible (row_mask bit set or no mask; inside the query's
//   range clipped to [0, N) or no range) and scores[q][t] >= threshold[q]; the comparison is false
//   for a NaN score or a NaN threshold, threshold = -inf makes every visible non-NaN column hot.
//   time[t] = row_time[t] (non-decreasing, not checked) or t.  Two hot columns a < b with no hot
//   column between them are LINKED iff time[b] - time[a] <= max_gap (cold and invisible columns
//   between them do not matter).  An EVENT is a maximal chain of linked hot columns; its record is
//   begin / end (first / last hot column, inclusive), count (hot columns), peak (largest score,
//   bits copied) and peak_col (lowest column attaining the peak).  It QUALIFIES iff count >=
//   min_count.  The outputs hold the qualifying events by peak descending (score_key's order),
//   then begin ascending; unused slots are -inf / -1 / -1 / -1 / 0; out_total is the number of
//   qualifying events whatever k.
//
// Kernels.  A query's columns are split into blocks of event_block_cols(N) columns (a multiple of
// 256, at most 1024 blocks), one wave per (query, block): Q = 1 uses the chip.  A wave walks its
// block 64 columns a step: one __ballot is the hot word; a hot lane finds its previous hot lane by
// bit operations and that lane's time by a shuffle (the block's carry when the word has none), so
// a second __ballot is the START word (hot, and the previous hot column absent or too far back);
// a segmented max-scan across the lanes (segment heads = starts) gives every run of the word its
// peak and lowest peak column.  What crosses words is a wave-uniform open record.  Two shortcuts
// give the same records: a word with at most SERIAL_HOT hot columns is walked column by column on
// wave-uniform values (the statement itself: the common case under a selective threshold), and a
// word without a start takes one max-reduction in place of the scan.
//   event_walk<false>  per block a summary: first / last hot time, the partial record before its
//                      first start (head), the partial record from its last start on (tail);
//                      within this pass a block's first hot column is not a start.
//   event_scan         one workgroup per query: the exclusive prefix of the summaries under their
//                      associative combine = the open record and last hot time entering each block.
//   event_walk<true>   walks again from the carried state.  An event is closed, complete, by the
//                      wave that sees the next start (or column N): however many blocks it spans,
//                      one wave emits it.  Qualifying events are counted and inserted into the
//                      wave's sorted list, one entry per lane, key = (score_key(peak), ~begin).
//   event_reduce       one workgroup per query merges the blocks' lists (begin is unique per
//                      query, so keys are) and sums the blocks' counts.
// No workgroup waits for another inside a launch: what crosses blocks is carried between launches
// through the workspace.  No atomics, no allocation, no host synchronisation; every array is read
// by the kernels; the totals are integer sums of per-block counts.  All stores are ordinary vector
// stores.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "internal.hpp"
#include "rank_keys.hpp"

namespace miclip {
namespace {
using rankk::al128;
using rankk::score_key;

constexpr int64_t MAX_BLOCKS = 1024;   // blocks of one query
constexpr int64_t STEP_COLS = 256;     // columns loaded per walk iteration: 4 words in flight
constexpr int REDUCE_WAVES = 16;
constexpr int SERIAL_HOT = 6;          // a word with at most this many hot columns is walked column by column
constexpr int SCAN_THREADS = 512;      // event_scan: threads per query, SCAN_PER blocks each
constexpr int SCAN_PER = MAX_BLOCKS / SCAN_THREADS;

// columns of one block at N (a multiple of STEP_COLS): 256 until N passes 1024 blocks of them
int64_t block_cols(int64_t N) {
  const int64_t per = (N + MAX_BLOCKS - 1) / MAX_BLOCKS;
  const int64_t bc = (per + STEP_COLS - 1) / STEP_COLS * STEP_COLS;
  return bc > STEP_COLS ? bc : STEP_COLS;
}
int64_t block_count(int64_t N) { return (N + block_cols(N) - 1) / block_cols(N); }
// an upper bound of block_count that is monotone in N (block_count itself drops when block_cols steps up)
int64_t block_bound(int64_t N) {
  const int64_t b = (N + STEP_COLS - 1) / STEP_COLS;
  return b < MAX_BLOCKS ? b : MAX_BLOCKS;
}

// a (partial) event; count 0 = none
struct Rec {
  int32_t begin, end, count, pcol;
  uint32_t pkey, pbits;   // score_key of the peak (> 0 for every hot score) and its bits
};
// a block's (or a range of blocks') summary.  split: the range holds a start; then head is the
// partial record before the first start and tail the one from the last start on; else head is all
// of its hot columns
struct BlockSum {
  int64_t first_time, last_time;
  Rec head, tail;
  int32_t any, split;
};
// what enters a block: the open record (count 0: none) and the time of the last hot column
struct Carry {
  int64_t last_time;
  Rec rec;
  int32_t open, pad;
};

// a (left) absorbs b (right, not empty); the left peak wins ties: the lowest column
__host__ __device__ inline void extend(Rec& a, const Rec& b) {
  if (a.count == 0) {
    a = b;
    return;
  }
  a.end = b.end;
  a.count += b.count;
  if (b.pkey > a.pkey) {
    a.pkey = b.pkey;
    a.pcol = b.pcol;
    a.pbits = b.pbits;
  }
}

__device__ __forceinline__ void store_rec(Rec* o, const Rec& r) {
  o->begin = r.begin, o->end = r.end, o->count = r.count, o->pcol = r.pcol, o->pkey = r.pkey, o->pbits = r.pbits;
}

__host__ __device__ inline bool far_apart(int64_t later, int64_t earlier, uint64_t gap) {
  return (uint64_t)later - (uint64_t)earlier > gap;   // later >= earlier: exact as unsigned
}

// the summary of range A followed by range B (associative; any = 0 is the identity)
__host__ __device__ inline BlockSum combine(const BlockSum& A, const BlockSum& B, uint64_t gap) {
  if (!B.any) return A;
  if (!A.any) return B;
  BlockSum R = A;
  R.last_time = B.last_time;
  if (!far_apart(B.first_time, A.last_time, gap)) {   // B's head continues A's open record
    if (!A.split) {
      extend(R.head, B.head);
      R.split = B.split;
      R.tail = B.tail;
    } else if (B.split) {
      R.tail = B.tail;
    } else {
      extend(R.tail, B.head);
    }
  } else {   // B's first hot column is a start
    R.split = 1;
    R.tail = B.split ? B.tail : B.head;
  }
  return R;
}

__device__ __forceinline__ int rl(int v, int l) {
  return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(l));
}
__device__ __forceinline__ uint64_t rl64(uint64_t v, int l) {
  return ((uint64_t)(uint32_t)rl((int)(v >> 32), l) << 32) | (uint32_t)rl((int)v, l);
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int l) {
  return ((uint64_t)(uint32_t)__shfl((int)(v >> 32), l, 64) << 32) | (uint32_t)__shfl((int)v, l, 64);
}
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d) {
  return ((uint64_t)(uint32_t)__shfl_up((int)(v >> 32), d, 64) << 32) | (uint32_t)__shfl_up((int)v, d, 64);
}
__device__ __forceinline__ uint64_t low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }   // bits 0 .. n-1

__device__ __forceinline__ uint64_t event_key(uint32_t pkey, int32_t begin) {
  return ((uint64_t)pkey << 32) | (0xFFFFFFFFu - (uint32_t)begin);   // larger is better; 0: empty
}

__device__ __forceinline__ int shfl_up_pay(int v) { return __shfl_up(v, 1, 64); }
__device__ __forceinline__ int4 shfl_up_pay(int4 v) {
  return make_int4(__shfl_up(v.x, 1, 64), __shfl_up(v.y, 1, 64), __shfl_up(v.z, 1, 64), __shfl_up(v.w, 1, 64));
}
__device__ __forceinline__ int rl_pay(int v, int l) { return rl(v, l); }
__device__ __forceinline__ int4 rl_pay(int4 v, int l) { return make_int4(rl(v.x, l), rl(v.y, l), rl(v.z, l), rl(v.w, l)); }

// a wave's sorted list: lane i holds the i-th best entry so far (key 0: none) and its payload P
template <class P>
struct WaveList {
  uint64_t key = 0;
  P pay = {};
  uint64_t kth = 0;   // wave-uniform: the key of entry k - 1

  __device__ __forceinline__ void insert(int lane, int k, uint64_t nk, P np) {   // nk, np are wave-uniform
    if (nk <= kth) return;
    const int pos = __builtin_popcountll(__ballot(key > nk));
    const uint64_t uk = shfl_up64(key, 1);
    const P up = shfl_up_pay(pay);
    if (lane > pos) {
      key = uk, pay = up;
    } else if (lane == pos) {
      key = nk, pay = np;
    }
    kth = rl64(key, k - 1);
  }

  // one candidate per lane (key 0: none): those that can still enter the list, in lane order
  __device__ __forceinline__ void merge(int lane, int k, uint64_t ck, P cp) {
    uint64_t m = __ballot(ck > kth);
    while (m) {
      const int e = __builtin_ctzll(m);
      insert(lane, k, rl64(ck, e), rl_pay(cp, e));
      m &= m - 1ull;
    }
  }
};

template <bool EMIT>
__global__ __launch_bounds__(64) void event_walk(const float* __restrict__ scores, int64_t N, int64_t Q,
                                                 const float* __restrict__ threshold,
                                                 const int64_t* __restrict__ row_time,
                                                 const uint32_t* __restrict__ row_mask,
                                                 const int64_t* __restrict__ query_range, uint64_t gap, int min_count,
                                                 int k, int64_t bc, int64_t nblk, BlockSum* __restrict__ sums,
                                                 const Carry* __restrict__ carries, uint64_t* __restrict__ ckey,
                                                 int4* __restrict__ cpay, int32_t* __restrict__ ccnt) {
  const int lane = threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x % Q, b = (int64_t)blockIdx.x / Q;
  const float tau = threshold[q];
  int64_t lo = 0, hi = N;
  if (query_range) {
    lo = max(query_range[2 * q], (int64_t)0);
    hi = min(query_range[2 * q + 1], N);
  }
  const int64_t cb = b * bc, ce = min(N, cb + bc);
  const float* srow = scores + q * N;
  const uint64_t lt = low_bits(lane), le = low_bits(lane + 1);

  // wave-uniform state
  bool open = false, split = false;
  int64_t first_time = 0, last_time = 0;
  Rec rec = {}, head = {};
  int nqual = 0;
  WaveList<int4> list;   // payload: end, count, peak column, peak bits
  if (EMIT) {
    const Carry c = carries[q * nblk + b];
    open = c.open != 0;
    last_time = c.last_time;
    rec = c.rec;
  }
  auto emit = [&](const Rec& r) {
    if (r.count < min_count) return;
    ++nqual;
    list.insert(lane, k, event_key(r.pkey, r.begin), make_int4(r.end, r.count, r.pcol, (int)r.pbits));
  };
  // a start was seen: the open record r is complete (EMIT), or is the block's head if it is the first
  auto close = [&](const Rec& r) {
    if (EMIT) {
      emit(r);
    } else if (!split) {
      head = r;
      split = true;
    }
  };

  auto word = [&](int64_t c0, float s, int64_t t, bool hot) {
    const uint64_t H = __ballot(hot);
    if (H == 0ull) return;
    const int cbase = (int)c0;
    const uint32_t key = score_key(s, 0), bits = __float_as_uint(s);
    if (__builtin_popcountll(H) <= SERIAL_HOT) {
      // few hot columns: the statement itself, column by column, on wave-uniform values
      uint64_t m = H;
      while (m) {
        const int l = __builtin_ctzll(m);
        m &= m - 1ull;
        const int64_t tl = row_time ? (int64_t)rl64((uint64_t)t, l) : c0 + l;
        const Rec one = {cbase + l, cbase + l, 1, cbase + l, (uint32_t)rl((int)key, l), (uint32_t)rl((int)bits, l)};
        if (!EMIT && !open) first_time = tl;
        if (open && far_apart(tl, last_time, gap)) {
          close(rec);
          rec = one;
        } else {
          extend(rec, one);   // (not open: rec is empty)
        }
        open = true;
        last_time = tl;
      }
      return;
    }
    // the previous hot column: in the word, else the carried one
    const uint64_t below = H & lt;
    const int pl = below ? 63 - __builtin_clzll(below) : -1;
    int64_t pt = row_time ? (int64_t)shfl64((uint64_t)t, pl < 0 ? 0 : pl) : c0 + pl;
    const bool hasp = pl >= 0 || open;
    if (pl < 0) pt = last_time;
    const bool start = hot && (hasp ? far_apart(t, pt, gap) : EMIT);
    const uint64_t S = __ballot(start);
    const int top = 63 - __builtin_clzll(H);
    if (!EMIT && !open) first_time = (int64_t)rl64((uint64_t)t, __builtin_ctzll(H));
    if (S == 0ull) {
      // no start: the word's hot columns all continue the open record; one max-reduction of the keys
      uint32_t mk = hot ? key : 0u;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) mk = max(mk, (uint32_t)__shfl_xor((int)mk, d, 64));
      const int pl0 = __builtin_ctzll(__ballot(hot && key == mk));   // the lowest column attaining it
      const Rec seg = {cbase + __builtin_ctzll(H), cbase + top, __builtin_popcountll(H), cbase + pl0, mk,
                       (uint32_t)rl((int)bits, pl0)};
      extend(rec, seg);
      open = true;
      last_time = (int64_t)rl64((uint64_t)t, top);
      return;
    }
    // segmented max-scan of (key, lowest lane) over the lanes, segment heads = starts
    uint64_t comp = hot ? ((((uint64_t)key << 6) | (uint64_t)(63 - lane)) + 1ull) : 0ull;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t o = shfl_up64(comp, d);
      const bool ok = lane >= d && ((S >> ((lane - d + 1) & 63)) & low_bits(d)) == 0ull;
      if (ok && o > comp) comp = o;
    }
    // a run's last hot lane holds the run: its start (-1: it continues the open record), count, peak
    const uint64_t sm = S & le;
    const int ss = sm ? 63 - __builtin_clzll(sm) : -1;
    const int cnt = __builtin_popcountll(H & le & ~low_bits(ss < 0 ? 0 : ss));
    const uint64_t c1 = comp - 1ull;
    const uint32_t pkey = (uint32_t)(c1 >> 6);
    const int plane = 63 - (int)(c1 & 63ull);
    const uint32_t pbits = (uint32_t)__shfl((int)bits, plane & 63, 64);

    // the hot columns before the word's first start continue the open record, which ends there
    const uint64_t headmask = H & low_bits(__builtin_ctzll(S));
    if (headmask) {
      const int he = 63 - __builtin_clzll(headmask);
      const Rec seg = {cbase + __builtin_ctzll(headmask), cbase + he, rl(cnt, he), cbase + rl(plane, he),
                       (uint32_t)rl((int)pkey, he), (uint32_t)rl((int)pbits, he)};
      extend(rec, seg);
      open = true;
    }
    if (open) close(rec);
    if (EMIT) {   // the runs between two starts of the word end here too
      const uint64_t above = H & ~le;
      const int nh = above ? __builtin_ctzll(above) : 64;
      const bool closing = hot && nh < 64 && ((S >> nh) & 1ull) && ss >= 0 && cnt >= min_count;
      const uint64_t ekey = event_key(pkey, cbase + ss);
      nqual += __builtin_popcountll(__ballot(closing));
      uint64_t m = __ballot(closing && ekey > list.kth);
      while (m) {
        const int e = __builtin_ctzll(m);
        list.insert(lane, k, rl64(ekey, e), make_int4(cbase + e, rl(cnt, e), cbase + rl(plane, e), rl((int)pbits, e)));
        m &= m - 1ull;
      }
    }
    // the run from the last start on is the open record now
    rec = Rec{cbase + (63 - __builtin_clzll(S)), cbase + top, rl(cnt, top), cbase + rl(plane, top),
              (uint32_t)rl((int)pkey, top), (uint32_t)rl((int)pbits, top)};
    open = true;
    last_time = (int64_t)rl64((uint64_t)t, top);
  };

  for (int64_t c0 = cb; c0 < ce; c0 += STEP_COLS) {
    if (c0 >= hi || c0 + STEP_COLS <= lo) continue;   // wave-uniform: nothing visible here
    float sv[4];
    int64_t tv[4];
    bool vis[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t col = c0 + 64 * u + lane;
      bool ok = col < ce && col >= lo && col < hi;
      if (ok && row_mask) ok = (row_mask[col >> 5] >> (col & 31)) & 1u;
      vis[u] = ok;
      sv[u] = ok ? srow[col] : 0.f;
      tv[u] = ok && row_time ? row_time[col] : col;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) word(c0 + 64 * u, sv[u], tv[u], vis[u] && sv[u] >= tau);
  }

  const int64_t slot = q * nblk + b;
  if (EMIT) {
    if (b == nblk - 1 && open) emit(rec);   // column N closes the last event
    if (lane < k) {
      ckey[slot * k + lane] = list.key;
      cpay[slot * k + lane] = list.pay;
    }
    if (lane == 0) ccnt[slot] = nqual;
  } else if (lane == 0) {
    BlockSum* o = sums + slot;   // field by field: a struct temporary would live in scratch
    o->first_time = first_time;
    o->last_time = last_time;
    if (!split) {
      head = rec;
      rec = Rec{};
    }
    store_rec(&o->head, head);
    store_rec(&o->tail, rec);
    o->any = open;
    o->split = split;
  }
}

__device__ __forceinline__ BlockSum shfl_up_sum(const BlockSum& v, int d) {
  constexpr int W = sizeof(BlockSum) / 4;
  union {
    BlockSum s;
    int w[W];
  } a, r;
  a.s = v;
#pragma unroll
  for (int i = 0; i < W; ++i) r.w[i] = __shfl_up(a.w[i], d, 64);
  return r.s;
}

// carries[q][b] = the state after blocks 0 .. b-1 of query q.  One workgroup per query: a thread
// folds its SCAN_PER blocks (loaded together), each wave scans its 64 folds with shuffles (six
// combine steps; one thread doing 64 in a row is a 30 us dependent chain), a thread prefixes the
// earlier waves' sums and walks its blocks again
__global__ __launch_bounds__(SCAN_THREADS) void event_scan(const BlockSum* __restrict__ sums, int64_t nblk,
                                                           uint64_t gap, Carry* __restrict__ carries) {
  constexpr int NWV = SCAN_THREADS / 64;
  __shared__ BlockSum wsum[NWV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const BlockSum* qs = sums + (int64_t)blockIdx.x * nblk;
  Carry* qc = carries + (int64_t)blockIdx.x * nblk;
  const int64_t b0 = (int64_t)tid * SCAN_PER;
  BlockSum v[SCAN_PER];
#pragma unroll
  for (int j = 0; j < SCAN_PER; ++j) v[j] = b0 + j < nblk ? qs[b0 + j] : BlockSum{};
  BlockSum a = v[0];
#pragma unroll
  for (int j = 1; j < SCAN_PER; ++j) a = combine(a, v[j], gap);
  // inclusive scan of the wave's 64 folds by shuffles, then the earlier waves' sums through LDS
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const BlockSum o = shfl_up_sum(a, d);
    if (lane >= d) a = combine(o, a, gap);
  }
  if (lane == 63) wsum[wave] = a;
  BlockSum p = shfl_up_sum(a, 1);   // exclusive within the wave
  if (lane == 0) p = BlockSum{};
  __syncthreads();
  BlockSum e = {};
  for (int w = 0; w < wave; ++w) e = combine(e, wsum[w], gap);
  p = combine(e, p, gap);
#pragma unroll
  for (int j = 0; j < SCAN_PER; ++j) {
    if (b0 + j >= nblk) break;
    Carry* c = qc + b0 + j;
    c->last_time = p.last_time;
    store_rec(&c->rec, p.any ? (p.split ? p.tail : p.head) : Rec{});
    c->open = p.any;
    c->pad = 0;
    p = combine(p, v[j], gap);
  }
}

// the query's top-k of its blocks' lists and the sum of their counts; nblk = 0 writes the empty
// slots and a zero total
__global__ __launch_bounds__(64 * REDUCE_WAVES) void event_reduce(
    const uint64_t* __restrict__ ckey, const int4* __restrict__ cpay, const int32_t* __restrict__ ccnt, int64_t nblk,
    int k, int64_t index_base, float* __restrict__ out_score, int64_t* __restrict__ out_peak,
    int64_t* __restrict__ out_begin, int64_t* __restrict__ out_end, int32_t* __restrict__ out_count,
    int32_t* __restrict__ out_total) {
  __shared__ uint64_t skey[REDUCE_WAVES][64];
  __shared__ int32_t ssrc[REDUCE_WAVES][64];
  __shared__ int32_t part[REDUCE_WAVES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t q = blockIdx.x, n = nblk * k;   // n <= 65536
  const uint64_t* keys = ckey + q * n;
  WaveList<int> list;   // payload: the candidate's number
  for (int64_t i0 = (int64_t)wave * 256; i0 < n; i0 += 256 * REDUCE_WAVES) {
    uint64_t kv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = i0 + 64 * u + lane;
      kv[u] = i < n ? keys[i] : 0ull;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) list.merge(lane, k, kv[u], (int)(i0 + 64 * u + lane));
  }
  skey[wave][lane] = list.key;
  ssrc[wave][lane] = list.pay;
  // the total: a fixed-order integer sum
  int32_t c = 0;
  for (int64_t i = tid; i < nblk; i += 64 * REDUCE_WAVES) c += ccnt[q * nblk + i];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
  if (lane == 0) part[wave] = c;
  __syncthreads();
  if (wave != 0) return;
  for (int w = 1; w < REDUCE_WAVES; ++w) list.merge(lane, k, skey[w][lane], ssrc[w][lane]);
  if (lane < k) {
    const bool used = list.key != 0ull;
    const int4 p = used ? cpay[q * n + list.pay] : make_int4(0, 0, 0, 0);   // end, count, peak column, peak bits
    const int64_t o = q * k + lane;
    const int64_t begin = (int64_t)(0xFFFFFFFFu - (uint32_t)list.key);
    out_score[o] = used ? __uint_as_float((uint32_t)p.w) : -INFINITY;
    out_peak[o] = used ? index_base + p.z : (int64_t)-1;
    out_begin[o] = used ? index_base + begin : (int64_t)-1;
    out_end[o] = used ? index_base + p.x : (int64_t)-1;
    out_count[o] = used ? p.y : 0;
  }
  if (lane == 0) {
    int32_t t = 0;
#pragma unroll
    for (int w = 0; w < REDUCE_WAVES; ++w) t += part[w];
    out_total[q] = t;
  }
}

struct Workspace {
  BlockSum* sums;
  Carry* carries;
  int32_t* ccnt;
  uint64_t* ckey;
  int4* cpay;
  size_t bytes;
};
Workspace carve(void* ws, int64_t slots, int k) {
  Workspace w;
  char* p = (char*)ws;
  size_t o = 0;
  w.sums = (BlockSum*)(p + o), o += al128((size_t)slots * sizeof(BlockSum));
  w.carries = (Carry*)(p + o), o += al128((size_t)slots * sizeof(Carry));
  w.ccnt = (int32_t*)(p + o), o += al128((size_t)slots * sizeof(int32_t));
  w.ckey = (uint64_t*)(p + o), o += al128((size_t)slots * k * sizeof(uint64_t));
  w.cpay = (int4*)(p + o), o += al128((size_t)slots * k * sizeof(int4));
  w.bytes = o;
  return w;
}

}  // namespace

int64_t event_block_cols(int64_t N) { return block_cols(N > 0 ? N : 1); }

size_t event_workspace_bytes(int64_t N, int64_t Q, int k) {
  return carve(nullptr, (Q > 0 ? Q : 1) * (block_bound(N) > 0 ? block_bound(N) : 1), k).bytes;
}

bool event_sizes_ok(int64_t N, int64_t Q) { return N < ((int64_t)1 << 31) && Q * block_bound(N) < ((int64_t)1 << 31); }

hipError_t event_topk(const float* scores, int64_t N, int64_t Q, const float* threshold, const int64_t* row_time,
                      const uint32_t* row_mask, const int64_t* query_range, int64_t max_gap, int min_count, int k,
                      int64_t index_base, float* out_score, int64_t* out_peak, int64_t* out_begin, int64_t* out_end,
                      int32_t* out_count, int32_t* out_total, void* ws, hipStream_t s) {
  if (Q < 1 || N < 0 || k < 1 || k > 64 || max_gap < 0 || min_count < 1 || !event_sizes_ok(N, Q))
    return hipErrorInvalidValue;
  const int64_t nblk = N > 0 ? block_count(N) : 0, bc = block_cols(N > 0 ? N : 1);
  const Workspace w = carve(ws, Q * nblk, k);
  if (nblk > 0) {
    const dim3 grid((unsigned)(Q * nblk));
    hipError_t e = launch_kernel(event_walk<false>, grid, 64, s, scores, N, Q, threshold, row_time, row_mask,
                                 query_range, (uint64_t)max_gap, min_count, k, bc, nblk, w.sums,
                                 (const Carry*)w.carries, w.ckey, w.cpay, w.ccnt);
    if (e != hipSuccess) return e;
    e = launch_kernel(event_scan, dim3((unsigned)Q), SCAN_THREADS, s, (const BlockSum*)w.sums, nblk, (uint64_t)max_gap,
                      w.carries);
    if (e != hipSuccess) return e;
    e = launch_kernel(event_walk<true>, grid, 64, s, scores, N, Q, threshold, row_time, row_mask, query_range,
                      (uint64_t)max_gap, min_count, k, bc, nblk, w.sums, (const Carry*)w.carries, w.ckey, w.cpay,
                      w.ccnt);
    if (e != hipSuccess) return e;
  }
  return launch_kernel(event_reduce, dim3((unsigned)Q), 64 * REDUCE_WAVES, s, (const uint64_t*)w.ckey,
                       (const int4*)w.cpay, (const int32_t*)w.ccnt, nblk, k, index_base, out_score, out_peak,
                       out_begin, out_end, out_count, out_total);
}

}  // namespace miclip

// introspection (not in miclip.h): the columns one workgroup covers at N, for tests that place
// events on workgroup boundaries
extern "C" int64_t mi_debug_event_block_cols(int64_t N) { return miclip::event_block_cols(N); }
