// Distinct top-k (gfx950): collapse near-duplicate frames among a query's ranked candidates.
//
// Reference call sites this serves: the `top_k * 3` over-fetch that the strategies filter on the
// host (query_strategies.py:55, 253-361); here the rows live in HBM (and a library's f32 and f16
// videos in two buffers), so the collapse runs on the device, after any ranking route, on that
// route's [Q, P] candidate list.
//
// Semantics (tests/collapse_ref.py states them in NumPy):
//   sim(a, b) = dot(a, b) / (|a| |b|) of the STORED rows widened exactly to f32, all three sums in
//   f32; a row whose sum of squares is zero or not finite is similar to nothing; NaN >= theta is
//   false.  Candidates are walked in list order (never re-sorted), empty slots (index -1 or outside
//   both corpora) skipped.  Candidate j joins the accepted hit in the LOWEST slot it is similar to;
//   else, while fewer than k hits are accepted, it becomes the next hit; else it is dropped
//   (slot -1).  The walk runs to the end of the list, so the counts cover the whole pool.
//
// Kernel: one workgroup of four waves per query.
//   gather  the P <= 64 candidate rows, KCH columns at a time, from either corpus (f32 / bf16 /
//           f16 per corpus) into LDS as f32 [64][KCH + 4]; rows past P and empty slots are zero.
//           Whole rows would not fit (64 x 768 f32 = 192 KB), so the Gram matrix is accumulated
//           over the chunks; the next chunk's loads are in flight under the current chunk's MFMAs.
//   Gram    64 x 64 = 2 x 2 tiles of v_mfma_f32_32x32x2_f32, one tile per wave, the accumulators
//           kept over all chunks.  A lane reads four consecutive columns of its row (one
//           ds_read_b128 per operand) and feeds four MFMAs; both operands use the same lane ->
//           column map, so the tile is the exact-f32 fma chain of the rows' products in that order.
//           Row norms are the diagonal.
//   masks   one __ballot per accumulator register is 2 rows x 32 columns of `sim >= theta`;
//           candidate j's conflict set is the 64-bit mask of its row (bit i: similar to i).
//   walk    wave 0 walks the masks with scalar arithmetic: accepted set, slot = rank of the lowest
//           similar accepted candidate in that set.
// Nothing synchronises or allocates; index and score arrays are read by the kernel.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "internal.hpp"

namespace miclip {
namespace {

constexpr int CP = 64;          // candidate rows, padded: two 32-row MFMA tiles
constexpr int KCH = 128;        // columns staged per chunk
constexpr int LSTR = KCH + 4;   // LDS row stride (f32): 16-byte rows, b128 reads spread over the banks
constexpr int NT = 256;
constexpr int ROWS_PER_PASS = NT / (KCH / 4);   // 8: a thread owns one 4-column unit of every 8th row
constexpr int UNITS = CP / ROWS_PER_PASS;       // 8 units per thread per chunk
static_assert(KCH % 8 == 0 && NT % (KCH / 4) == 0 && CP % ROWS_PER_PASS == 0, "chunk geometry");

struct Corpora {   // global index - index_base in [0, n0): first corpus; in [n0, n0 + n1): second
  const char* c0;
  const char* c1;
  int64_t n0, n1;
  int dt0, dt1;
};

__device__ __forceinline__ int elem_bytes(int dt) { return dt == 0 ? 4 : 2; }

// columns col .. col + 3 of the row at p (dt: 0 f32, 1 bf16, 2 f16) as f32
__device__ __forceinline__ float4 load4(const char* p, int dt, int col) {
  if (dt == 0) return *(const float4*)(p + (size_t)col * 4);
  const uint2 w = *(const uint2*)(p + (size_t)col * 2);
  if (dt == 1)
    return make_float4(bf2f((u16)(w.x & 0xffff)), bf2f((u16)(w.x >> 16)), bf2f((u16)(w.y & 0xffff)),
                       bf2f((u16)(w.y >> 16)));
  union { uint2 u; _Float16 h[4]; } cv;
  cv.u = w;
  return make_float4((float)cv.h[0], (float)cv.h[1], (float)cv.h[2], (float)cv.h[3]);
}

__global__ __launch_bounds__(NT) void rank_collapse_kernel(
    Corpora src, int D, int64_t index_base, const float* __restrict__ cand_s, const int64_t* __restrict__ cand_i,
    int P, int k, float theta, float* __restrict__ out_s, int64_t* __restrict__ out_i, int32_t* __restrict__ out_c,
    int32_t* __restrict__ out_slot, uint64_t* __restrict__ ws_mask) {
  __shared__ __attribute__((aligned(16))) float rows[CP * LSTR];
  __shared__ const char* rptr[CP];   // the candidate's row, nullptr = empty slot
  __shared__ int rdt[CP];
  __shared__ float nrm2[CP];
  __shared__ uint32_t cm[CP][2];     // row i: similar columns 0..31 / 32..63
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t q = blockIdx.x;
  const float* qs = cand_s + q * P;
  const int64_t* qi = cand_i + q * P;

  if (tid < CP) {
    const char* p = nullptr;
    int dt = 0;
    if (tid < P) {
      const int64_t idx = qi[tid];
      if (idx >= 0 && idx >= index_base) {
        const uint64_t rel = (uint64_t)idx - (uint64_t)index_base;   // exact: idx >= index_base
        if (rel < (uint64_t)src.n0) {
          dt = src.dt0;
          p = src.c0 + rel * (uint64_t)D * elem_bytes(dt);
        } else if (rel - (uint64_t)src.n0 < (uint64_t)src.n1) {
          dt = src.dt1;
          p = src.c1 + (rel - (uint64_t)src.n0) * (uint64_t)D * elem_bytes(dt);
        }
      }
    }
    rptr[tid] = p;
    rdt[tid] = dt;
  }
  __syncthreads();

  // this thread's units: columns 4 c4 .. 4 c4 + 3 of rows r0, r0 + 8, ...
  const int c4 = tid & (KCH / 4 - 1), r0 = tid / (KCH / 4);
  const char* rp[UNITS];
  int rd[UNITS];
#pragma unroll
  for (int i = 0; i < UNITS; ++i) {
    rp[i] = rptr[r0 + ROWS_PER_PASS * i];
    rd[i] = rdt[r0 + ROWS_PER_PASS * i];
  }
  float4 v[UNITS];
  auto fetch = [&](int c0) {
    const int col = c0 + 4 * c4;
#pragma unroll
    for (int i = 0; i < UNITS; ++i)
      v[i] = rp[i] && col < D ? load4(rp[i], rd[i], col) : make_float4(0.f, 0.f, 0.f, 0.f);
  };

  const int ti = wave >> 1, tj = wave & 1;   // this wave's tile: rows 32 ti.., columns 32 tj..
  const int r = lane & 31, h = lane >> 5;
  const bool tile_live = 32 * ti < P && 32 * tj < P;   // (a dead tile holds zero rows: its sums stay 0)
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;

  fetch(0);
  for (int c0 = 0; c0 < D; c0 += KCH) {
#pragma unroll
    for (int i = 0; i < UNITS; ++i) *(float4*)&rows[(r0 + ROWS_PER_PASS * i) * LSTR + 4 * c4] = v[i];
    __syncthreads();
    if (c0 + KCH < D) fetch(c0 + KCH);
    if (tile_live) {
      const int w = min(KCH, D - c0);   // D % 32 == 0
      const float* pa = &rows[(32 * ti + r) * LSTR + 4 * h];
      const float* pb = &rows[(32 * tj + r) * LSTR + 4 * h];
      for (int kk = 0; kk < w; kk += 8) {
        const float4 a = *(const float4*)(pa + kk), b = *(const float4*)(pb + kk);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // row norms: the diagonal of the diagonal tiles
  if (ti == tj) {
#pragma unroll
    for (int rg = 0; rg < 16; ++rg)
      if (c_row(rg, h) == r) nrm2[32 * ti + r] = acc[rg];
  }
  __syncthreads();

  {
    const float nj = nrm2[32 * tj + r];
    const bool vj = nj > 0.f && __builtin_isfinite(nj);
    const float sj = sqrtf(nj);
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
      const float ni = nrm2[32 * ti + c_row(rg, h)];
      const bool vi = ni > 0.f && __builtin_isfinite(ni);
      const float sim = acc[rg] / (sqrtf(ni) * sj);
      const uint64_t b = __ballot(vi && vj && sim >= theta);   // lanes 0..31: row c_row(rg, 0); 32..63: c_row(rg, 1)
      if (lane == 0) {
        cm[32 * ti + c_row(rg, 0)][tj] = (uint32_t)b;
        cm[32 * ti + c_row(rg, 1)][tj] = (uint32_t)(b >> 32);
      }
    }
  }
  __syncthreads();

  if (wave != 0) return;
  // the walk: lane j owns candidate j (its mask, its slot) and hit slot j (its count)
  const uint64_t m = (uint64_t)cm[lane][0] | (uint64_t)cm[lane][1] << 32;
  const uint32_t mlo = (uint32_t)m, mhi = (uint32_t)(m >> 32);
  const uint64_t present = __ballot(rptr[lane] != nullptr);
  if (lane < P) ws_mask[q * P + lane] = m;
  uint64_t taken = 0ull;   // accepted candidates; the hit in slot s is the s-th set bit
  int ntaken = 0, myslot = -1, cnt = 0;
  for (int j = 0; j < P; ++j) {
    if (!((present >> j) & 1ull)) continue;
    const uint64_t mj = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)mlo, j) |
                        (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)mhi, j) << 32;
    const uint64_t hit = mj & taken;
    int s = -1;
    if (hit) {
      s = __builtin_popcountll(taken & ((1ull << __builtin_ctzll(hit)) - 1ull));
    } else if (ntaken < k) {
      s = ntaken++;
      taken |= 1ull << j;
    }
    if (lane == j) myslot = s;
    if (lane == s) ++cnt;
  }
  if (lane < P) out_slot[q * P + lane] = myslot;
  if (lane < k) {
    out_c[q * k + lane] = cnt;
    if (lane >= ntaken) {
      out_s[q * k + lane] = -INFINITY;
      out_i[q * k + lane] = -1;
    }
  }
  if ((taken >> lane) & 1ull) {   // an accepted candidate: its score bit for bit, its index
    ((uint32_t*)out_s)[q * k + myslot] = ((const uint32_t*)qs)[lane];
    out_i[q * k + myslot] = qi[lane];
  }
}

}  // namespace

size_t rank_collapse_workspace_bytes(int64_t Q, int P) { return ((size_t)Q * (size_t)P * sizeof(uint64_t) + 127) / 128 * 128; }

hipError_t rank_collapse(const void* c0, int64_t n0, int dt0, const void* c1, int64_t n1, int dt1, int64_t D,
                         int64_t base, const float* cand_s, const int64_t* cand_i, int64_t Q, int P, int k,
                         float theta, float* out_s, int64_t* out_i, int32_t* out_c, int32_t* out_slot, void* ws,
                         hipStream_t s) {
  if (P < 1 || P > CP || k < 1 || k > P || Q < 1 || Q > 0x7fffffffll || D < 32 || D % 32 || D > RANK_MAX_D)
    return hipErrorInvalidValue;
  const Corpora src{(const char*)c0, (const char*)c1, n0, c1 ? n1 : 0, dt0, dt1};
  return launch_kernel(rank_collapse_kernel, dim3((unsigned)Q), NT, s, src, (int)D, base, cand_s, cand_i, P, k, theta,
                       out_s, out_i, out_c, out_slot, (uint64_t*)ws);
}

}  // namespace miclip
