// Multi-head attention core of openai/CLIP's nn.MultiheadAttention
// (softmax(q k^T / sqrt(64)) v per 64-wide head, causal mask for the text
// tower), restated in oracle/clip_ref.py::_mha.  Built with -fno-honor-nans
// (Makefile): the softmax max/sum chains then compile to v_max3 without NaN
// canonicalisation; -inf masking is unaffected.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "common.hpp"
#include "internal.hpp"

namespace miclip {

namespace {

// ------------------------------------------------------- shared device pieces
// (the only copy of each; the kernels below describe where they use them)

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4n __attribute__((ext_vector_type(4)));

// compile-time tile counts handed to the kernels' generic lambdas (bools travel as std::bool_constant)
template <int V>
using Int = std::integral_constant<int, V>;

constexpr float sl2 = 0.125f * 1.4426950408889634f;   // head_dim^-0.5 * log2(e): scores to the log2 domain
constexpr float RESCALE = 8.0f;                       // lazy-rescale threshold (log2 units)

// A query row's max / sum over the lanes that hold it.  16x16 C layout: the row is on lane fr of
// each of the four 16-lane groups -> permlane16 then permlane32 swap; 32x32 layout (P16 = false): on
// lane r of both wave halves -> the permlane32 swap alone.
template <bool P16 = true>
__device__ __forceinline__ float group_max(float v) {
  if (P16) {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  }
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
template <bool P16 = true>
__device__ __forceinline__ float group_sum(float v) {
  if (P16) {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  }
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// Lazy rescale of the online softmax (log2 domain): the running max m only moves, and l and the
// accumulators o are only rescaled, when the chunk max cmu exceeds m by more than 2^RESCALE, so
// P <= 256 and the result is exact after the final 1 / l.  o: f32x4[4] (16x16) or f32x16[2] (32x32).
template <class V, int N>
__device__ __forceinline__ void lazy_rescale(float& m, float& l, V (&o)[N], float cmu) {
  if (cmu > m + RESCALE) {
    const float alpha = __builtin_amdgcn_exp2f(m - cmu);
    l *= alpha;
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] *= alpha;
    m = cmu;
  }
}

// Q fragments (B operand of S^T = K Q^T) of a 16-row query tile for the 16x16x32 MFMA: lane (fr, g)
// holds head dims 32 s + 8 g .. + 7 of row 16 tile + fr, rows past S clamped.  (attention_r32_kernel's
// two loads of a 32-row block stay written out: through a helper its two-phase instantiation changed.)
__device__ __forceinline__ void load_q16(const uint16_t* qb, int64_t ld, int tile, int S, int fr, int g, bf16x8 (&q)[2]) {
  const int qrow = min(tile * 16 + fr, S - 1);
#pragma unroll
  for (int s = 0; s < 2; ++s) q[s] = *(const bf16x8*)(qb + (int64_t)qrow * ld + 32 * s + 8 * g);
}

// ds_read_b64_tr_b16 of the row-major V image, and the V^T A-operand fragment of two of them (the
// second `hi` bytes further on: the next 4-key group of the MFMA's k order)
__device__ __forceinline__ s16x4 tr_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(LDS_AS char*)(uintptr_t)(const LDS_AS char*)p);
}
__device__ __forceinline__ bf16x8 vfrag(const char* p, int hi) {
  const s16x4 lo = tr_read(p);
  const s16x4 up = tr_read(p + hi);
  return __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(lo, up, 0, 1, 2, 3, 4, 5, 6, 7));
}

// Where a (sequence, head)'s output rows go, and in which format: bf16 rows of `out`, or (q8) MX-fp8
// rows of q8 with the head's 64 dims as one 64-k block of out_proj, scale bytes in qs.  The
// accumulators are normalised by inv = 1 / l on the way out.  Built at the call, AttnOut{...}.store16(...):
// kept in a variable that the kernels' lambdas capture by reference, it changed the product kernels'
// code (profiles/attention_isa.log).
struct AttnOut {
  uint16_t* out;
  uint8_t* q8;
  uint8_t* qs;
  int64_t rows_pad;
  int bseq, S, W, h;

  // 16x16 C layout, o[dt][j]: query qrow, head dim dt*16 + 4g + j.  bf16 of one row qrow < S:
  __device__ __forceinline__ void row16_bf16(int qrow, int g, const f32x4 (&o)[4], float inv) const {
    uint16_t* dst = out + ((int64_t)bseq * S + qrow) * W + h * 64 + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      *(uint2*)(dst + dt * 16) = make_uint2(pack_bf16x2(o[dt][0] * inv, o[dt][1] * inv),
                                            pack_bf16x2(o[dt][2] * inv, o[dt][3] * inv));
  }
  // ... in either format, rows >= S dropped (every lane of the wave calls this: the MX block's amax is
  // reduced across the row's four lanes)
  __device__ __forceinline__ void store16(int qrow, int g, const f32x4 (&o)[4], float inv) const {
    if (q8) {
      float amax = 0.f;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int j = 0; j < 4; ++j) amax = fmaxf(amax, fabsf(o[dt][j] * inv));
      amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
      amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
      const int X = mx_block_exp(amax);
      const float scl = ldexpf(1.0f, -X);
      if (qrow < S) {
        const int64_t row = (int64_t)bseq * S + qrow;
        uint8_t* dst = q8 + row * W + h * 64 + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          *(uint32_t*)(dst + dt * 16) = mx_pack4(o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv, scl);
        if (g == 0) qs[mx_scale_index(row, h, rows_pad)] = (uint8_t)(X + 127);
      }
      return;
    }
    if (qrow < S) row16_bf16(qrow, g, o, inv);
  }
};

// --------------------------------------------------------------- attention
// One wave per (sequence, head), head dim 64, whole padded sequence (SP rows,
// multiple of 32) per wave; no workgroup barriers.
//   S = Q K^T : Q (A operand) and K (B operand) fragments are loaded straight
//     from the packed qkv rows as 16-byte pieces (the 16x16x32 operand map
//     wants 8 consecutive head dims of one row per lane), rows past S clamped;
//   softmax over keys in f32 registers (scale 1/8, key >= S and causal masks),
//     rows reduced across the 16 lanes that hold them; P normalised, to bf16,
//     through a per-wave LDS tile (C layout -> operand layout);
//   O^T = V^T P^T with V^T (A operand) from a per-wave transposed LDS image
//     and P (B operand), so each lane holds 4 consecutive head dims of one
//     query row -> one 8-byte store.
// LDS rows are padded to an odd number of 16-byte slots.
template <int SP>
__global__ __launch_bounds__(64) void attention_kernel(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ out,
                                                       int S, int W, int H, int causal, int items) {
  constexpr int TS = SP + 8;  // bf16 per V^T / P row (odd number of 16-byte slots)
  __shared__ __attribute__((aligned(16))) uint16_t lds[64 * TS + 16 * TS];
  uint16_t* Vt = lds;
  uint16_t* Pw = lds + 64 * TS;
  const int item = blockIdx.x;
  if (item >= items) return;
  const int bseq = item / H, h = item % H;
  const int lane = threadIdx.x;
  const int64_t ld = 3 * (int64_t)W;
  const uint16_t* qb = qkv + (int64_t)bseq * S * ld + h * 64;
  const uint16_t* kb = qb + W;
  const uint16_t* vb = qb + 2 * W;

  // V^T image: lane (ch = lane>>3, r8 = lane&7) loads 8 head dims of key
  // row r and scatters them down column r of V^T (consecutive lanes ->
  // consecutive keys, so the 2-byte writes of an instruction are contiguous).
  for (int r0 = 0; r0 < SP; r0 += 8) {
    const int r = r0 + (lane & 7), ch = lane >> 3;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r < S) v = *(const uint4*)(vb + (int64_t)r * ld + ch * 8);
    const uint16_t* vv = (const uint16_t*)&v;
#pragma unroll
    for (int e = 0; e < 8; ++e) Vt[(ch * 8 + e) * TS + r] = vv[e];
  }

  constexpr int NKT = SP / 16;
  const float scale = 0.125f;  // 64 ** -0.5
  const int fr = lane & 15, fk = 8 * (lane >> 4);
  const int nqt = (S + 15) / 16;
  for (int qt = 0; qt < nqt; ++qt) {
    const int64_t qrow = min(qt * 16 + fr, S - 1);
    bf16x8 qa[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) qa[s] = *(const bf16x8*)(qb + qrow * ld + 32 * s + fk);
    f32x4 sc[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      const int64_t krow = min(kt * 16 + fr, S - 1);
      f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 kf = *(const bf16x8*)(kb + krow * ld + 32 * s + fk);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[s], kf, c, 0, 0, 0);
      }
      sc[kt] = c;
    }
    // sc[kt][j]: query row qt*16 + 4*(lane>>4) + j, key kt*16 + (lane&15)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = qt * 16 + 4 * (lane >> 4) + j;
      float m = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        const int key = kt * 16 + fr;
        float v = sc[kt][j] * scale;
        if (key >= S || (causal && key > row)) v = -INFINITY;
        sc[kt][j] = v;
        m = fmaxf(m, v);
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
      float sum = 0.f;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        const float p = __expf(sc[kt][j] - m);
        sc[kt][j] = p;
        sum += p;
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) sum += __shfl_xor(sum, o, 64);
      const float inv = 1.0f / sum;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) Pw[(4 * (lane >> 4) + j) * TS + kt * 16 + fr] = f2bf_hw(sc[kt][j] * inv);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    // O^T[d][q] = sum_key V^T[d][key] P[q][key]
    uint2 ov[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < SP / 32; ++s) {
        const bf16x8 va = *(const bf16x8*)(Vt + (dt * 16 + fr) * TS + 32 * s + fk);
        const bf16x8 pb = *(const bf16x8*)(Pw + fr * TS + 32 * s + fk);
        o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb, o, 0, 0, 0);
      }
      ov[dt] = make_uint2(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]));
    }
    // lane: query row qt*16 + (lane&15), head dims dt*16 + 4*(lane>>4) + 0..3
    const int row = qt * 16 + fr;
    if (row < S) {
      uint16_t* dst = out + ((int64_t)bseq * S + row) * W + h * 64 + 4 * (lane >> 4);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) *(uint2*)(dst + dt * 16) = ov[dt];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  }
}

// ------------------------------------ attention, long sequences, K/V in LDS
// One workgroup of NW waves per (sequence, head); wave w owns the NT query
// tiles w, w + NW, ... (16 rows each) for the whole key sweep, so every 64-key
// chunk of K and V is fetched from HBM/L2 ONCE per (sequence, head) and shared
// by all waves through a two-slot LDS ring (a wave-per-query-tile design
// re-reads K per tile: 37 x the K bytes at 577 tokens, 1.8x slower).  Per chunk:
//   stage   : each thread register-loads 16 B of K and of V of chunk c + 1
//             (issued before chunk c's math, written to the other ring slot
//             after it; one barrier per chunk).  K lands row-major (144-byte
//             rows: the 16 rows of an A-operand read hit disjoint banks), V
//             transposed (V^T rows of 64 keys, 136-byte rows).
//   frags   : the chunk's K (A operand of S^T = K Q^T) and V^T (A operand of
//             O^T = V^T P^T) fragments are read from LDS once per chunk into
//             registers and reused by the wave's NT tiles.
//   softmax : scores in the log2 domain u = s * log2(e)/8 (one FMA per score
//             with the reference max folded in); the running max is only
//             moved (and O, l rescaled) when the chunk max exceeds it by more
//             than 2^8 - lazy rescaling: P <= 256, exact after the final 1/l;
//             row max across the 4 lane groups by permlane16/32 swaps.
// Keys >= S are masked (only in the last chunk, and 16-key tiles past S skip
// their MFMAs; skipping their exponentials too measured 10% slower - the extra
// uniform branches split the softmax block); V^T columns >= S are 0.
// SLOTS = 1: S <= 64 (one chunk; B/32's 50 tokens): a single LDS slot and no
// look-ahead staging, which halves the LDS footprint and frees the staging
// registers, so more workgroups fit per CU for this latency-bound case.
// NW = blockDim / 64 waves (8, or 4 for the single-slot S <= 64 instance);
// PP = 16-byte staging pieces of K (and of V) per thread per chunk (1 for 8
// waves, 2 for 4).
// HP heads per workgroup (A/B: 2 = adjacent heads of one sequence, their 128-byte row segments
// read together as 256 bytes), each on its own NW waves and LDS slots.
// PIPE (S <= 64: NT = 1, SLOTS = 1, HP = 1): persistent workgroups walk items blockIdx.x,
// + gridDim.x, ... and load the next item's Q fragments and K / V pieces into registers before
// computing the current one, so a workgroup always has an item's qkv reads in flight.
// VB (S <= 64 instance): the V^T fragments' eight LDS reads issued together and waited for once
// before the P V MFMAs (hipcc otherwise waits for each read right before its MFMA)
template <int NT, int PP, int SLOTS, int HP = 1, bool PIPE = false, bool VB = false>
__device__ __forceinline__ void attention_flash_body(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ out,
                                                     int S, int W, int H, int causal, uint8_t* __restrict__ q8,
                                                     uint8_t* __restrict__ qs, int64_t rows_pad, int items = 0) {
  static_assert(!PIPE || (NT == 1 && SLOTS == 1 && HP == 1), "PIPE: the single-chunk instance only");
  // ATT_Q0_ONLY: the first 16-query tile only (the last vision block, whose outputs are read at the
  // CLS rows alone, api.cpp last_block_cls); the other tiles' waves still stage K / V
  const bool q0only = causal & ATT_Q0_ONLY;
  causal &= ATT_CAUSAL;
  constexpr int KS = 72, VS = 68;  // LDS row strides (bf16)
  const int NW = PP == 1 ? 8 : (int)(blockDim.x >> 6) / HP;  // PP = 1 is launched with 8 waves
  __shared__ __attribute__((aligned(16))) uint16_t Ksh[HP][SLOTS][64 * KS];
  __shared__ __attribute__((aligned(16))) uint16_t Vsh[HP][SLOTS][64 * VS];
  const int hh = HP == 1 ? 0 : (int)(threadIdx.x >> 6) / NW;   // this thread's head of the workgroup's HP
  uint16_t(*Ks)[64 * KS] = Ksh[hh];
  uint16_t(*Vs)[64 * VS] = Vsh[hh];
  const int tid = threadIdx.x - hh * 64 * NW, lane = tid & 63, wave = tid >> 6;
  const int64_t ld = 3 * (int64_t)W;
  // Staging of one 64-key chunk, in two halves around the previous chunk's math.  First half: this
  // thread's PP 16-byte pieces of K and of V (rows c*64.. of an item's kb_ / vb_; rows >= S: zeros) into
  // the registers kr_ / vr_; second half: the pieces into a ring slot, K row-major, V transposed.
  // These two stay macros, the only ones in the file: as lambdas or as functions, however their
  // operands were passed, every product instantiation of this kernel compiled to other code
  // (profiles/attention_isa.log).
#define FA_STAGE_LOAD(kb_, vb_, c, kr_, vr_)                                              \
  _Pragma("unroll") for (int i = 0; i < PP; ++i) {                                        \
    const int p_ = tid + i * 64 * NW, r_ = (c) * 64 + (p_ >> 3), ch_ = p_ & 7;            \
    kr_[i] = make_uint4(0, 0, 0, 0);                                                      \
    vr_[i] = make_uint4(0, 0, 0, 0);                                                      \
    if ((PP == 1 || p_ < 512) && r_ < S) {                                                \
      kr_[i] = *(const uint4*)((kb_) + (int64_t)r_ * ld + ch_ * 8);                       \
      vr_[i] = *(const uint4*)((vb_) + (int64_t)r_ * ld + ch_ * 8);                       \
    }                                                                                     \
  }
#define FA_STAGE_WRITE(slot)                                                              \
  _Pragma("unroll") for (int i = 0; i < PP; ++i) {                                        \
    const int p_ = tid + i * 64 * NW, r_ = p_ >> 3, ch_ = p_ & 7;                         \
    if (PP == 1 || p_ < 512) {                                                            \
      *(uint4*)(&Ks[slot][r_ * KS + ch_ * 8]) = kr[i];                                    \
      const uint16_t* vv_ = (const uint16_t*)&vr[i];                                      \
      _Pragma("unroll") for (int e = 0; e < 8; ++e) Vs[slot][(ch_ * 8 + e) * VS + r_] = vv_[e]; \
    }                                                                                     \
  }
  int item = blockIdx.x;
  bool first = true;
  uint4 kr_n[PP], vr_n[PP];   // PIPE: the next item's K / V pieces and Q fragments
  bf16x8 qf_n[2];
  for (;;) {
  const int bseq = item / (H / HP), h = (item % (H / HP)) * HP + hh;
  const uint16_t* qb = qkv + (int64_t)bseq * S * ld + h * 64;
  const uint16_t* kb = qb + W;
  const uint16_t* vb = qb + 2 * W;
  const int nch = (S + 63) / 64, nqt = q0only ? 1 : (S + 15) / 16;
  const int fr = lane & 15, g = lane >> 4, fk = 8 * g;

  uint4 kr[PP], vr[PP];
  bf16x8 qf[NT][2];
  float m[NT], l[NT];
  f32x4 o[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    // (load_q16 and, below, lazy_rescale written out: through the helpers the single-tile product
    // kernels <1, 1> and <1, 2, 1> compiled to other code, profiles/attention_isa.log)
    const int qrow = min((wave + NW * t) * 16 + fr, S - 1);
#pragma unroll
    for (int s = 0; s < 2; ++s) qf[t][s] = (!PIPE || first) ? *(const bf16x8*)(qb + (int64_t)qrow * ld + 32 * s + fk) : qf_n[s];
    m[t] = -INFINITY;
    l[t] = 0.f;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if (!PIPE || first) {
    FA_STAGE_LOAD(kb, vb, 0, kr, vr);
  } else {
#pragma unroll
    for (int i = 0; i < PP; ++i) {
      kr[i] = kr_n[i];
      vr[i] = vr_n[i];
    }
  }
  // (PIPE: the previous item's LDS reads ended at the chunk loop's closing barrier)
  FA_STAGE_WRITE(0);
  __syncthreads();
  if (PIPE && item + (int)gridDim.x < items) {   // the next item's operands, in flight during this one
    const int nx = item + (int)gridDim.x;
    const uint16_t* nq = qkv + (int64_t)(nx / H) * S * ld + (nx % H) * 64;
    load_q16(nq, ld, wave, S, fr, g, qf_n);
    FA_STAGE_LOAD(nq + W, nq + 2 * W, 0, kr_n, vr_n);
  }

  for (int c = 0; c < nch; ++c) {
    const int slot = SLOTS == 1 ? 0 : (c & 1);
    if (SLOTS > 1 && c + 1 < nch) FA_STAGE_LOAD(kb, vb, c + 1, kr, vr);
    const int kvalid = min(64, S - c * 64);  // keys of this chunk < S
    bf16x8 kf[4][2], vf[4][2];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int s = 0; s < 2; ++s) kf[kt][s] = *(const bf16x8*)(&Ks[slot][(kt * 16 + fr) * KS + 32 * s + fk]);
    auto read_vf = [&]() {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const uint16_t* vrow = &Vs[slot][(dt * 16 + fr) * VS + 32 * s + 4 * g];
          const uint2 lo = *(const uint2*)vrow;
          const uint2 hi = *(const uint2*)(vrow + 16);
          vf[dt][s] = __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
        }
    };
    // NT > 1: V^T fragments read once per chunk for all tiles; single-tile
    // (S <= 64) instance: read after the softmax, so K and V^T fragments are
    // never live together (fewer VGPRs -> more resident workgroups)
    if (SLOTS > 1) read_vf();
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int qt = wave + NW * t;
      if (qt >= nqt || (causal && c * 64 > qt * 16 + 15)) continue;  // wave-uniform
      const int qrow = qt * 16 + fr;
      f32x4 sc[4];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (kt * 16 < kvalid) {
#pragma unroll
          for (int s = 0; s < 2; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kt][s], qf[t][s], acc, 0, 0, 0);
        }
        sc[kt] = acc;
      }
      // sc[kt][j]: query qrow, key c*64 + kt*16 + 4g + j
      if (kvalid < 64 || (causal && (c + 1) * 64 > qt * 16)) {
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int key = c * 64 + kt * 16 + 4 * g + j;
            if (key >= S || (causal && key > qrow)) sc[kt][j] = -INFINITY;
          }
      }
      float cm = fmaxf(fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3])),
                       fmaxf(fmaxf(sc[1][0], sc[1][1]), fmaxf(sc[1][2], sc[1][3])));
      cm = fmaxf(cm, fmaxf(fmaxf(fmaxf(sc[2][0], sc[2][1]), fmaxf(sc[2][2], sc[2][3])),
                           fmaxf(fmaxf(sc[3][0], sc[3][1]), fmaxf(sc[3][2], sc[3][3]))));
      cm = group_max(cm);
      const float cmu = cm * sl2;  // finite: chunk 0 holds key 0 <= every row
      if (cmu > m[t] + RESCALE) {
        const float alpha = __builtin_amdgcn_exp2f(m[t] - cmu);
        l[t] *= alpha;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[t][dt] *= alpha;
        m[t] = cmu;
      }
      const float mu = m[t];
      float ps[4];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) sc[kt][j] = __builtin_amdgcn_exp2f(fmaf(sc[kt][j], sl2, -mu));
        ps[kt] = (sc[kt][0] + sc[kt][1]) + (sc[kt][2] + sc[kt][3]);
      }
      l[t] += (ps[0] + ps[1]) + (ps[2] + ps[3]);
      if (SLOTS == 1) {
        __builtin_amdgcn_sched_barrier(0);
        read_vf();
        if (VB) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (s == 1 && kvalid <= 32) break;  // keys past round32(S): P = 0, V^T = 0
        bf16x8 pb;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          pb[j] = (__bf16)sc[2 * s][j];
          pb[4 + j] = (__bf16)sc[2 * s + 1][j];
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[t][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[dt][s], pb, o[t][dt], 0, 0, 0);
      }
    }
    if (SLOTS > 1 && c + 1 < nch) FA_STAGE_WRITE(slot ^ 1);
    __syncthreads();
  }
#undef FA_STAGE_LOAD
#undef FA_STAGE_WRITE

#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int qt = wave + NW * t;
    if (qt >= nqt) continue;
    AttnOut{out, q8, qs, rows_pad, bseq, S, W, h}.store16(qt * 16 + fr, g, o[t], 1.0f / group_sum(l[t]));
  }
  if (!PIPE) break;
  item += (int)gridDim.x;
  if (item >= items) break;
  first = false;
  }   // items
}

template <int NT, int PP, int SLOTS = 2>
__global__ __launch_bounds__(512) void attention_flash_kernel(const uint16_t* __restrict__ qkv,
                                                                uint16_t* __restrict__ out, int S, int W, int H,
                                                                int causal, uint8_t* __restrict__ q8,
                                                                uint8_t* __restrict__ qs, int64_t rows_pad) {
  attention_flash_body<NT, PP, SLOTS>(qkv, out, S, W, H, causal, q8, qs, rows_pad);
}

#if MICLIP_AB
// A/B variants of the S <= 64 case (B/32's 50 tokens) on the flash body, whose instance
// attention_flash_kernel<1, 2, 1> on 4 waves was the default before attention_s64_kernel below.  Timed in interleaved rounds at 10k frames (scripts/attn_micro.py,
// profiles/r04_ai_attn_micro.log), all bit-identical: default 603 us; an occupancy target of 6 waves
// per SIMD (72 instead of 74 VGPRs, MICLIP_ATTN_SHORT=3) 604 us; two adjacent heads per 8-wave
// workgroup, their 128-byte qkv / output row segments together (=2) 616 us.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6))) void attention_short_kernel(
    const uint16_t* __restrict__ qkv, uint16_t* __restrict__ out, int S, int W, int H, int causal,
    uint8_t* __restrict__ q8, uint8_t* __restrict__ qs, int64_t rows_pad) {
  attention_flash_body<1, 2, 1>(qkv, out, S, W, H, causal, q8, qs, rows_pad);
}

__global__ __launch_bounds__(256) void attention_pipe_kernel(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ out,
                                                             int S, int W, int H, int causal, uint8_t* __restrict__ q8,
                                                             uint8_t* __restrict__ qs, int64_t rows_pad, int items) {
  attention_flash_body<1, 2, 1, 1, true>(qkv, out, S, W, H, causal, q8, qs, rows_pad, items);
}

__global__ __launch_bounds__(256) void attention_vb_kernel(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ out,
                                                           int S, int W, int H, int causal, uint8_t* __restrict__ q8,
                                                           uint8_t* __restrict__ qs, int64_t rows_pad) {
  attention_flash_body<1, 2, 1, 1, false, true>(qkv, out, S, W, H, causal, q8, qs, rows_pad);
}

__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(6))) void attention_short2_kernel(
    const uint16_t* __restrict__ qkv, uint16_t* __restrict__ out, int S, int W, int H, int causal,
    uint8_t* __restrict__ q8, uint8_t* __restrict__ qs, int64_t rows_pad) {
  attention_flash_body<1, 2, 1, 2>(qkv, out, S, W, H, causal, q8, qs, rows_pad);
}
#endif

// ------------------------------------------ attention, S <= 64, by workgroup shape
// The single-chunk case of attention_flash_body (one (sequence, head) per workgroup, keys 0 .. 63 in
// one LDS slot) with the workgroup's shape as template parameters; every query row's MFMA sequence,
// softmax arithmetic and store conversion are that body's, so all instances are bit-identical to it.
//   NWV  : waves per workgroup, 4 (one 16-query tile each) or 2 (tiles w and w + 2 each: the same
//          waves per CU then belong to twice as many workgroups, each with its own item's loads out);
//   KG   : the K fragments (A operand of S^T = K Q^T) are loaded from the qkv rows as 16-byte
//          pieces, the way Q is, by every wave with a tile (rows >= S clamped: their scores are
//          masked) -- no K image in LDS; otherwise K is staged row-major in 144-byte rows as in
//          the flash body;
//   VTR  : V stays row-major in LDS (one 16-byte store per staged piece, 8-byte unit u of key row r
//          at u ^ (((r >> 1) & 3) << 2): attention_res_kernel's image) and the V^T fragments are
//          read transposed by ds_read_b64_tr_b16; otherwise V is transposed by 2-byte LDS stores
//          as in the flash body.  Either way rows >= S of the image are zeros.
//   CLS  : the last vision block, read at its CLS rows alone (api.cpp last_block_cls): only wave 0
//          loads Q (row 0 on every lane of the tile: a query's result depends on its own Q row
//          alone), runs tile 0 and stores row 0, as row `sequence` of the compact bf16 rows `out`
//          (cls_pitch elements apart); the other waves stage their K / V pieces and leave.
//   ST   : how a tile's 16 output rows are stored (bf16 output; MX-fp8 always as 0).  0: AttnOut's 8 bytes
//          a lane, sixteen 32-byte pieces per store instruction -- measured, these stores and not the
//          loads were the slow part of the kernel (384 us without them, 605 with);
//          1: 16 bytes a lane after an exchange between neighbouring lane groups, 64 contiguous bytes a
//          row; 3: the rows through LDS (the K image, dead once every wave holds its fragments), each
//          store instruction 8 whole 128-byte lines; 4 / 5: 1 / 3 as nontemporal stores; 2: none (A/B
//          timing probe, wrong results).
// LDS per workgroup: 17 920 B with K and transposed V, 8 704 / 8 192 B with V alone.
template <int NWV, bool KG, bool VTR, bool CLS, int ST>
__device__ __forceinline__ void attention_s64_body(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ out, int S,
                                                   int W, int H, int causal, uint8_t* __restrict__ q8,
                                                   uint8_t* __restrict__ qs, int64_t rows_pad, int64_t cls_pitch) {
  static_assert(NWV == 2 || NWV == 4, "attention_s64: the four query tiles over 2 or 4 waves");
  constexpr int NT = 4 / NWV, PP = 8 / NWV;   // tiles per wave; 16-byte staging pieces per thread (512 a chunk)
  constexpr int KS = 72, VS = 68;             // LDS row strides (bf16) of the K image and the transposed V image
  constexpr int KBYTES = KG ? 0 : 64 * KS * 2, VBYTES = VTR ? 64 * 128 : 64 * VS * 2;
  __shared__ __attribute__((aligned(16))) char lds[KBYTES + VBYTES];
  uint16_t* Ks = (uint16_t*)lds;
  char* Vimg = lds + KBYTES;
  uint16_t* Vs = (uint16_t*)Vimg;
  const int item = blockIdx.x;
  const int bseq = item / H, h = item % H;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t ld = 3 * (int64_t)W;
  const uint16_t* qb = qkv + (int64_t)bseq * S * ld + h * 64;
  const uint16_t* kb = qb + W;
  const uint16_t* vb = qb + 2 * W;
  const int nqt = CLS ? 1 : (S + 15) / 16;
  const int fr = lane & 15, g = lane >> 4, fk = 8 * g;
  const int kvalid = S;   // keys of the chunk < S

  // ---- loads: Q fragments of this wave's tiles, K fragments (KG), K / V staging pieces
  bf16x8 qf[NT][2], kf[4][2];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int qt = wave + NWV * t;
    const int qrow = CLS ? 0 : min(qt * 16 + fr, S - 1);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      qf[t][s] = bf16x8{};
      if (qt < nqt) qf[t][s] = *(const bf16x8*)(qb + (int64_t)qrow * ld + 32 * s + fk);
    }
  }
  if (KG) {
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const int krow = min(kt * 16 + fr, S - 1);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        kf[kt][s] = bf16x8{};
        if (wave < nqt && kt * 16 < kvalid) kf[kt][s] = *(const bf16x8*)(kb + (int64_t)krow * ld + 32 * s + fk);
      }
    }
  }
  uint4 kr[PP], vr[PP];
#pragma unroll
  for (int i = 0; i < PP; ++i) {
    const int p = tid + i * 64 * NWV, r = p >> 3, ch = p & 7;
    kr[i] = make_uint4(0, 0, 0, 0);
    vr[i] = make_uint4(0, 0, 0, 0);
    if (r < S) {
      if (!KG) kr[i] = *(const uint4*)(kb + (int64_t)r * ld + ch * 8);
      vr[i] = *(const uint4*)(vb + (int64_t)r * ld + ch * 8);
    }
  }
  // ---- the pieces into the LDS images (PP * 64 * NWV = 512 pieces: key rows 0 .. 63 x 8 chunks)
#pragma unroll
  for (int i = 0; i < PP; ++i) {
    const int p = tid + i * 64 * NWV, r = p >> 3, ch = p & 7;
    if (!KG) *(uint4*)(&Ks[r * KS + ch * 8]) = kr[i];
    if (VTR) {
      *(uint4*)(Vimg + r * 128 + ((ch ^ (((r >> 1) & 3) << 1)) << 4)) = vr[i];
    } else {
      const uint16_t* vv = (const uint16_t*)&vr[i];
#pragma unroll
      for (int e = 0; e < 8; ++e) Vs[(ch * 8 + e) * VS + r] = vv[e];
    }
  }
  __syncthreads();
  constexpr bool STL = ST == 3 || ST == 5;   // output rows staged in LDS (below)
  static_assert(!STL || !KG, "attention_s64: the staged output rows take the K image's place");
  if (!STL && wave >= nqt) return;   // (no barrier below)

  if (!KG) {
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int s = 0; s < 2; ++s) kf[kt][s] = *(const bf16x8*)(&Ks[(kt * 16 + fr) * KS + 32 * s + fk]);
  }
  if (STL) {   // every wave holds its K fragments: the K image's 9216 bytes become 4 x 16 output rows of 144
    __syncthreads();
    if (wave >= nqt) return;
  }
  bf16x8 vf[4][2];
  // transposed reads of the row-major image (attention_res_kernel's lane map): lane (fr, g) gets head
  // dim dt * 16 + fr of keys 32 s + 4 g .. + 3 and 32 s + 16 + 4 g .. + 3, the P V MFMA's k order
  const int vq = fr >> 2, vp = lane & 3, vx = (2 * g + (vq >> 1)) & 3;
  const int rvb = (4 * g + vq) * 128 + vp * 8;
  auto read_vf = [&]() {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (VTR) {
          vf[dt][s] = vfrag(Vimg + 32 * s * 128 + rvb + ((dt ^ vx) << 5), 16 * 128);
        } else {
          const uint16_t* vrow = &Vs[(dt * 16 + fr) * VS + 32 * s + 4 * g];
          const uint2 lo = *(const uint2*)vrow;
          const uint2 hi = *(const uint2*)(vrow + 16);
          vf[dt][s] = __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
        }
      }
  };

#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int qt = wave + NWV * t;
    if (qt >= nqt) continue;  // wave-uniform
    const int qrow = qt * 16 + fr;
    float m = -INFINITY, l = 0.f;
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 sc[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      if (kt * 16 < kvalid) {
#pragma unroll
        for (int s = 0; s < 2; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kt][s], qf[t][s], acc, 0, 0, 0);
      }
      sc[kt] = acc;
    }
    // sc[kt][j]: query qrow, key kt*16 + 4g + j
    if (kvalid < 64 || (causal && 64 > qt * 16)) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int key = kt * 16 + 4 * g + j;
          if (key >= S || (causal && key > qrow)) sc[kt][j] = -INFINITY;
        }
    }
    float cm = fmaxf(fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3])),
                     fmaxf(fmaxf(sc[1][0], sc[1][1]), fmaxf(sc[1][2], sc[1][3])));
    cm = fmaxf(cm, fmaxf(fmaxf(fmaxf(sc[2][0], sc[2][1]), fmaxf(sc[2][2], sc[2][3])),
                         fmaxf(fmaxf(sc[3][0], sc[3][1]), fmaxf(sc[3][2], sc[3][3]))));
    cm = group_max(cm);
    const float cmu = cm * sl2;  // finite: the chunk holds key 0 <= every row
    lazy_rescale(m, l, o, cmu);
    const float mu = m;
    float ps[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
      for (int j = 0; j < 4; ++j) sc[kt][j] = __builtin_amdgcn_exp2f(fmaf(sc[kt][j], sl2, -mu));
      ps[kt] = (sc[kt][0] + sc[kt][1]) + (sc[kt][2] + sc[kt][3]);
    }
    l += (ps[0] + ps[1]) + (ps[2] + ps[3]);
    if (t == 0) {   // after the first softmax: K and V^T fragments are not live together before it
      __builtin_amdgcn_sched_barrier(0);
      read_vf();
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (s == 1 && kvalid <= 32) break;  // keys past round32(S): P = 0, V^T = 0
      bf16x8 pb;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pb[j] = (__bf16)sc[2 * s][j];
        pb[4 + j] = (__bf16)sc[2 * s + 1][j];
      }
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[dt][s], pb, o[dt], 0, 0, 0);
    }
    const float inv = 1.0f / group_sum(l);
    if (CLS) {   // row 0 alone, as row bseq of the compact rows (AttnOut with one cls_pitch-wide row a sequence)
      if (fr == 0) AttnOut{out, nullptr, nullptr, 0, bseq, 1, (int)cls_pitch, h}.row16_bf16(0, g, o, inv);
    } else if (STL && !q8) {
      // whole-line stores: the tile's 16 rows of packed bf16 (row16_bf16's conversion) through this wave's LDS
      // rows (144 bytes apart: the 8-byte writes of a half wave hit disjoint banks), read back as 16-byte
      // pieces, lane L piece L & 7 of row L >> 3 (+ 8), so one store instruction writes 8 rows of 128 bytes
      char* os = lds + wave * (16 * 144);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        *(uint2*)(os + fr * 144 + dt * 32 + g * 8) = make_uint2(pack_bf16x2(o[dt][0] * inv, o[dt][1] * inv),
                                                                pack_bf16x2(o[dt][2] * inv, o[dt][3] * inv));
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int r = p * 8 + (lane >> 3), row = qt * 16 + r;
        const u32x4n v = *(const u32x4n*)(os + r * 144 + (lane & 7) * 16);
        u32x4n* dst = (u32x4n*)(out + ((int64_t)bseq * S + row) * W + h * 64 + (lane & 7) * 8);
        if (row < S) {
          if (ST == 5) __builtin_nontemporal_store(v, dst);
          else *dst = v;
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (NT = 2: the next tile writes these rows again)
      __builtin_amdgcn_wave_barrier();
    } else if ((ST == 1 || ST == 4) && !q8) {
      // 16-byte stores: the row's packed bf16 (row16_bf16's conversion) exchanged between the lane groups g and
      // g ^ 1, so an even group holds dims 16 dt + 4 g .. + 7 of dt = 0 / 2 and an odd one dims 16 dt + 4 (g - 1)
      // .. + 7 of dt = 1 / 3: two stores of 64 contiguous bytes a row instead of four of 32
      uint16_t* dst = out + ((int64_t)bseq * S + qrow) * W + h * 64 + ((g & 1) ? 16 + 4 * (g - 1) : 4 * g);
#pragma unroll
      for (int dp = 0; dp < 2; ++dp) {
        const f32x4 &oa = o[2 * dp], &ob = o[2 * dp + 1];
        const auto x = __builtin_amdgcn_permlane16_swap(pack_bf16x2(oa[0] * inv, oa[1] * inv),
                                                        pack_bf16x2(ob[0] * inv, ob[1] * inv), false, false);
        const auto y = __builtin_amdgcn_permlane16_swap(pack_bf16x2(oa[2] * inv, oa[3] * inv),
                                                        pack_bf16x2(ob[2] * inv, ob[3] * inv), false, false);
        const u32x4n v = {x[0], y[0], x[1], y[1]};
        if (qrow < S) {
          if (ST == 4) __builtin_nontemporal_store(v, (u32x4n*)(dst + 32 * dp));
          else *(u32x4n*)(dst + 32 * dp) = v;
        }
      }
    } else if (ST == 2) {   // timing probe: no output stores (wrong results)
      if (inv == 12345.678f) AttnOut{out, q8, qs, rows_pad, bseq, S, W, h}.store16(qrow, g, o, inv);
    } else {
      AttnOut{out, q8, qs, rows_pad, bseq, S, W, h}.store16(qrow, g, o, inv);
    }
  }
}

template <bool KG, bool VTR, bool CLS, int ST = 0>
__global__ __launch_bounds__(256) void attention_s64_kernel(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ out,
                                                            int S, int W, int H, int causal, uint8_t* __restrict__ q8,
                                                            uint8_t* __restrict__ qs, int64_t rows_pad,
                                                            int64_t cls_pitch) {
  attention_s64_body<4, KG, VTR, CLS, ST>(qkv, out, S, W, H, causal, q8, qs, rows_pad, cls_pitch);
}
// 2 waves x 2 tiles: 4 waves per SIMD asked of the register allocator (a wave's two tiles unrolled side by
// side otherwise take 137 registers: 3 waves per SIMD, 6 workgroups per CU; at 5 per SIMD it spills)
template <bool KG, bool VTR, bool CLS, int ST = 0>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(4))) void attention_s64w2_kernel(
    const uint16_t* __restrict__ qkv, uint16_t* __restrict__ out, int S, int W, int H, int causal,
    uint8_t* __restrict__ q8, uint8_t* __restrict__ qs, int64_t rows_pad, int64_t cls_pitch) {
  attention_s64_body<2, KG, VTR, CLS, ST>(qkv, out, S, W, H, causal, q8, qs, rows_pad, cls_pitch);
}


// ----------------------------- attention, vision towers: K/V resident in LDS
// 64 < S <= 640, non-causal (ViT-L/14 257 tokens, L/14@336 577).  One
// workgroup of NW waves per (sequence, head).  The whole head's K and V
// (rows padded to 32, rows >= S clamped copies: masked / multiplied by P = 0)
// are DMA'd into LDS ONCE (global_load_lds, 8 rows x 128 B per instruction),
// then every wave runs its query tiles (16 rows: w, w + NW, ...) over all keys
// with no further workgroup barrier — a straggler wave no longer parks the
// other seven at a per-chunk barrier, and a second workgroup on the CU
// (S = 257: 72 KB of LDS each) fills the SIMDs meanwhile.
//   K image : 16-byte chunk c of key row r at slot c ^ ((r >> 1) & 7) (the 16
//             rows of a ds_read_b128 A-operand read hit all 16 slots);
//   V image : row-major [key][64 dims], 8-byte unit u at u ^ (((r >> 1) & 3) << 2),
//             read transposed by ds_read_b64_tr_b16 into the V^T A operand of
//             O^T = V^T P^T (a 32-lane half = 8 consecutive keys x 4 units:
//             all 32 8-byte bank pairs once) — no transposing LDS writes;
//   per 64-key chunk: S^T = K Q^T (8 MFMA), online softmax in the log2
//   domain with lazy rescale (flash kernel above), P to bf16, 8 PV MFMAs;
//   the partial last chunk runs only its valid 16-key tiles (NKT template).
// SPLIT (S % 16 small, e.g. L/14's 257 = 16 x 16 + 1): the last, nearly empty query tile
// would add a third tile to wave 0 while the other waves idle with two; instead every wave
// runs it over its share of the 16-key tiles (w, w + NW, ...) and wave 0 merges the partial
// softmax states (m, l, o) of its valid rows through LDS.
template <int NW, bool TT2 = true, bool SPLIT = false, bool SFIRST = false, bool QPF = false>
__global__ __launch_bounds__(NW * 64) void attention_res_kernel(const uint16_t* __restrict__ qkv,
                                                                uint16_t* __restrict__ out, int S, int W, int H,
                                                                uint8_t* __restrict__ q8, uint8_t* __restrict__ qs,
                                                                int64_t rows_pad) {
  extern __shared__ __attribute__((aligned(16))) char res_lds[];
  const int spad = (S + 31) & ~31;
  char* Kimg = res_lds;
  char* Vimg = res_lds + spad * 128;
  const int item = blockIdx.x;
  const int bseq = item / H, h = item % H;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t ld = 3 * (int64_t)W;
  const uint16_t* qb = qkv + (int64_t)bseq * S * ld + h * 64;
  const uint16_t* kb = qb + W;
  const uint16_t* vb = qb + 2 * W;

  // ---- K, V -> LDS (one DMA instruction = 8 rows).  This loop and attention_r32_kernel's differ only
  // in the V swizzle term, and both stay written out: as one shared function either product kernel
  // came out with its loop's address arithmetic compiled differently (profiles/attention_isa.log).
  {
    const int nr8 = spad >> 3;
    const int slot = lane & 7;
    for (int i = wave; i < 2 * nr8; i += NW) {
      const bool isv = i >= nr8;
      const int i8 = isv ? i - nr8 : i;
      const int r = i8 * 8 + (lane >> 3);
      const int c = isv ? (slot ^ (((r >> 1) & 3) << 1)) : (slot ^ ((r >> 1) & 7));
      glds16((isv ? vb : kb) + (int64_t)min(r, S - 1) * ld + c * 8, (isv ? Vimg : Kimg) + i8 * 1024);
    }
  }

  const int nqt = (S + 15) / 16, nch = (S + 63) / 64;
  const int last_kvalid = S - (nch - 1) * 64;   // 1..64
  const int fr = lane & 15, g = lane >> 4;
  const int rk0 = fr * 128 + (((0 + g) ^ (fr >> 1)) << 4);
  const int rk1 = fr * 128 + (((4 + g) ^ (fr >> 1)) << 4);
  const int vq = (lane & 15) >> 2, vp = lane & 3;
  const int vx = (2 * g + (vq >> 1)) & 3;
  const int rvb = (4 * g + vq) * 128 + vp * 8;

  // QPF (A/B): a tile's Q fragments are loaded one tile ahead (the wave's first tile's beside the
  // K/V load), so their latency is not exposed at the head of every tile
  bf16x8 qn[2];
  if (QPF) load_q16(qb, ld, wave, S, fr, g, qn);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // A wave's query tiles are w, w + NW, w + 2 NW, ...; it runs them two at a
  // time (TT = 2): each K / V^T fragment read from LDS feeds both tiles' MFMAs,
  // and one tile's softmax VALU has the other tile's MFMAs beside it (one tile
  // at a time, the QK MFMA -> max -> exp -> PV MFMA chain left the matrix pipe
  // idle behind its own dependencies).  An odd last tile runs alone (TT = 1).
  auto tiles = [&](auto tt_c, int t0, int t1) {
    constexpr int TT = decltype(tt_c)::value;
    const int tq[2] = {t0, t1};
    bf16x8 qf[TT][2];
    if (QPF && TT == 1) {
      qf[0][0] = qn[0];
      qf[0][1] = qn[1];
      if (t0 + NW < (SPLIT ? nqt - 1 : nqt)) load_q16(qb, ld, t0 + NW, S, fr, g, qn);   // the wave's next tile
    } else {
#pragma unroll
      for (int u = 0; u < TT; ++u) load_q16(qb, ld, tq[u], S, fr, g, qf[u]);
    }
    float m[TT], l[TT];
    f32x4 o[TT][4];
#pragma unroll
    for (int u = 0; u < TT; ++u) {
      m[u] = -INFINITY;
      l[u] = 0.f;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[u][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // one 64-key chunk; NKT valid 16-key tiles, MASK: keys >= S inside them
    auto chunk = [&](auto nkt_c, auto mask_c, int c) {
      constexpr int NKT = decltype(nkt_c)::value;
      constexpr bool MASK = decltype(mask_c)::value;
      const char* kc = Kimg + c * 64 * 128;
      f32x4 sc[TT][NKT];
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        const bf16x8 k0 = *(const bf16x8*)(kc + kt * 16 * 128 + rk0);
        const bf16x8 k1 = *(const bf16x8*)(kc + kt * 16 * 128 + rk1);
#pragma unroll
        for (int u = 0; u < TT; ++u) {
          const f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf[u][0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          sc[u][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf[u][1], acc, 0, 0, 0);
        }
      }
      // sc[u][kt][j]: query tq[u]*16 + fr, key c*64 + kt*16 + 4g + j
#pragma unroll
      for (int u = 0; u < TT; ++u) {
        if (MASK) {
#pragma unroll
          for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (c * 64 + kt * 16 + 4 * g + j >= S) sc[u][kt][j] = -INFINITY;
        }
        float cm = fmaxf(fmaxf(sc[u][0][0], sc[u][0][1]), fmaxf(sc[u][0][2], sc[u][0][3]));
#pragma unroll
        for (int kt = 1; kt < NKT; ++kt)
          cm = fmaxf(cm, fmaxf(fmaxf(sc[u][kt][0], sc[u][kt][1]), fmaxf(sc[u][kt][2], sc[u][kt][3])));
        cm = group_max(cm);
        const float cmu = cm * sl2;   // finite: chunk 0 holds key 0 for every row
        lazy_rescale(m[u], l[u], o[u], cmu);
        float ps = 0.f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
          for (int j = 0; j < 4; ++j) sc[u][kt][j] = __builtin_amdgcn_exp2f(fmaf(sc[u][kt][j], sl2, -m[u]));
          ps += (sc[u][kt][0] + sc[u][kt][1]) + (sc[u][kt][2] + sc[u][kt][3]);
        }
        l[u] += ps;
      }
#pragma unroll
      for (int s2 = 0; s2 < (NKT + 1) / 2; ++s2) {
        bf16x8 pb[TT];
#pragma unroll
        for (int u = 0; u < TT; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            pb[u][j] = (__bf16)sc[u][2 * s2][j];
            pb[u][4 + j] = 2 * s2 + 1 < NKT ? (__bf16)sc[u][(2 * s2 + 1) < NKT ? 2 * s2 + 1 : 0][j] : (__bf16)0.f;
          }
        const char* vc = Vimg + (c * 64 + 32 * s2) * 128 + rvb;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const bf16x8 vf = vfrag(vc + ((dt ^ vx) << 5), 16 * 128);
#pragma unroll
          for (int u = 0; u < TT; ++u) o[u][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pb[u], o[u][dt], 0, 0, 0);
        }
      }
    };
    for (int c = 0; c < nch - 1; ++c) chunk(Int<4>{}, std::bool_constant<false>{}, c);
    {
      const int c = nch - 1;
      if (last_kvalid > 48) chunk(Int<4>{}, std::bool_constant<true>{}, c);
      else if (last_kvalid > 32) chunk(Int<3>{}, std::bool_constant<true>{}, c);
      else if (last_kvalid > 16) chunk(Int<2>{}, std::bool_constant<true>{}, c);
      else chunk(Int<1>{}, std::bool_constant<true>{}, c);
    }

#pragma unroll
    for (int u = 0; u < TT; ++u)
      AttnOut{out, q8, qs, rows_pad, bseq, S, W, h}.store16(tq[u] * 16 + fr, g, o[u], 1.0f / group_sum(l[u]));
  };
  // SPLIT: the last tile's rows over this wave's key tiles, partial states to LDS (SFIRST: before the
  // full tiles, so every wave reaches the merge barrier with the same work behind it)
  auto split_part = [&]() __attribute__((always_inline)) {
    // the last query tile (rows 16 (nqt - 1) .. S - 1, vr <= 16 of them) over this wave's
    // 16-key tiles; the same arithmetic as chunk() per key tile (log2-domain online softmax)
    const int tl = nqt - 1, vr = S - 16 * tl;
    const int nkt = (S + 15) / 16;
    bf16x8 qf[2];
    load_q16(qb, ld, tl, S, fr, g, qf);
    float m = -INFINITY, l = 0.f;
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kt = wave; kt < nkt; kt += NW) {
      const int kb = kt * 16;
      const bf16x8 k0 = *(const bf16x8*)(Kimg + kb * 128 + rk0);
      const bf16x8 k1 = *(const bf16x8*)(Kimg + kb * 128 + rk1);
      f32x4 sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf[1], sc, 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (kb + 4 * g + j >= S) sc[j] = -INFINITY;
      const float cm = group_max(fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3])));
      const float cmu = cm * sl2;   // finite: key tile kb < S holds key kb
      lazy_rescale(m, l, o, cmu);
#pragma unroll
      for (int j = 0; j < 4; ++j) sc[j] = __builtin_amdgcn_exp2f(fmaf(sc[j], sl2, -m));
      l += (sc[0] + sc[1]) + (sc[2] + sc[3]);
      bf16x8 pb;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pb[j] = (__bf16)sc[j];
        pb[4 + j] = (__bf16)0.f;
      }
      const char* vc = Vimg + kb * 128 + rvb;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vfrag(vc + ((dt ^ vx) << 5), 16 * 128), pb, o[dt], 0, 0, 0);
    }
    const float lt = group_sum(l);
    // partial states of the valid rows: [wave][row][m, l, o 0..63] after the K / V images
    float* part = (float*)(res_lds + 2 * spad * 128);
    if (fr < vr) {
      float* pw = part + (wave * vr + fr) * 68;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int j = 0; j < 4; ++j) pw[4 + dt * 16 + 4 * g + j] = o[dt][j];
      if (g == 0) {
        pw[0] = m;
        pw[1] = lt;
      }
    }
  };
  if (SPLIT && SFIRST) split_part();
  const int nfull = SPLIT ? nqt - 1 : nqt;   // SPLIT: the last tile is shared out below
  for (int t = wave; t < nfull; t += 2 * NW) {
    if (TT2 && t + NW < nfull) tiles(Int<2>{}, t, t + NW);
    else {
      tiles(Int<1>{}, t, t);
      if (!TT2 && t + NW < nfull) tiles(Int<1>{}, t + NW, t + NW);
    }
  }
  if (SPLIT && !SFIRST) split_part();
  if (SPLIT) {   // (launched with bf16 output only: attention() runs the unsplit kernel when q8 is set)
    const int tl = nqt - 1, vr = S - 16 * tl;
    float* part = (float*)(res_lds + 2 * spad * 128);
    __syncthreads();
    if (wave == 0 && fr < vr) {
      float M = -INFINITY;
#pragma unroll
      for (int w = 0; w < NW; ++w) M = fmaxf(M, part[(w * vr + fr) * 68]);
      float L = 0.f;
      f32x4 O[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) O[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const float* pw = part + (w * vr + fr) * 68;
        const float sw = pw[0] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(pw[0] - M);
        L += pw[1] * sw;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
          for (int j = 0; j < 4; ++j) O[dt][j] += pw[4 + dt * 16 + 4 * g + j] * sw;
      }
      AttnOut{out, q8, qs, rows_pad, bseq, S, W, h}.row16_bf16(tl * 16 + fr, g, O, 1.0f / L);   // (fr < vr: a row < S)
    }
  }
}

// ------------- attention, vision towers: K/V resident in LDS, 32x32x16 MFMAs
// Same work split and LDS residency as attention_res_kernel, on the 32 x 32
// MFMA shape, whose 32 cycles hold the SIMD's issue for 8 (the 16 x 16 shape
// holds 8 of 16), so the softmax VALU of the other wave on the SIMD finds
// twice the issue slots beside the matrix pipe.  Per wave: query blocks of 32
// rows (two at a time, sharing every K / V^T fragment read), 64-key chunks.
//   S^T = K Q^T : K is the A operand (lane: key r, 8 dims of k-step s at
//     chunk 2s + half), Q^T the B operand held in registers for the block;
//     the result X[key][query] has the query on the lane (r = lane & 31) and
//     16 keys per lane half in registers: key (reg & 3) + 8 (reg >> 2) + 4 half;
//   softmax in the log2 domain with the lazy rescale of the kernels above;
//     a row's max over 64 keys is 32 in-lane values and one permlane32 swap;
//   O^T = V^T P^T : X's registers 8s .. 8s + 7, packed to bf16, ARE the B
//     operand of k-step s (the MFMA's k order inside a step is key
//     16s + 8(j >> 2) + 4 half + (j & 3) for element j), so P never leaves the
//     lane; V^T is the A operand, read transposed (ds_read_b64_tr_b16) in that
//     same key order: two reads of 4 keys x 16 dims per 16-lane group.
//   K image : 16-byte chunk c of key row r at slot c ^ ((r >> 1) & 7) (a
//             16-lane group of the A-operand read covers all 64 banks);
//   V image : chunk c of row r at slot c ^ (((r >> 1) & 1) << 2): the four rows
//             of a transposed read (r0 .. r0 + 3, r0 % 4 == 0) put their 64
//             bytes in four disjoint quarter-banks.
// s_waitcnt vmcnt(n) for a wave-uniform n in [0, N] (the count is an immediate)
template <int N>
__device__ __forceinline__ void vm_wait_younger(int n) {
  if constexpr (N > 0) {
    if (n >= N) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
      return;
    }
    vm_wait_younger<N - 1>(n);
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
}

// ABL (A/B timing probes only): 1 = no exponentials, 2 = no K/V DMA, 3 = no softmax VALU.
// PH2: the K/V load in two phases, keys [0, 64 c0) (c0 = spad / 128 chunks) first; the wave's first query
// block, its Q loaded ahead of the DMAs, starts on the first phase's keys after one
// barrier and takes a second barrier (vmcnt(0)) before chunk c0, so the second half of
// the 148 KB load (S = 577) arrives under the first half's math instead of before it.
template <int NW, bool TT2 = true, int ABL = 0, bool PH2 = false>
__global__ __launch_bounds__(NW * 64) void attention_r32_kernel(const uint16_t* __restrict__ qkv,
                                                                uint16_t* __restrict__ out, int S, int W, int H,
                                                                uint8_t* __restrict__ q8, uint8_t* __restrict__ qs,
                                                                int64_t rows_pad, int stagger_ticks) {
  extern __shared__ __attribute__((aligned(16))) char r32_lds[];
  const int spad = (S + 31) & ~31;
  char* Kimg = r32_lds;
  char* Vimg = r32_lds + spad * 128;
  const int item = blockIdx.x;
  const int bseq = item / H, head = item % H;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t ld = 3 * (int64_t)W;
  const uint16_t* qb = qkv + (int64_t)bseq * S * ld + head * 64;
  const uint16_t* kb = qb + W;
  const uint16_t* vb = qb + 2 * W;

  // ---- K, V -> LDS (one DMA instruction = 8 rows; rows >= S clamped copies)
  // The first workgroups on the CUs start together and, all taking the same
  // time, would keep issuing their K/V loads (148 KB each at S = 577) in
  // chip-wide bursts; a start delay of 0-3 quarters of a workgroup's time on
  // the first workgroup of each CU spreads them out for the rest of the grid.
  if (stagger_ticks > 0 && (int)blockIdx.x < 256) {
    const int ph = (blockIdx.x >> 3) & 3;
    if (ph) {
      const uint64_t until = __builtin_amdgcn_s_memrealtime() + (uint64_t)ph * stagger_ticks;
      while (__builtin_amdgcn_s_memrealtime() < until) __builtin_amdgcn_s_sleep(8);
    }
  }
  const int nch = (S + 63) >> 6;
  const int nr8 = spad >> 3;
  const int c0 = PH2 ? max(1, nr8 >> 4) : nch;   // chunks of the first load phase (nr8 >= 12 for S > 64)
  static_assert(!PH2 || (NW == 12 && !TT2), "attention_r32: the two-phase load's slot count assumes 12 waves");
  // NI2 (below) x 12 waves >= 2 nr8 for spad <= 640
  bf16x8 qf0[4];
  if (PH2) {   // the first block's Q, ahead of the DMAs: waiting for it drains none of them
    const int qrow = min(wave * 32 + (lane & 31), S - 1);
#pragma unroll
    for (int s = 0; s < 4; ++s) qf0[s] = *(const bf16x8*)(qb + (int64_t)qrow * ld + 16 * s + 8 * (lane >> 5));
  }
  // PH2: NI2 DMA slots per wave in global order g = wave + 12 k, so each wave issues its
  // first-phase blocks (g < 2 h0: K then V blocks of keys < 64 c0) before its second-phase
  // ones; slots past the 2 nr8 blocks re-load the last block (identical bytes, same place)
  constexpr int NI2 = 14;
  const int h0 = 8 * c0;
  if (ABL != 2 && PH2) {
    const int slot = lane & 7;
    const int n1 = nr8 - h0;
#pragma unroll
    for (int k = 0; k < NI2; ++k) {
      const int g = min(wave + NW * k, 2 * nr8 - 1);
      const bool ph = g >= 2 * h0;
      const int j = ph ? g - 2 * h0 : g, cnt = ph ? n1 : h0;
      const bool isv = j >= cnt;
      const int i8 = (ph ? h0 : 0) + (isv ? j - cnt : j);
      const int rr = i8 * 8 + (lane >> 3);
      const int cc = isv ? (slot ^ (((rr >> 1) & 1) << 2)) : (slot ^ ((rr >> 1) & 7));
      glds16((isv ? vb : kb) + (int64_t)min(rr, S - 1) * ld + cc * 8, (isv ? Vimg : Kimg) + i8 * 1024);
    }
  }
  if (ABL != 2 && !PH2) {
    const int slot = lane & 7;
    for (int i = wave; i < 2 * nr8; i += NW) {
      const bool isv = i >= nr8;
      const int i8 = isv ? i - nr8 : i;
      const int rr = i8 * 8 + (lane >> 3);
      const int cc = isv ? (slot ^ (((rr >> 1) & 1) << 2)) : (slot ^ ((rr >> 1) & 7));
      glds16((isv ? vb : kb) + (int64_t)min(rr, S - 1) * ld + cc * 8, (isv ? Vimg : Kimg) + i8 * 1024);
    }
  }

  const int r = lane & 31, hh = lane >> 5;
  const int ksw = (r >> 1) & 7;
  // transposed V^T reads: lane 4q + p of each 16-lane group gives row q
  // (key 4 half + q of the 8-key half-step), dims 16 g + 4p .. + 3 of the
  // 32-dim block
  const int i16 = lane & 15, gq = (lane >> 4) & 1, tq = i16 >> 2, tp = i16 & 3;
  const int vrow = (4 * hh + tq) * 128 + 8 * (tp & 1);
  const int vof0 = vrow + 16 * ((0 + 2 * gq + (tp >> 1)) ^ ((tq >> 1) << 2));
  const int vof1 = vrow + 16 * ((4 + 2 * gq + (tp >> 1)) ^ ((tq >> 1) << 2));
  const int nqb = (S + 31) >> 5;
  const int last_keys = S - (nch - 1) * 64;   // 1..64

  if (PH2) {   // this wave's first-phase DMAs (and Q): the NI2 - n0 younger ones may stay in flight
    const int n0 = 2 * h0 > wave ? (2 * h0 - wave + NW - 1) / NW : 0;
    vm_wait_younger<NI2>(NI2 - min(n0, NI2));
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();

  auto blocks = [&](auto tt_c, int b0, int b1, bool first) {
    constexpr int TT = decltype(tt_c)::value;
    const int bq[2] = {b0, b1};
    bf16x8 qf[TT][4];
#pragma unroll
    for (int u = 0; u < TT; ++u) {
      const int qrow = min(bq[u] * 32 + r, S - 1);
#pragma unroll
      for (int s = 0; s < 4; ++s)
        qf[u][s] = PH2 && first ? qf0[s] : *(const bf16x8*)(qb + (int64_t)qrow * ld + 16 * s + 8 * hh);
    }
    float m[TT], l[TT];
    f32x16 o[TT][2];
#pragma unroll
    for (int u = 0; u < TT; ++u) {
      m[u] = -INFINITY;
      l[u] = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) o[u][0][i] = o[u][1][i] = 0.f;
    }

    // one 64-key chunk: NKB valid 32-key blocks, MASK: keys >= S inside them
    auto chunk = [&](auto nkb_c, auto mask_c, int c) {
      constexpr int NKB = decltype(nkb_c)::value;
      constexpr bool MASK = decltype(mask_c)::value;
      f32x16 x[TT][NKB];
#pragma unroll
      for (int kt = 0; kt < NKB; ++kt) {
        const char* kp = Kimg + (c * 64 + kt * 32 + r) * 128;
        bf16x8 kf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) kf[s] = *(const bf16x8*)(kp + 16 * ((2 * s + hh) ^ ksw));
#pragma unroll
        for (int u = 0; u < TT; ++u) {
          f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[0], qf[u][0], f32x16{}, 0, 0, 0);
#pragma unroll
          for (int s = 1; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[s], qf[u][s], acc, 0, 0, 0);
          x[u][kt] = acc;
        }
      }
#pragma unroll
      for (int u = 0; u < TT && ABL != 3; ++u) {
        if (MASK) {
#pragma unroll
          for (int kt = 0; kt < NKB; ++kt)
#pragma unroll
            for (int i = 0; i < 16; ++i)
              if (c * 64 + kt * 32 + c_row(i, hh) >= S) x[u][kt][i] = -INFINITY;
        }
        float cm = x[u][0][0];
#pragma unroll
        for (int kt = 0; kt < NKB; ++kt)
#pragma unroll
          for (int i = (kt ? 0 : 1); i < 16; ++i) cm = fmaxf(cm, x[u][kt][i]);
        cm = group_max<false>(cm);
        const float cmu = cm * sl2;   // finite: chunk 0 holds key 0 for every row
        lazy_rescale(m[u], l[u], o[u], cmu);
        float ps = 0.f;
#pragma unroll
        for (int kt = 0; kt < NKB; ++kt) {
#pragma unroll
          for (int i = 0; i < 16; ++i)
            x[u][kt][i] = ABL == 1 ? fmaf(x[u][kt][i], sl2, -m[u]) : __builtin_amdgcn_exp2f(fmaf(x[u][kt][i], sl2, -m[u]));
#pragma unroll
          for (int i = 0; i < 16; i += 4) ps += (x[u][kt][i] + x[u][kt][i + 1]) + (x[u][kt][i + 2] + x[u][kt][i + 3]);
        }
        l[u] += ps;
      }
#pragma unroll
      for (int kt = 0; kt < NKB; ++kt)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const char* vp = Vimg + (c * 64 + kt * 32 + 16 * s) * 128;
          const bf16x8 v0 = vfrag(vp + vof0, 8 * 128);
          const bf16x8 v1 = vfrag(vp + vof1, 8 * 128);
#pragma unroll
          for (int u = 0; u < TT; ++u) {
            uint32_t pk[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) pk[j] = pack_bf16x2(x[u][kt][8 * s + 2 * j], x[u][kt][8 * s + 2 * j + 1]);
            typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
            const bf16x8 pb = __builtin_bit_cast(bf16x8, (u32x4_t){pk[0], pk[1], pk[2], pk[3]});
            o[u][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v0, pb, o[u][0], 0, 0, 0);
            o[u][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v1, pb, o[u][1], 0, 0, 0);
          }
        }
    };
    for (int c = 0; c < nch - 1; ++c) {
      if (PH2 && first && c == c0) {   // the second load phase (every wave passes here once)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
      chunk(Int<2>{}, std::bool_constant<false>{}, c);
    }
    if (PH2 && first && c0 >= nch - 1) {   // short sequences: the second phase before the last chunk
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    if (last_keys > 32) chunk(Int<2>{}, std::bool_constant<true>{}, nch - 1);
    else chunk(Int<1>{}, std::bool_constant<true>{}, nch - 1);

    // The epilogue of the 32x32 layout has this one site and stays written out: as a member of
    // AttnOut beside store16 it moved instructions in the product kernel's K/V load loop
    // (profiles/attention_isa.log).
#pragma unroll
    for (int u = 0; u < TT; ++u) {
      const float inv = 1.0f / group_sum<false>(l[u]);
      const int qrow = bq[u] * 32 + r;
      // o[u][db][i]: query qrow, head dim 32 db + (i & 3) + 8 (i >> 2) + 4 hh
      if (q8) {   // MX-fp8 output: this head's 64 dims are one 64-k block of out_proj
        float amax = 0.f;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(o[u][db][i] * inv));
        amax = group_max<false>(amax);
        const int X = mx_block_exp(amax);
        const float scl = ldexpf(1.0f, -X);
        if (qrow < S) {
          const int64_t row = (int64_t)bseq * S + qrow;
          uint8_t* dst = q8 + row * W + head * 64 + 4 * hh;
#pragma unroll
          for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int t = 0; t < 4; ++t)
              *(uint32_t*)(dst + 32 * db + 8 * t) = mx_pack4(o[u][db][4 * t] * inv, o[u][db][4 * t + 1] * inv,
                                                             o[u][db][4 * t + 2] * inv, o[u][db][4 * t + 3] * inv, scl);
          if (hh == 0) qs[mx_scale_index(row, head, rows_pad)] = (uint8_t)(X + 127);
        }
        continue;
      }
      if (qrow < S) {
        uint16_t* dst = out + ((int64_t)bseq * S + qrow) * W + head * 64 + 4 * hh;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int t = 0; t < 4; ++t)
            *(uint2*)(dst + 32 * db + 8 * t) = make_uint2(pack_bf16x2(o[u][db][4 * t] * inv, o[u][db][4 * t + 1] * inv),
                                                          pack_bf16x2(o[u][db][4 * t + 2] * inv, o[u][db][4 * t + 3] * inv));
      }
    }
  };
  if (TT2) {
    for (int b = wave; b < nqb; b += 2 * NW) {
      if (b + NW < nqb) blocks(Int<2>{}, b, b + NW, false);
      else blocks(Int<1>{}, b, b, false);
    }
  } else {
    if (PH2 && wave >= nqb) {   // no block: the second phase's barrier all the same
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    for (int b = wave; b < nqb; b += NW) blocks(Int<1>{}, b, b, b == wave);
  }
}

}  // namespace

// A compile-time kernel pointer handed to a generic lambda (launch_kernel<K::value>)
template <auto KERNEL>
using Kern = std::integral_constant<decltype(KERNEL), KERNEL>;

hipError_t attention(const uint16_t* qkv, uint16_t* out, int B, int S, int W, int flags, hipStream_t s, uint8_t* q8,
                     uint8_t* qs, uint16_t* cls_out, int64_t cls_pitch) {
  const int H = W / 64;
  const int items = B * H;
  if (items <= 0) return hipSuccess;
  if (S > 640) return hipErrorInvalidValue;
  // Every length has a flash kernel (scripts/attn_micro.py, this
  // round: B/32 S=50 177 vs 181 us for the one-wave kernel, text S=77 25.9 vs
  // 30.0, L/14 408 vs 572 and L/14@336 547 vs 1004 for the per-query-tile-K
  // kernel it replaced).  ATT_ONE_WAVE selects the one-wave kernel for S <= 96
  // (A/B and parity tests of both paths; it has no fp8 output).

  // ---- 1. flags (AttnFlags, internal.hpp)
#if MICLIP_AB
  const bool one_wave = (flags & ATT_ONE_WAVE) && S <= 96 && !q8;
#else
  if (flags & ATT_ONE_WAVE) return hipErrorNotSupported;   // the one-wave kernel is in the A/B build only
  constexpr bool one_wave = false;
#endif
  const bool stream = flags & ATT_STREAM;   // A/B: the chunk-streaming flash kernel for S > 64
  const int q0 = flags & ATT_Q0_ONLY;       // the first query tile only (S <= 64 kernel; others compute all)
  const int causal = flags & ATT_CAUSAL;
  const int64_t rows_pad = ((int64_t)B * S + 1) & ~1;   // rows of the MX scale layout (mx_scale_index)
  const size_t res_lds = 2 * (size_t)((S + 31) & ~31) * 128;   // resident kernels: the K and V images

  // ---- 2. S <= 64: attention_s64_kernel in its measured shape S64_SHAPE (bit 0: 2 waves x 2 tiles instead of
  // 4 x 1, bit 1: K fragments from global memory, bit 2: V row-major in LDS, read transposed, bits 3 up:
  // the output store form; -1: the flash body's single-chunk instance in section 5).  cls_out: the CLS-row form,
  // row 0 of every sequence into the compact rows (ATT_Q0_ONLY, bf16 output).  A/B: MICLIP_ATTN_SHORT, 100 + shape
  // (+ 8 x the output store form, below), 30 for the flash body's instance, the older variants described
  // at their kernels.
  // Measured (scripts/attn_micro.py): 2 waves x 2 tiles, K and transposed V in LDS, whole-line
  // nontemporal stores (shape 1 + 8 x 5); the CLS form on 4 waves.  ATT_Q0_ONLY without compact rows (A/B,
  // MICLIP_CLS_ATT=0) stays on the flash body's instance, which stops after the first tile.
  constexpr int S64_SHAPE = 41, S64_CLS_SHAPE = 0;
  if (cls_out && (!q0 || S > 64 || q8 || causal || one_wave || stream)) return hipErrorInvalidValue;
  if (!one_wave && !stream && S <= 64) {
    auto s64 = [&](auto shape) {
      constexpr int SH = decltype(shape)::value;
      constexpr int NWV = (SH & 1) ? 2 : 4;
      constexpr bool KG = SH & 2, VTR = SH & 4;
      // output stores: 0 8 bytes a lane; 1 16 bytes (64 contiguous a row); 3 whole 128-byte lines through LDS (shapes
      // with a K image); 4 / 5: 1 / 3 nontemporal; 2: none (A/B timing probe)
      constexpr int ST = SH >> 3;
      auto go = [&](auto cls, uint16_t* dst, int cz) {
        constexpr bool CLS = decltype(cls)::value;
        constexpr int STK = CLS ? 0 : ST;   // (the CLS form stores one row on four lanes)
        if constexpr (NWV == 2)
          return launch_kernel(attention_s64w2_kernel<KG, VTR, CLS, STK>, items, 128, s, qkv, dst, S, W, H, cz, q8, qs,
                               rows_pad, cls_pitch);
        else
          return launch_kernel(attention_s64_kernel<KG, VTR, CLS, STK>, items, 256, s, qkv, dst, S, W, H, cz, q8, qs,
                               rows_pad, cls_pitch);
      };
      if (cls_out) return go(std::true_type{}, cls_out, 0);
      return go(std::false_type{}, out, causal);   // (ATT_Q0_ONLY without compact rows: every row is computed)
    };
#if MICLIP_AB
    const int sw = ab_env_int("MICLIP_ATTN_SHORT", 0);
    // 5x: persistent workgroups with the next item's operands prefetched, x workgroups per CU (a bare 5: 4 per
    // CU: 128 VGPRs)
    if (!cls_out && (sw == 5 || sw / 10 == 5)) {
      const int per = sw == 5 ? 4 : sw % 10;
      const int gp = std::min(items, cu_count() * (per > 0 ? per : 5));
      return launch_kernel(attention_pipe_kernel, gp, 256, s, qkv, out, S, W, H, causal, q8, qs, rows_pad, items);
    }
    if (sw >= 100)   // (16: the timing probe, shape 0 without its output stores)
      return with_value<0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 24, 25, 28, 29, 32, 33, 36, 37, 40, 41, 44,
                        45>(sw - 100, s64);
    if (!cls_out) switch (sw) {
      case 30:   // the flash body's single-chunk instance on 4 waves
        return launch_kernel(attention_flash_kernel<1, 2, 1>, items, 256, s, qkv, out, S, W, H, causal | q0, q8, qs, rows_pad);
      case 6:   // the V^T fragment reads batched
        return launch_kernel(attention_vb_kernel, items, 256, s, qkv, out, S, W, H, causal | q0, q8, qs, rows_pad);
      case 2:   // two heads per workgroup (an odd H: as 3)
        if (H % 2 == 0)
          return launch_kernel(attention_short2_kernel, items / 2, 512, s, qkv, out, S, W, H, causal, q8, qs, rows_pad);
        [[fallthrough]];
      case 3:   // the occupancy-targeted single-head kernel
        return launch_kernel(attention_short_kernel, items, 256, s, qkv, out, S, W, H, causal, q8, qs, rows_pad);
      case 1:   // non-causal: the resident-K/V kernel with 4 waves (causal: the default below)
        if (!causal)
          return launch_kernel<attention_res_kernel<4, false>>(items, 256, res_lds, s, qkv, out, S, W, H, q8, qs, rows_pad);
        break;
      default: break;
    }
#endif
    if (cls_out) return s64(Int<S64_CLS_SHAPE>{});
    if (S64_SHAPE >= 0 && !q0) return s64(Int<(S64_SHAPE >= 0 ? S64_SHAPE : S64_CLS_SHAPE)>{});
  }

  // ---- 3. vision towers (257 / 577 tokens): K/V resident in LDS, no per-chunk barriers
  if (!one_wave && !stream && !causal && S > 64) {
    // Defaults (scripts/attn_micro.py, r03): S <= 320 (L/14, 257 tokens) attention_res_kernel
    // with 8 waves, one 16-row query tile at a time; S > 320 (L/14@336, 577 tokens) the
    // 32x32x16 kernel with 12 waves, one 32-row block each (2157 us per 1000-frame chunk
    // against 2392 for attention_res_kernel).  The A/B variants (MICLIP_ATTN_VAR) are the cases below.
    int var = ab_env_int("MICLIP_ATTN_VAR", 0);
    if (var < 1 || var > 14) var = S > 320 ? 5 : 1;
    const int vr = S - 16 * ((S + 15) / 16 - 1);   // rows of the last query tile
    // 11 = 1; 12 / 13 (SPLIT) only for a nearly empty last tile (S % 16 in 1..4) and bf16 output (the merge
    // has no MX-fp8 store), otherwise 1
    if (var == 11 || ((var == 12 || var == 13) && !(vr <= 4 && !q8))) var = 1;
    auto res = [&](auto k, int threads, size_t lds) {
      return launch_kernel<decltype(k)::value>(items, threads, lds, s, qkv, out, S, W, H, q8, qs, rows_pad);
    };
    auto r32 = [&](auto k, int threads, int stagger_ticks) {
      return launch_kernel<decltype(k)::value>(items, threads, res_lds, s, qkv, out, S, W, H, q8, qs, rows_pad,
                                               stagger_ticks);
    };
    switch (var) {
      case 1: return res(Kern<attention_res_kernel<8, false>>{}, 512, res_lds);    // 8 waves x 1 tile
      case 5: return r32(Kern<attention_r32_kernel<12, false>>{}, 768, 0);         // 12 waves x 1 block
#if MICLIP_AB
      case 2: return res(Kern<attention_res_kernel<8, true>>{}, 512, res_lds);     // 8 waves x 2 tiles
      case 3: return res(Kern<attention_res_kernel<16, false>>{}, 1024, res_lds);  // 16 waves
      case 4: return r32(Kern<attention_r32_kernel<8, true>>{}, 512, 0);           // 8 waves x 2 blocks
      case 6:
      case 7:   // 5 with a start stagger of 1 / 2 quarter workgroup times
        return r32(Kern<attention_r32_kernel<12, false>>{}, 768, (var - 5) * (S * S / 378));
      case 8: return r32(Kern<attention_r32_kernel<12, false, 2>>{}, 768, 0);      // timing probe: no K/V load (wrong results)
      case 10: return r32(Kern<attention_r32_kernel<12, false, 0, true>>{}, 768, 0);   // 5 with the two-phase K/V load
      // 12: the nearly empty last query tile split over the 8 waves' key tiles (attention_res_kernel SPLIT).
      // Measured at L/14 (scripts/attn_micro.py, r04): 1074 vs 1031 us per 1667-frame chunk -- the second
      // workgroup on the CU already fills the idle waves -- so the unsplit kernel stays the default.
      case 12: return res(Kern<attention_res_kernel<8, false, true>>{}, 512, res_lds + (size_t)8 * vr * 68 * 4);
      // 13: the split tile first, then the full tiles, then the merge
      case 13: return res(Kern<attention_res_kernel<8, false, true, true>>{}, 512, res_lds + (size_t)8 * vr * 68 * 4);
      case 14: return res(Kern<attention_res_kernel<8, false, false, false, true>>{}, 512, res_lds);   // Q fragments one tile ahead
      default: return r32(Kern<attention_r32_kernel<12, false, 1>>{}, 768, 0);     // 9: timing probe, no exponentials (wrong results)
#else
      default: return hipErrorNotSupported;   // (no switch: var is 1 or 5)
#endif
    }
  }

  // ---- 4. A/B only: the one-wave kernel, whole padded sequence per wave
#if MICLIP_AB
  if (one_wave)
    return with_value<32, 64, 96>(std::max(32, (S + 31) & ~31), [&](auto sp) {
      return launch_kernel(attention_kernel<decltype(sp)::value>, items, 64, s, qkv, out, S, W, H, causal, items);
    });
#endif

  // ---- 5. flash
  // NT = ceil(tiles / 8) query tiles per wave on 8 waves; S <= 64 (here only with ATT_Q0_ONLY and no
  // compact rows, or as the A/B baseline; section 2 otherwise): one tile on
  // each of 4 waves, single slot.  Fewer waves with fewer idle tile slots
  // measured slower (L/14 257 tokens on 6 waves x 3 tiles: 470 vs 421 us; text
  // 77 on 5 x 1: 45 vs 31 us): a workgroup lasts as long as its busiest wave
  // either way, and 8 waves spread that wave's SIMD over fewer partners.
  const int nqt = (S + 15) / 16;
  if (nqt <= 4)
    return launch_kernel(attention_flash_kernel<1, 2, 1>, items, 256, s, qkv, out, S, W, H, causal | q0, q8, qs, rows_pad);
  return with_value<1, 2, 3, 4, 5>((nqt + 7) / 8, [&](auto nt) {
    return launch_kernel(attention_flash_kernel<decltype(nt)::value, 1>, items, 512, s, qkv, out, S, W, H, causal, q8, qs,
                         rows_pad);
  });
}

}  // namespace miclip
