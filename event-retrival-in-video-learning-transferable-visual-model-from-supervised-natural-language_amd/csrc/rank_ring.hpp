// The row ring of the register-query rank passes (rank.hip rank_reg, rank_mirror.hip
// rank_mirror_kernel, rank_cert.hip rank_cert_kernel): one wave per SIMD, the 32 queries of the
// block held in registers, the corpus streamed through a per-wave LDS ring of 4-KB chunks (32 rows x
// 128 B) by buffer-descriptor DMA, PF chunks ahead, with counted vmcnt waits and no barriers (each
// wave fills and reads only its own slots).  Here: the ring (DMA side and read side of one layout),
// and the workgroup's LDS layout, which kernels and launchers both take from RingLds.
#pragma once
#include "internal.hpp"
#include "rank_keys.hpp"

namespace miclip {
namespace rankk {

constexpr int RING_NW = 4;           // waves per workgroup
constexpr int RING_SLOT = 32 * 128;  // one chunk: 32 rows x 128 B

// NB slots, PF chunks in flight, NCH chunks per 32-row tile (a row is NCH x 128 B).
// AHEAD: a chunk's fragments are read one chunk ahead (two register buffers), so the LDS latency
// hides under the previous chunk's MFMAs and the DMA lookahead is PF - 1 chunks beyond the one
// being read.
// Image: row r of a chunk at r * 128 B, its 16-byte piece p at slot p ^ ((r >> 1) & 7) (the
// GEMM's conflict-free image); the DMA permutes its source pieces, frag() undoes it.
// Invariants:
//  * chunk c + PF goes into slot (c + PF) % NB, issued at the top of chunk c's iteration, only
//    after the chunk that slot held, c + PF - NB, was read and its reads waited for.  Read after
//    the wait, that is an earlier iteration's lgkmcnt(0): c + PF - NB <= c - 1.  Read AHEAD, chunk
//    c's fragments were read in iteration c - 1 and are waited for before iteration c's issue():
//    c + PF - NB <= c;
//  * the counted wait (4 DMA instructions per chunk) fits the 6-bit vmcnt field.
template <int NB_, int PF_, int NCH_, bool AHEAD_ = false>
struct RowRing {
  static constexpr int NB = NB_, PF = PF_, NCH = NCH_, SLOT = RING_SLOT;
  static constexpr bool AHEAD = AHEAD_;
  // s_waitcnt vmcnt(WAIT) after an iteration's issue(): the chunk whose fragments are read next
  // has landed (AHEAD: the next chunk, PF - 1 younger ones in flight; else this one, PF younger)
  static constexpr int WAIT = 4 * (AHEAD ? PF - 1 : PF);
  static_assert(NB >= PF + (AHEAD ? 0 : 1), "row ring: a refilled slot must have been read in an earlier chunk");
  static_assert(4 * PF <= 63, "row ring: vmcnt(4 PF) exceeds the counter");

  const char* corpus;   // the rows streamed: row i at i * NCH * 128 B
  int64_t r_begin;      // the workgroup's range of them: its first row ...
  int nrows;            // ... and its rows: candidates carry 32-bit rows of the range, and the load cursor's tile
                        // row (int) runs up to PF chunks past the last tile, so nrows < 2^31 - 128 (PF / NCH + 2)
  int wave;             // this wave's tile t is 32-row tile wave + RING_NW t of the range
  char* wring;          // this wave's NB slots
  int rbase, sw;        // this lane's fragment row r = lane & 31: its byte offset in a slot, its piece swizzle
  uint32_t voff[4];
  int lt = 0, lj = 0, lslot = 0;   // load cursor: tile ordinal, chunk, ring slot
  __amdgpu_buffer_rsrc_t rs;

  // ring: the workgroup's [RING_NW][NB][SLOT]
  __device__ __forceinline__ RowRing(const void* corpus_, int64_t r_begin_, int nrows_, char* ring, int wave_,
                                     int lane)
      : corpus((const char*)corpus_), r_begin(r_begin_), nrows(nrows_), wave(wave_), wring(ring + wave_ * NB * SLOT),
        rbase((lane & 31) * 128), sw(((lane & 31) >> 1) & 7) {
    // DMA: 4 x 1 KB per chunk; instruction m covers image rows 8m .. 8m + 7,
    // lane l row 8m + (l >> 3), LDS slot (l & 7), source piece (l & 7) ^ ((row >> 1) & 7)
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int row = 8 * m + (lane >> 3);
      const int c = (lane & 7) ^ ((row >> 1) & 7);
      voff[m] = (uint32_t)(row * NCH * 128 + c * 16);
    }
    make_rs();
  }
  // first row (of the range) of this wave's tile t
  __device__ __forceinline__ int tile_row(int t) const { return (wave + RING_NW * t) * 32; }
  // descriptor of tile lt: base its first row, range its valid rows, so rows past the range (and
  // tiles past the wave's last) read zeros
  __device__ __forceinline__ void make_rs() {
    const int trow = tile_row(lt);
    const int n = max(0, min(32, nrows - trow));
    // wave-uniform by construction; readfirstlane makes it provable (no waterfall loop per load, guide T20)
    const uint64_t base = (uint64_t)(uintptr_t)(corpus + (r_begin + (n ? trow : 0)) * (int64_t)(NCH * 128));
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)base);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
    const int nrec = __builtin_amdgcn_readfirstlane(n * NCH * 128);
    rs = __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)(((uint64_t)hi << 32) | lo), (short)0, nrec, 0x00020000);
  }
  // chunk (lt, lj) -> slot lslot, cursor advanced
  __device__ __forceinline__ void issue() {
    char* dst = wring + lslot * SLOT;
#pragma unroll
    for (int m = 0; m < 4; ++m)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (LDS_AS void*)(dst + m * 1024), 16, voff[m], lj * 128, 0, 0);
    lslot = lslot == NB - 1 ? 0 : lslot + 1;
    if (++lj == NCH) {
      lj = 0;
      ++lt;
      make_rs();
    }
  }
  // LDS address of this lane's row's 16-byte piece `piece` of the chunk in `slot`
  __device__ __forceinline__ uint32_t frag(int slot, int piece) const {
    return (uint32_t)(uintptr_t)(const LDS_AS char*)(wring + slot * SLOT + rbase + ((piece ^ sw) << 4));
  }
};

// The workgroup's dynamic LDS, for kernel and launcher alike: the ring [RING_NW][NB][SLOT], the
// per-wave row reciprocals [RING_NW][32] f32 (NORMS), tau [32] u32, the lead keys [32][8] u32,
// then EXTRA bytes of the kernel's own.  A kernel whose ring is larger than the launch's
// allocation puts what follows the ring past the end of the workgroup's LDS, where reads return
// zero (round 2's 9-slot attempt: every score came out 0).  The merge tails reuse
// the area from its start.
template <int NB, bool NORMS, size_t EXTRA = 0>
struct RingLds {
  static constexpr size_t nrm = (size_t)RING_NW * NB * RING_SLOT;
  static constexpr size_t tau = nrm + (NORMS ? RING_NW * 32 * 4 : 0);
  static constexpr size_t lead = tau + FQ * 4;
  static constexpr size_t extra = lead + LEAD_LDS;
  static constexpr size_t bytes = extra + EXTRA;
  static_assert(bytes <= 160 * 1024, "ring kernel: LDS layout exceeds the CU's 160 KB");
  static_assert(bytes >= (size_t)64 * RING_NW * 16 * 8, "ring kernel: list merge area exceeds the allocation");
  static_assert(bytes >= fold_lds(64 * RING_NW), "ring kernel: in-launch merge area exceeds the allocation");
};

}  // namespace rankk
}  // namespace miclip
