// The GEMM family's shared helpers (gemm.hip, gemm_8q.hip, gemm_mx.hip and the A/B build's
// gemm_8p / gemm_8r / gemm_w4 / gemm_mx8q / gemm_1d): the only copy of each device helper and the
// host side's one launch idiom.
#pragma once
#include <cstdlib>
#include <type_traits>

#include "common.hpp"
#include "internal.hpp"

namespace miclip {
namespace {

// ------------------------------------------------------------------ device helpers

// compile-time phase number handed to the 8-phase kernels' generic lambdas (bools travel as
// std::bool_constant)
template <int P>
using Phase = std::integral_constant<int, P>;

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef int v8i __attribute__((ext_vector_type(8)));

// Half-tile ids of the 8-phase kernels (gemm_8p / gemm_8q / gemm_mx8q): issue / read order and slot
// in a K-tile buffer of four half-tiles
constexpr int H_A0 = 0, H_B0 = 1, H_B1 = 2, H_A1 = 3;
// gemm_8p / gemm_8q: K staged 64 wide; a half-tile is 128 rows x 64 bf16 / fp16
constexpr int BK8 = 64;
constexpr int HALF = 128 * BK8 * 2;   // 16 KB half-tile
constexpr int BUF = 4 * HALF;         // 64 KB K-tile buffer

// Logical tile t -> (m-block, n-block).  Tiles are taken in groups of `ng`
// n-blocks (ng <= 0 or >= tiles_n: plain m-major raster): within a group all m-blocks
// are swept with the group's n-blocks innermost, so the W column panel of the
// group stays L2-resident while the XCD streams A (each A panel is re-read by
// the ng concurrent tiles of its row).  With xcd_remap each XCD owns a
// contiguous run of t, i.e. one group and a contiguous range of m-blocks.
__device__ __forceinline__ void tile_coords(int t, int tiles_m, int tiles_n, int ng, int& mb, int& nb) {
  if (ng <= 0 || ng >= tiles_n) {
    mb = t / tiles_n;
    nb = t % tiles_n;
    return;
  }
  const int per = tiles_m * ng;
  const int g = t / per, r = t - g * per;
  const int ngg = min(ng, tiles_n - g * ng);
  mb = r / ngg;
  nb = g * ng + r % ngg;
}

// QuickGELU x * sigmoid(1.702 x) for bf16 / fp8 outputs comes in TWO forms that round differently
// (either is ~1 ulp of f32, far inside the output format; what matters is which kernels must agree
// bit for bit):
//   quick_gelu        __expf + rcp, per value: gemm.hip's kernels, gemm_w4 and EVERY MX kernel
//                     (gemm_mx.hip, gemm_mx8q.hip -- tests/test_gpu_mx.py holds them bit-identical);
//   quick_gelu_exp2   one exp2 with 1.702 * log2(e) folded in, packed multiplies / adds, per pair:
//                     the bf16 8-phase kernels gemm_8p / gemm_8q / gemm_8r / gemm_1d (bit-identical
//                     among themselves); quick_gelu_stage is the same arithmetic per value.
__device__ __forceinline__ float quick_gelu(float v) {
  return v * __builtin_amdgcn_rcpf(1.0f + __expf(-1.702f * v));
}
__device__ __forceinline__ f32x2 quick_gelu_exp2(f32x2 v) {
  const f32x2 t = v * (f32x2){-2.45546696f, -2.45546696f};   // -1.702 * log2(e)
  f32x2 e = {__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
  e = e + 1.0f;
  return v * (f32x2){__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y)};
}
// quick_gelu_exp2 over NP pairs in stage order (all multiplies, all exponentials, all adds, all
// reciprocals, all products), so consecutive transcendental ops are independent (gemm_8q F_GSTAGE)
// (PK: the adds as packed pairs -- the same additions, bit-identical; one wave alone issues a
// v_pk_add_f32 in 5.1 cycles against 4.7 for a v_add_f32, scripts/probes/valu_rate.hip)
template <int NP, bool PK = false>
__device__ __forceinline__ void quick_gelu_stage(f32x2 (&v)[NP]) {
  float e[2 * NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const f32x2 t = v[k] * (f32x2){-2.45546696f, -2.45546696f};
    e[2 * k] = t.x;
    e[2 * k + 1] = t.y;
  }
#pragma unroll
  for (int k = 0; k < 2 * NP; ++k) e[k] = __builtin_amdgcn_exp2f(e[k]);
  if (PK) {
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const f32x2 p = (f32x2){e[2 * k], e[2 * k + 1]} + (f32x2){1.0f, 1.0f};
      e[2 * k] = p.x;
      e[2 * k + 1] = p.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 2 * NP; ++k) e[k] = e[k] + 1.0f;
  }
#pragma unroll
  for (int k = 0; k < 2 * NP; ++k) e[k] = __builtin_amdgcn_rcpf(e[k]);
#pragma unroll
  for (int k = 0; k < NP; ++k) v[k] = v[k] * (f32x2){e[2 * k], e[2 * k + 1]};
}

// 16-byte-chunk permutation g = {0,2,3,1} of the 64-byte-row LDS images (gemm.hip header)
__device__ __forceinline__ int swz(int x) { return (0x1320 >> (4 * x)) & 0xF; }

// LDS read the compiler does not see: a plain ds_read of the bias would make
// hipcc wait vmcnt(0) (it cannot prove the read misses the in-flight LDS-DMA
// of the next tile's stages), draining the prefetch at every epilogue.
__device__ __forceinline__ float4 lds_read_f4(const float* p) {
  float4 v;
  const uint32_t addr = (uint32_t)(uintptr_t)(const LDS_AS float*)p;
  asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
  return v;
}

// lane id through asm: opaque to CSE / LICM, so offsets derived from it are rebuilt where used
// instead of hoisted out of the tile loop and held (or spilled) for the kernel's life
__device__ __forceinline__ int lane_id() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// ------------------------------------------------------------------ host: one launch idiom
// (launch_kernel, with_value and ab_env_int: internal.hpp)

inline int tile_count(const GemmArgs& a, int bm, int bn) { return ((a.M + bm - 1) / bm) * (a.N / bn); }
// persistent kernels: one workgroup per CU (per `cus` slots), fewer when there are fewer tiles
inline int persistent_grid(int nt, int cus) { return nt < cus ? nt : cus; }

// with_value for the epilogue (GemmEpi)
template <int... EPIS, class F>
hipError_t with_epi(int epi, F&& f) {
  return with_value<EPIS...>(epi, f);
}

}  // namespace
}  // namespace miclip
