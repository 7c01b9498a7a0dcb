// Shared by the bf16 weight-stream GEMMs (decode_gemm.hip, M <= 32, and
// decode_gemm_mt.hip, 32 < M <= 256): fragment types and loads, the weight
// layout tags with their un-permuting column map.
// Both kernels read the SAME swizzled weight copy ([N/32][K/16][lane][8],
// decode_swizzle_w) and keep one summation order per output, so these must
// stay one definition. Everything here has internal linkage.
#pragma once

#include <torch/extension.h>

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8v;
typedef __attribute__((ext_vector_type(16))) float f32x16v;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4v;

__device__ __forceinline__ bf16x8v nt_load8v(const uint16_t *p) {
  union { u32x4v u; bf16x8v v; } c;
  c.u = __builtin_nontemporal_load(reinterpret_cast<const u32x4v *>(p));
  return c.v;
}

__device__ __forceinline__ bf16x8v load8v(const uint16_t *p) {
  union { u32x4v u; bf16x8v v; } c;
  c.u = *reinterpret_cast<const u32x4v *>(p);
  return c.v;
}

// ---- weight layout tags and epilogue modes -----------------------------
// The swizzled weight copy may hold its rows PERMUTED so that the values
// an elementwise consumer pairs up land in one workgroup's 32-row block:
//   LAYOUT_GLU16  fused gate-up [2I, K]: block b = gate rows 16b..16b+15
//                 (local rows 0..15) + up rows 16b..16b+15 (16..31).
//   LAYOUT_ROPE16 fused qkv: inside each q/k head, block j of the head =
//                 rows d = 16j..16j+15 (local 0..15) + their rotate-half
//                 partners d + Dh/2 (local 16..31); v heads in order.
// A row permutation leaves every output's k-order and the 4-way LDS
// reduce order alone, so each sum is bit-identical to the plain layout.
// EPI_*_STORE write y row-major at the ORIGINAL column (4 consecutive
// local rows stay 4 consecutive columns); the fused modes consume the
// block in place of swiglu/geglu_packed_dec and qkv_rope_append.
enum { LAYOUT_PLAIN = 0, LAYOUT_GLU16 = 1, LAYOUT_ROPE16 = 2 };
enum { EPI_PLAIN = 0, EPI_GLU_STORE, EPI_ROPE_STORE, EPI_SWIGLU, EPI_GEGLU,
       EPI_ROPE, EPI_ROPE_VT };

struct EpiArgs {
  int inter;                   // glu16: I
  int hq, hkv, dh, bs;         // rope16: heads, head dim, cache block size
  uint16_t *swz;               // glu: down-proj operand [I/16][64][8]
  uint16_t *q_out;             // rope: [M, Hq, Dh]
  uint16_t *k_cache, *v_cache;
  const float *cs, *sn;        // [max_pos, Dh/2] f32
  const int32_t *pos, *slots;  // [M]
};

// original y column of local row `en` (a multiple of 4) of block nblk
template <int EPI>
__device__ __forceinline__ int epi_col(int nblk, int en, const EpiArgs &e) {
  if constexpr (EPI == EPI_GLU_STORE) {
    return (en < 16 ? 0 : e.inter - 16) + nblk * 16 + en;
  } else if constexpr (EPI == EPI_ROPE_STORE) {
    const int bph = e.dh / 32;
    const int head = nblk / bph;
    if (head >= e.hq + e.hkv) return nblk * 32 + en;
    const int j = nblk - head * bph;
    return head * e.dh + 16 * j + (en & 15) + (en < 16 ? 0 : e.dh / 2);
  } else {
    return nblk * 32 + en;
  }
}

// Validates a layout tag's arguments against N and fills the fields
// epi_col reads.
inline EpiArgs layout_args(int64_t layout, int64_t N, int64_t hq, int64_t hkv,
                           int64_t dh) {
  EpiArgs ep = {};
  TORCH_CHECK(layout >= LAYOUT_PLAIN && layout <= LAYOUT_ROPE16,
              "decode_gemm: unknown weight layout ", layout);
  if (layout == LAYOUT_GLU16) {
    TORCH_CHECK(N % 32 == 0, "decode_gemm: glu16 needs I % 16 == 0");
    ep.inter = (int)(N / 2);
  } else if (layout == LAYOUT_ROPE16) {
    TORCH_CHECK(dh > 0 && dh % 32 == 0 && (hq + 2 * hkv) * dh == N,
                "decode_gemm: rope16 needs (Dh/2) % 16 == 0 and "
                "N == (Hq + 2*Hkv) * Dh");
    ep.hq = (int)hq; ep.hkv = (int)hkv; ep.dh = (int)dh;
  }
  return ep;
}

}  // namespace
