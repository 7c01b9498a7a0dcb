// In-register OCP e4m3 -> bf16 dequantization shared by the fp8
// weight-only GEMMs (decode_gemm_w8.hip for M <= 32, gemm_w8.hip for any
// M). One definition, so both kernels multiply by bit-identical weights:
// the e4m3 value itself, exact in bf16; the per-channel scale is applied
// to the fp32 sum in each kernel's epilogue, never to the weights.
#pragma once

#include "common.h"

// The epilogues add and scale adjacent floats, which the compiler would
// fuse into packed-fp32 VALU ops; the kernels here are built without them.
#define RB_W8_NO_PK __attribute__((target("no-packed-fp32-ops")))

namespace rb {

typedef __attribute__((ext_vector_type(8))) __bf16 w8_bf16x8v;

// two e4m3 codes (the low or high half of w) -> one dword of two bf16: the
// conversion to f32 is exact and so is dropping the 16 low (zero) bits.
// Byte selector: 2,3 = the high half of the second operand, 6,7 = of the
// first.
template <bool HI>
RB_DEV uint32_t w8_pair(uint32_t w) {
  const auto f = __builtin_amdgcn_cvt_pk_f32_fp8(w, HI);
  const float lo = f[0], up = f[1];
  return __builtin_amdgcn_perm(__float_as_uint(up), __float_as_uint(lo),
                               0x07060302u);
}

// 8 codes (bytes 0..3 of w0, then of w1) -> 8 bf16 A-fragment elements
RB_DEV w8_bf16x8v w8_dequant8(uint32_t w0, uint32_t w1) {
  typedef __attribute__((ext_vector_type(4))) unsigned int u32x4v;
  union { u32x4v u; w8_bf16x8v v; } c;
  c.u[0] = w8_pair<false>(w0);
  c.u[1] = w8_pair<true>(w0);
  c.u[2] = w8_pair<false>(w1);
  c.u[3] = w8_pair<true>(w1);
  return c.v;
}

}  // namespace rb
