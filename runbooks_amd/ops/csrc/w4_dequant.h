// In-register int4 -> bf16 dequantization shared by the int4 weight-only
// GEMMs (decode_gemm_w4.hip for M <= 32, gemm_w4.hip for any M). One
// definition, so both kernels multiply by bit-identical weights and
// ops/linear.py dequantize_int4(q, s, bf16) is the exact weight reference
// for both: (nibble - 8) * float(scale) in fp32, round-to-nearest-even bf16.
#pragma once

#include "common.h"

namespace rb {

typedef __attribute__((ext_vector_type(8))) __bf16 w4_bf16x8v;

// byte b of `bytes` (a nibble value n = 0..15) -> the f32 128 + n, built
// by one byte permute: 0x43000000 is 128.0f and mantissa bit 16 weighs 1,
// so dropping n into byte 2 adds exactly n. (Byte selector: 7 = byte 3 of
// the first operand, b = byte b of the second, 0x0C = constant zero.)
template <int B>
RB_DEV float w4_byte_to_f32(uint32_t bytes) {
  union { uint32_t u; float f; } c;
  c.u = __builtin_amdgcn_perm(0x43000000u, bytes, 0x07000C0Cu | (B << 16));
  return c.f;
}

// 8 nibbles of one dword -> 8 bf16 A-fragment elements; nb = -136 * s, so
// fma(128 + n, s, nb) == (n - 8) * s exactly (every term fits 16 bits).
RB_DEV w4_bf16x8v w4_dequant8(uint32_t w, float s, float nb) {
  const uint32_t even = w & 0x0F0F0F0Fu;          // nibbles 0,2,4,6
  const uint32_t odd = (w >> 4) & 0x0F0F0F0Fu;    // nibbles 1,3,5,7
  w4_bf16x8v v;
  v[0] = (__bf16)__builtin_fmaf(w4_byte_to_f32<0>(even), s, nb);
  v[1] = (__bf16)__builtin_fmaf(w4_byte_to_f32<0>(odd), s, nb);
  v[2] = (__bf16)__builtin_fmaf(w4_byte_to_f32<1>(even), s, nb);
  v[3] = (__bf16)__builtin_fmaf(w4_byte_to_f32<1>(odd), s, nb);
  v[4] = (__bf16)__builtin_fmaf(w4_byte_to_f32<2>(even), s, nb);
  v[5] = (__bf16)__builtin_fmaf(w4_byte_to_f32<2>(odd), s, nb);
  v[6] = (__bf16)__builtin_fmaf(w4_byte_to_f32<3>(even), s, nb);
  v[7] = (__bf16)__builtin_fmaf(w4_byte_to_f32<3>(odd), s, nb);
  return v;
}

}  // namespace rb
