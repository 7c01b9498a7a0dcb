// Fragment types and the C -> B repack for v_mfma_f32_32x32x16_bf16, shared
// by the flash-attention forward (flash_fwd_core.h) and backward
// (attention_bwd.hip).
//
// mfma_f32_32x32x16_bf16 layouts (cdna_hip_programming.md §3):
//   A[i][k]: i = lane&31, k = (lane>>5)*8 + e (e = 0..7)
//   B[k][j]: j = lane&31, k = (lane>>5)*8 + e
//   C[i][j]: j = lane&31, i = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
// mfma_probe_32x32x16 (attention_prefill.hip) checks these maps on the GPU.
#pragma once

#include "common.h"

namespace rb {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8v;
typedef __attribute__((ext_vector_type(16))) float f32x16v;

RB_DEV unsigned pack_bf16(float lo, float hi) {
  union { __bf16 b; unsigned short u; } a, b;
  a.b = (__bf16)lo;
  b.b = (__bf16)hi;
  return ((unsigned)b.u << 16) | a.u;
}

RB_DEV bf16x8v frag_from_words(unsigned w0, unsigned w1, unsigned w2, unsigned w3) {
  union { unsigned u[4]; bf16x8v v; } c;
  c.u[0] = w0; c.u[1] = w1; c.u[2] = w2; c.u[3] = w3;
  return c.v;
}

// C-layout values (16 regs = 32 i-rows, this lane's column j) -> the B
// fragment of the same column for k = i in [16*kslot, 16*kslot + 16).
// A lane holds i = 8*(r>>2) + 4*hi + (r&3): of the 8 consecutive k a B
// fragment needs, it has 4 and lane^32 has the other 4, so the values are
// rounded to bf16 pairs (v_cvt) and the halves traded with
// v_permlane32_swap.
RB_DEV bf16x8v repack_c_to_b(const float *p, int kslot) {
  const int r0 = kslot * 8;
  unsigned pk0 = pack_bf16(p[r0 + 0], p[r0 + 1]);
  unsigned pk1 = pack_bf16(p[r0 + 2], p[r0 + 3]);
  unsigned pk2 = pack_bf16(p[r0 + 4], p[r0 + 5]);
  unsigned pk3 = pack_bf16(p[r0 + 6], p[r0 + 7]);
  auto r02 = __builtin_amdgcn_permlane32_swap(pk0, pk2, false, false);
  auto r13 = __builtin_amdgcn_permlane32_swap(pk1, pk3, false, false);
  return frag_from_words(r02[0], r13[0], r02[1], r13[1]);
}

}  // namespace rb
