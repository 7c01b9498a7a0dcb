// The flash-attention forward body (causal, bf16) for CDNA4 (gfx950), shared
// by the dense kernel (attention_prefill.hip) and the paged-cache kernel
// (attention_prefill_paged.hip). Both are flash_fwd_rows (the KV loop) with
// a different KV source, then flash_fwd_store (the epilogue), so their rows
// are bit-identical by construction.
//
// MFMA-native design following the CDNA4 attention recipe:
//  * workgroup = 8 waves; each wave owns 32 query rows (WG tile = 256).
//  * KV tiles of 64 keys, aligned to absolute key 0, staged to LDS; K
//    row-major, V TRANSPOSED ([d][key]) so both QK^T and PV read 16 B/lane
//    fragments. Rows padded +16 B so the b128 column-slice reads are
//    bank-conflict-free (stride/4 mod 64 cycles through distinct banks; no
//    XOR swizzle).
//  * swapped QK^T: mfma(A=K, B=Q) so the C layout has qrow = lane&31 —
//    the whole softmax row lives on a lane pair (l, l^32); row max is a
//    16-reg in-lane reduce + one shfl_xor(32).
//  * online softmax in registers; P repacked to PV B fragments with
//    repack_c_to_b (mfma_frag.h, which also holds the fragment maps).
//  * PV: mfma(A=V^T, B=P^T) accumulating O^T in 16-reg tiles.
//
// A row's result depends only on the sequence of 32-key sub-tiles from key
// 0: a fully masked sub-tile is an exact no-op (alpha == 1, p == 0), so
// where a workgroup's first row sits changes nothing.
#pragma once

#include <type_traits>

#include <c10/util/Exception.h>
#include <hip/hip_runtime.h>

#include "mfma_frag.h"

namespace rb {

constexpr int FLASH_BLOCK = 512;  // 8 waves
constexpr int FLASH_KVB = 64;     // keys per LDS tile

// dynamic LDS of one workgroup: K image [KVB][DH*2+16] + V^T image
// [DH][KVB*2+16]
template <int DH>
constexpr size_t flash_fwd_smem() {
  return FLASH_KVB * (DH * 2 + 16) + DH * (FLASH_KVB * 2 + 16);
}

// A lane's running state for its query row: O^T (unnormalised), row max
// and this lane's half of the row sum.
template <int DH>
struct FlashAcc {
  f32x16v o[DH / 32];
  float m, l;
};

// The KV loop for the workgroup's 256 rows, of which this lane's is `q`:
//   q        the row's DH queries (any readable row if !q_valid)
//   qrow     its absolute position: keys [0, qrow] are visible
//   S        keys exist at [0, S)
//   row0     absolute position of the workgroup's first row
// KV is a struct with
//   template <int DH> RB_DEV void stage(int kt, char *k_img, char *v_img) const
// that fills the K image ([KVB][DH*2+16], row-major) and the V^T image
// ([DH][KVB*2+16]) with keys [kt*KVB, kt*KVB + KVB), zeros at keys >= S.
template <int DH, class KV>
RB_DEV FlashAcc<DH> flash_fwd_rows(const uint16_t *q, int qrow, bool q_valid,
                                   int S, int row0, const KV &kv,
                                   float scale) {
  constexpr int KVB = FLASH_KVB;
  constexpr int KSTEPS = DH / 16;       // QK^T contraction steps
  constexpr int DTILES = DH / 32;       // O column tiles
  constexpr int K_STRIDE = DH * 2 + 16; // K row bytes (+16 pad)
  constexpr int V_STRIDE = KVB * 2 + 16;  // V^T row bytes (+16 pad)

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *k_img = smem;                       // [KVB][K_STRIDE]
  char *v_img = smem + KVB * K_STRIDE;      // [DH][V_STRIDE]

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int hi = lane >> 5;
  const int col = lane & 31;                // qrow within the wave tile

  // ---- Q fragments (B operand of swapped QK^T), pre-scaled --------------
  bf16x8v qf[KSTEPS];
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks) {
    const uint16_t *src = q + ks * 16 + hi * 8;
    float f[8];
    VIO<uint16_t>::load(src, f);
    union { unsigned short u[8]; bf16x8v v; } c;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      c.u[e] = f32_to_bf16(q_valid ? f[e] * scale : 0.0f);
    qf[ks] = c.v;
  }

  FlashAcc<DH> acc;
  f32x16v (&acc_o)[DTILES] = acc.o;
  float &m_run = acc.m, &l_run = acc.l;
#pragma unroll
  for (int dt = 0; dt < DTILES; ++dt) acc_o[dt] = (f32x16v)(0.0f);
  m_run = -INFINITY;
  l_run = 0.0f;

  const int kv_end = min(S, row0 + 256);  // causal upper bound for this WG
  const int n_tiles = (kv_end + KVB - 1) / KVB;
  const int wave_kmax = row0 + wid * 32 + 31;  // last key this wave can see

  for (int kt = 0; kt < n_tiles; ++kt) {
    const int kbase = kt * KVB;

    kv.template stage<DH>(kt, k_img, v_img);
    __syncthreads();

    if (kbase <= wave_kmax) {
      // two 32-key sub-tiles per LDS tile
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        // ---- QK^T^T: scores[key][qrow] ----------------------------------
        f32x16v s = (f32x16v)(0.0f);
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
          const bf16x8v kf = *reinterpret_cast<const bf16x8v *>(
              k_img + (it * 32 + col) * K_STRIDE + (ks * 16 + hi * 8) * 2);
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s, 0, 0, 0);
        }

        // ---- mask + online softmax --------------------------------------
        float p[16];
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kbase + it * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
          p[r] = (key <= qrow) ? s[r] : -INFINITY;
          mx = fmaxf(mx, p[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));     // full row max
        const float mn = fmaxf(m_run, mx);
        if (mn != -INFINITY) {
          const float alpha = (m_run == -INFINITY) ? 0.0f : __expf(m_run - mn);
          float psum = 0.0f;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            p[r] = (p[r] == -INFINITY) ? 0.0f : __expf(p[r] - mn);
            psum += p[r];
          }
          l_run = l_run * alpha + psum;
          m_run = mn;
          if (alpha != 1.0f) {
#pragma unroll
            for (int dt = 0; dt < DTILES; ++dt)
#pragma unroll
              for (int r = 0; r < 16; ++r) acc_o[dt][r] *= alpha;
          }

          // ---- P -> bf16 B-fragments, then PV ---------------------------
#pragma unroll
          for (int kslot = 0; kslot < 2; ++kslot) {
            const bf16x8v pf = repack_c_to_b(p, kslot);
            const int koff = (it * 32 + kslot * 16 + hi * 8) * 2;
#pragma unroll
            for (int dt = 0; dt < DTILES; ++dt) {
              const bf16x8v vf = *reinterpret_cast<const bf16x8v *>(
                  v_img + (dt * 32 + col) * V_STRIDE + koff);
              acc_o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                  vf, pf, acc_o[dt], 0, 0, 0);
            }
          }
        }
      }
    }
    __syncthreads();
  }

  return acc;
}

// Epilogue for a valid row: O^T regs -> out[0..DH), and the row's
// log-sum-exp to *lse unless lse is null.
template <int DH>
RB_DEV void flash_fwd_store(const FlashAcc<DH> &acc, uint16_t *out,
                            float *lse) {
  constexpr int DTILES = DH / 32;
  const int hi = (threadIdx.x & 63) >> 5;
  const float l_full = acc.l + __shfl_xor(acc.l, 32, 64);
  const float inv_l = (l_full > 0.0f) ? 1.0f / l_full : 0.0f;
  if (lse != nullptr && hi == 0)
    *lse = (l_full > 0.0f) ? acc.m + __logf(l_full) : -INFINITY;
#pragma unroll
  for (int dt = 0; dt < DTILES; ++dt) {
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      const int d0 = dt * 32 + 8 * rq + 4 * hi;
      uint16_t w[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        w[e] = f32_to_bf16(acc.o[dt][rq * 4 + e] * inv_l);
      *reinterpret_cast<uint2 *>(out + d0) =
          *reinterpret_cast<const uint2 *>(w);
    }
  }
}

// Host: runtime head dim -> template argument. f is a generic lambda called
// with std::integral_constant<int, DH>.
template <class F>
void flash_dispatch_dh(int64_t DH, const char *op, F &&f) {
  if (DH == 128) {
    f(std::integral_constant<int, 128>{});
  } else if (DH == 64) {
    f(std::integral_constant<int, 64>{});
  } else if (DH == 256) {
    f(std::integral_constant<int, 256>{});
  } else {
    TORCH_CHECK(false, op, ": DH must be 64, 128 or 256, got ", DH);
  }
}

}  // namespace rb
