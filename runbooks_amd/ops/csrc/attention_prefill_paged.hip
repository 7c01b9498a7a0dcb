// Flash-attention prefill over the PAGED KV cache (causal, GQA/MQA, bf16)
// for CDNA4 (gfx950).
//
// One sequence: T query rows at absolute positions [ctx_len, ctx_len + T)
// attend over keys [0, ctx_len + T), all of which already sit in the paged
// cache (the caller appended this chunk's k/v before the call). This is
// what lets a prefix-cache hit skip the cached part of a prompt and what
// lets a long prompt be prefilled in chunks (serve/engine.py).
//
// Geometry and arithmetic are those of flash_prefill_kernel
// (attention_prefill.hip), expression for expression: 8 waves x 32 query
// rows, 64-key LDS tiles aligned to absolute key 0 (= four 16-token cache
// blocks), K row-major + V^T images with the +16 B row pad, swapped QK^T,
// the same online softmax, permlane32_swap P repack, 32x32x16 bf16 PV. A
// row's result there depends only on the sequence of 32-key sub-tiles from
// key 0 (fully masked sub-tiles are exact no-ops: alpha == 1, p == 0), so
// this kernel is bit-identical to rows [ctx_len:] of flash_prefill on the
// concatenated sequence. Only the staging differs:
//  * K: 16 B loads from each block's contiguous [16][DH] rows.
//  * V, transposed-V blocks ([DH][16]): each d row is 32 contiguous bytes,
//    copied with two 16 B loads straight into the V^T image.
//  * V, plain blocks ([16][DH]): scalar transpose as in the dense kernel.
//  * the tile's four block ids are read once per tile; entries whose block
//    starts at or past ctx_len + T are never read, let alone dereferenced.
//  * keys >= ctx_len + T are zero-filled in LDS and never read from
//    memory: stale cache contents may be anything, and 0 x NaN in the PV
//    MFMA would poison the row.
//
// q, out: [T, Hq, DH] bf16. k_cache: [blk, Hkv, 16, DH]. v_cache: the same,
// or [blk, Hkv, DH, 16] (alloc_kv_cache v_transposed). DH in {64, 128, 256}.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

namespace {

constexpr int BLOCK = 512;   // 8 waves
constexpr int KVB = 64;      // keys per LDS tile
constexpr int CBS = 16;      // tokens per cache block
constexpr int TBLK = KVB / CBS;  // cache blocks per LDS tile

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

// bid[j] for a lane-varying j in 0..3 (register select, no indexed array)
RB_DEV int pick_block(const int (&bid)[TBLK], int j) {
  return j == 0 ? bid[0] : j == 1 ? bid[1] : j == 2 ? bid[2] : bid[3];
}

template <int DH, bool VT>
__global__ __launch_bounds__(BLOCK, 2) void flash_prefill_paged_kernel(
    const uint16_t *__restrict__ qp, const uint16_t *__restrict__ kcp,
    const uint16_t *__restrict__ vcp, const int *__restrict__ btp,
    uint16_t *__restrict__ op, int T, int ctx, int Hq, int Hkv, float scale) {
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

  const int S = ctx + T;                    // keys in the cache
  const int q0 = blockIdx.x * 256;          // first chunk row of this WG
  const int h = blockIdx.y;
  const int h_kv = h / (Hq / Hkv);
  const int crow = q0 + wid * 32 + col;     // this lane's row in the chunk
  const int qrow = ctx + crow;              // ... and its absolute position
  const bool q_valid = crow < T;

  // ---- Q fragments (B operand of swapped QK^T), pre-scaled --------------
  bf16x8v qf[KSTEPS];
  {
    const uint16_t *qrow_p =
        qp + ((int64_t)(q_valid ? crow : 0) * Hq + h) * DH;
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      const uint16_t *src = qrow_p + ks * 16 + hi * 8;
      float f[8];
      rb::VIO<uint16_t>::load(src, f);
      union { unsigned short u[8]; bf16x8v v; } c;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        c.u[e] = rb::f32_to_bf16(q_valid ? f[e] * scale : 0.0f);
      qf[ks] = c.v;
    }
  }

  f32x16v acc_o[DTILES];
#pragma unroll
  for (int dt = 0; dt < DTILES; ++dt) acc_o[dt] = (f32x16v)(0.0f);
  float m_run = -INFINITY;
  float l_run = 0.0f;

  const int kv_end = min(S, ctx + q0 + 256);  // causal upper bound for this WG
  const int n_tiles = (kv_end + KVB - 1) / KVB;
  const int wave_kmax = ctx + q0 + wid * 32 + 31;  // last key this wave can see

  // block bases in elements: a K block and a V block are both CBS*DH
  const int64_t blk_elems = (int64_t)Hkv * CBS * DH;
  const int64_t head_off = (int64_t)h_kv * CBS * DH;

  for (int kt = 0; kt < n_tiles; ++kt) {
    const int kbase = kt * KVB;

    // ---- the tile's cache blocks: one table read per tile -----------------
    // A block that starts at or past S holds no key this kernel reads; its
    // table entry may be anything, so it is not even loaded.
    int bid[TBLK];
#pragma unroll
    for (int j = 0; j < TBLK; ++j)
      bid[j] = (kbase + j * CBS < S) ? btp[kt * TBLK + j] : 0;

    // ---- stage K tile: [key][d] rows, each thread 16 B --------------------
    {
      const int per_pass = BLOCK * 8;       // elems per pass
      constexpr int total = KVB * DH;
#pragma unroll
      for (int p = 0; p < total / (BLOCK * 8); ++p) {
        const int idx = p * per_pass + tid * 8;
        const int key = idx / DH;
        const int d0 = idx % DH;
        const int gk = kbase + key;
        rb::bf16x8 val;
        if (gk < S) {
          const int64_t blk = pick_block(bid, key / CBS);
          val = *reinterpret_cast<const rb::bf16x8 *>(
              kcp + blk * blk_elems + head_off + (key % CBS) * DH + d0);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) val.v[e] = 0;
        }
        *reinterpret_cast<rb::bf16x8 *>(k_img + key * K_STRIDE + d0 * 2) = val;
      }
    }
    if constexpr (VT) {
      // ---- stage V^T from [DH][16] blocks: 16 B = 8 keys of one d row ----
      // chunk c: half = c & 1, d = (c >> 1) % DH, block = (c >> 1) / DH, so
      // consecutive lanes walk one block's DH*32 contiguous bytes.
      constexpr int CHUNKS = TBLK * DH * 2;
#pragma unroll
      for (int p = 0; p < CHUNKS / BLOCK; ++p) {
        const int c = p * BLOCK + tid;
        const int half = c & 1;
        const int d = (c >> 1) % DH;
        const int j = (c >> 1) / DH;
        const int key = j * CBS + half * 8;   // first key of the chunk
        const int gk = kbase + key;
        rb::bf16x8 val;
        if (gk < S) {
          const int64_t blk = pick_block(bid, j);
          val = *reinterpret_cast<const rb::bf16x8 *>(
              vcp + blk * blk_elems + head_off + d * CBS + half * 8);
          if (gk + 8 > S) {   // the block's tail past S: stale, zero it
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (gk + e >= S) val.v[e] = 0;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) val.v[e] = 0;
        }
        *reinterpret_cast<rb::bf16x8 *>(v_img + d * V_STRIDE + key * 2) = val;
      }
    } else {
      // ---- stage V tile transposed: thread owns column d, KPG keys -------
      constexpr int GRPS = BLOCK / DH;      // thread groups over keys
      constexpr int KPG = KVB / GRPS;       // keys per group (16 @DH=128)
      const int d = tid % DH;
      const int kg0 = (tid / DH) * KPG;
      // a run of SUB keys never straddles a cache block (SUB | 16 | kg0)
      constexpr int SUB = KPG < CBS ? KPG : CBS;
#pragma unroll
      for (int sb = 0; sb < KPG / SUB; ++sb) {
        const int key0 = kg0 + sb * SUB;
        const int64_t blk = pick_block(bid, key0 / CBS);
        const uint16_t *src =
            vcp + blk * blk_elems + head_off + (key0 % CBS) * DH + d;
        uint16_t tmp[SUB];
#pragma unroll
        for (int e = 0; e < SUB; ++e)
          tmp[e] = (kbase + key0 + e < S) ? src[e * DH] : (uint16_t)0;
#pragma unroll
        for (int c8 = 0; c8 < SUB / 8; ++c8)
          *reinterpret_cast<rb::bf16x8 *>(v_img + d * V_STRIDE + (key0 + c8 * 8) * 2) =
              *reinterpret_cast<rb::bf16x8 *>(&tmp[c8 * 8]);
      }
    }
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

          // ---- P -> bf16 B-fragments via permlane half-exchange ---------
#pragma unroll
          for (int kslot = 0; kslot < 2; ++kslot) {
            const int r0 = kslot * 8;
            unsigned pk0 = pack_bf16(p[r0 + 0], p[r0 + 1]);
            unsigned pk1 = pack_bf16(p[r0 + 2], p[r0 + 3]);
            unsigned pk2 = pack_bf16(p[r0 + 4], p[r0 + 5]);
            unsigned pk3 = pack_bf16(p[r0 + 6], p[r0 + 7]);
            auto r02 = __builtin_amdgcn_permlane32_swap(pk0, pk2, false, false);
            auto r13 = __builtin_amdgcn_permlane32_swap(pk1, pk3, false, false);
            const bf16x8v pf = frag_from_words(r02[0], r13[0], r02[1], r13[1]);
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

  // ---- epilogue: O^T regs -> out[crow, h, :] -------------------------------
  if (q_valid) {
    const float l_full = l_run + __shfl_xor(l_run, 32, 64);
    const float inv_l = (l_full > 0.0f) ? 1.0f / l_full : 0.0f;
    uint16_t *orow = op + ((int64_t)crow * Hq + h) * DH;
#pragma unroll
    for (int dt = 0; dt < DTILES; ++dt) {
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int d0 = dt * 32 + 8 * rq + 4 * hi;
        uint16_t w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          w[e] = rb::f32_to_bf16(acc_o[dt][rq * 4 + e] * inv_l);
        *reinterpret_cast<uint2 *>(orow + d0) =
            *reinterpret_cast<const uint2 *>(w);
      }
    }
  }
}

template <int DH, bool VT>
void launch_paged(const at::Tensor &q, const at::Tensor &kc,
                  const at::Tensor &vc, const at::Tensor &bt, at::Tensor &out,
                  int T, int ctx, int Hq, int Hkv, float scale) {
  constexpr size_t shmem = KVB * (DH * 2 + 16) + DH * (KVB * 2 + 16);
  const dim3 grid((T + 255) / 256, Hq);
  hipLaunchKernelGGL((flash_prefill_paged_kernel<DH, VT>), grid, dim3(BLOCK),
                     shmem, at::hip::getCurrentHIPStream(),
                     (const uint16_t *)q.data_ptr(),
                     (const uint16_t *)kc.data_ptr(),
                     (const uint16_t *)vc.data_ptr(),
                     (const int *)bt.data_ptr(), (uint16_t *)out.data_ptr(),
                     T, ctx, Hq, Hkv, scale);
}

}  // namespace

at::Tensor flash_prefill_paged(at::Tensor q, at::Tensor k_cache,
                               at::Tensor v_cache, at::Tensor block_table,
                               int64_t ctx_len, double scale) {
  TORCH_CHECK(k_cache.scalar_type() != at::kByte &&
                  v_cache.scalar_type() != at::kByte,
              "flash_prefill_paged: fp8 KV caches are not supported");
  TORCH_CHECK(q.is_cuda() && k_cache.is_cuda() && v_cache.is_cuda() &&
                  block_table.is_cuda(),
              "flash_prefill_paged: GPU tensors");
  TORCH_CHECK(q.is_contiguous() && k_cache.is_contiguous() &&
                  v_cache.is_contiguous() && block_table.is_contiguous(),
              "flash_prefill_paged: contiguous tensors");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16 &&
                  k_cache.scalar_type() == at::kBFloat16 &&
                  v_cache.scalar_type() == at::kBFloat16,
              "flash_prefill_paged: bf16 only");
  TORCH_CHECK(q.dim() == 3, "flash_prefill_paged: q must be [T, Hq, DH]");
  TORCH_CHECK(k_cache.dim() == 4 && v_cache.dim() == 4,
              "flash_prefill_paged: caches must be 4-d");
  TORCH_CHECK(block_table.scalar_type() == at::kInt && block_table.dim() == 1,
              "flash_prefill_paged: block_table must be int32 [n]");
  const int64_t T = q.size(0), Hq = q.size(1), DH = q.size(2);
  const int64_t Hkv = k_cache.size(1);
  TORCH_CHECK(T >= 1 && ctx_len >= 0, "flash_prefill_paged: T >= 1, ctx >= 0");
  TORCH_CHECK(ctx_len + T < (int64_t(1) << 30),
              "flash_prefill_paged: sequence too long");
  TORCH_CHECK(k_cache.size(2) == CBS && k_cache.size(3) == DH,
              "flash_prefill_paged: k_cache must be [blk, Hkv, 16, DH]");
  TORCH_CHECK(Hkv >= 1 && Hq % Hkv == 0, "flash_prefill_paged: Hq % Hkv");
  const bool vt = v_cache.size(2) == DH && v_cache.size(3) == CBS && DH != CBS;
  TORCH_CHECK(v_cache.size(0) == k_cache.size(0) && v_cache.size(1) == Hkv &&
                  (vt || (v_cache.size(2) == CBS && v_cache.size(3) == DH)),
              "flash_prefill_paged: v_cache must be [blk, Hkv, 16, DH] or "
              "[blk, Hkv, DH, 16]");
  TORCH_CHECK(block_table.numel() >= (ctx_len + T + CBS - 1) / CBS,
              "flash_prefill_paged: block_table shorter than ceil((ctx+T)/16)");
  auto out = at::empty_like(q);

#define RB_PAGED_LAUNCH(D)                                                    \
  if (vt)                                                                     \
    launch_paged<D, true>(q, k_cache, v_cache, block_table, out, (int)T,      \
                          (int)ctx_len, (int)Hq, (int)Hkv, (float)scale);     \
  else                                                                        \
    launch_paged<D, false>(q, k_cache, v_cache, block_table, out, (int)T,     \
                           (int)ctx_len, (int)Hq, (int)Hkv, (float)scale)
  if (DH == 128) {
    RB_PAGED_LAUNCH(128);
  } else if (DH == 64) {
    RB_PAGED_LAUNCH(64);
  } else if (DH == 256) {
    RB_PAGED_LAUNCH(256);
  } else {
    TORCH_CHECK(false, "flash_prefill_paged: DH must be 64, 128 or 256, got ",
                DH);
  }
#undef RB_PAGED_LAUNCH
  return out;
}
