// Flash-attention prefill over the PAGED KV cache (causal, GQA/MQA, bf16)
// for CDNA4 (gfx950).
//
// One sequence: T query rows at absolute positions [ctx_len, ctx_len + T)
// attend over keys [0, ctx_len + T), all of which already sit in the paged
// cache (the caller appended this chunk's k/v before the call). This is
// what lets a prefix-cache hit skip the cached part of a prompt and what
// lets a long prompt be prefilled in chunks (serve/engine.py).
// flash_prefill_paged_batch runs the same thing for several sequences'
// chunks packed into one token dimension, one launch for all of them.
//
// The kernel is flash_fwd_rows + flash_fwd_store (flash_fwd_core.h), the
// body of flash_prefill_kernel (attention_prefill.hip), fed by PagedKV
// below, so it is bit-identical to rows [ctx_len:] of flash_prefill on the
// concatenated sequence. This file owns the staging from the cache, the
// [T, Hq, DH] row mapping and the host checks. A 64-key LDS tile is four
// 16-token cache blocks:
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

#include "flash_fwd_core.h"

namespace {

constexpr int BLOCK = rb::FLASH_BLOCK;
constexpr int KVB = rb::FLASH_KVB;
constexpr int CBS = 16;      // tokens per cache block
constexpr int TBLK = KVB / CBS;  // cache blocks per LDS tile

// bid[j] for a lane-varying j in 0..3 (register select, no indexed array)
RB_DEV int pick_block(const int (&bid)[TBLK], int j) {
  return j == 0 ? bid[0] : j == 1 ? bid[1] : j == 2 ? bid[2] : bid[3];
}

// KV source: the cache blocks of one sequence, S keys, one kv head.
template <bool VT>
struct PagedKV {
  const uint16_t *__restrict__ kcp;
  const uint16_t *__restrict__ vcp;
  const int *__restrict__ btp;
  int S;
  // block bases in elements: a K block and a V block are both CBS*DH
  int64_t blk_elems;  // Hkv * CBS * DH
  int64_t head_off;   // h_kv * CBS * DH

  template <int DH>
  RB_DEV void stage(int kt, char *k_img, char *v_img) const {
    constexpr int K_STRIDE = DH * 2 + 16;
    constexpr int V_STRIDE = KVB * 2 + 16;
    const int tid = threadIdx.x;
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
  }
};

template <int DH, bool VT>
__global__ __launch_bounds__(BLOCK, 2) void flash_prefill_paged_kernel(
    const uint16_t *__restrict__ qp, const uint16_t *__restrict__ kcp,
    const uint16_t *__restrict__ vcp, const int *__restrict__ btp,
    uint16_t *__restrict__ op, int T, int ctx, int Hq, int Hkv, float scale) {
  const int S = ctx + T;                    // keys in the cache
  const int q0 = blockIdx.x * 256;          // first chunk row of this WG
  const int h = blockIdx.y;
  const int h_kv = h / (Hq / Hkv);
  // this lane's row in the chunk
  const int crow = q0 + (threadIdx.x >> 6) * 32 + (threadIdx.x & 31);
  const bool q_valid = crow < T;

  const auto acc = rb::flash_fwd_rows<DH>(
      qp + ((int64_t)(q_valid ? crow : 0) * Hq + h) * DH, ctx + crow, q_valid,
      S, ctx + q0,
      PagedKV<VT>{kcp, vcp, btp, S, (int64_t)Hkv * CBS * DH,
                  (int64_t)h_kv * CBS * DH},
      scale);
  if (q_valid)
    rb::flash_fwd_store<DH>(acc, op + ((int64_t)crow * Hq + h) * DH, nullptr);
}

// Several sequences' chunks packed into one token dimension ("varlen"): the
// grid's x is a list of 256-row tiles, each of ONE sequence, described by
// tile_seq / tile_row0. A tile is exactly a workgroup of
// flash_prefill_paged_kernel on that sequence alone (same rows, same row0,
// same KV source), so its rows are bit-identical to that kernel's.
//   cu_q     [B + 1]  sequence b owns packed rows [cu_q[b], cu_q[b+1])
//   ctx_lens [B]      keys cached before sequence b's chunk
//   btp      [B][maxb] block tables; row b is read below ceil(S_b/16) only
template <int DH, bool VT>
__global__ __launch_bounds__(BLOCK, 2) void flash_prefill_paged_batch_kernel(
    const uint16_t *__restrict__ qp, const uint16_t *__restrict__ kcp,
    const uint16_t *__restrict__ vcp, const int *__restrict__ btp,
    uint16_t *__restrict__ op, const int *__restrict__ cu_q,
    const int *__restrict__ ctx_lens, const int *__restrict__ tile_seq,
    const int *__restrict__ tile_row0, int maxb, int Hq, int Hkv,
    float scale) {
  const int b = tile_seq[blockIdx.x];
  const int q0 = tile_row0[blockIdx.x];     // first chunk row of this WG
  const int qbeg = cu_q[b];
  const int T = cu_q[b + 1] - qbeg;
  const int ctx = ctx_lens[b];
  const int S = ctx + T;                    // keys in the cache
  const int h = blockIdx.y;
  const int h_kv = h / (Hq / Hkv);
  // this lane's row in the sequence's chunk
  const int crow = q0 + (threadIdx.x >> 6) * 32 + (threadIdx.x & 31);
  const bool q_valid = crow < T;

  const auto acc = rb::flash_fwd_rows<DH>(
      qp + ((int64_t)(qbeg + (q_valid ? crow : 0)) * Hq + h) * DH, ctx + crow,
      q_valid, S, ctx + q0,
      PagedKV<VT>{kcp, vcp, btp + (int64_t)b * maxb, S,
                  (int64_t)Hkv * CBS * DH, (int64_t)h_kv * CBS * DH},
      scale);
  if (q_valid)
    rb::flash_fwd_store<DH>(
        acc, op + ((int64_t)(qbeg + crow) * Hq + h) * DH, nullptr);
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
  const dim3 grid((T + 255) / 256, Hq);

  rb::flash_dispatch_dh(DH, "flash_prefill_paged", [&](auto dh) {
    constexpr int D = decltype(dh)::value;
    auto kernel = vt ? flash_prefill_paged_kernel<D, true>
                     : flash_prefill_paged_kernel<D, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(BLOCK), rb::flash_fwd_smem<D>(),
                       at::hip::getCurrentHIPStream(),
                       (const uint16_t *)q.data_ptr(),
                       (const uint16_t *)k_cache.data_ptr(),
                       (const uint16_t *)v_cache.data_ptr(),
                       (const int *)block_table.data_ptr(),
                       (uint16_t *)out.data_ptr(), (int)T, (int)ctx_len,
                       (int)Hq, (int)Hkv, (float)scale);
  });
  return out;
}

// plan (int32, built by ops.paged_prefill_plan) is
//   [cu_q (B+1) | ctx_lens (B) | tile_seq (ntiles) | tile_row0 (ntiles)]
// plan_cpu is the host copy plan_dev was made from: every length is checked
// here against it and the tensor shapes, so the launch never waits for the
// device and an inconsistent call never reaches it.
at::Tensor flash_prefill_paged_batch(at::Tensor q, at::Tensor k_cache,
                                     at::Tensor v_cache,
                                     at::Tensor block_tables,
                                     at::Tensor plan_dev, at::Tensor plan_cpu,
                                     int64_t B, double scale) {
  const char *op = "flash_prefill_paged_batch";
  TORCH_CHECK(k_cache.scalar_type() != at::kByte &&
                  v_cache.scalar_type() != at::kByte,
              op, ": fp8 KV caches are not supported");
  TORCH_CHECK(q.is_cuda() && k_cache.is_cuda() && v_cache.is_cuda() &&
                  block_tables.is_cuda() && plan_dev.is_cuda(),
              op, ": GPU tensors");
  TORCH_CHECK(k_cache.device() == q.device() &&
                  v_cache.device() == q.device() &&
                  block_tables.device() == q.device() &&
                  plan_dev.device() == q.device(),
              op, ": all tensors on q's device");
  TORCH_CHECK(q.is_contiguous() && k_cache.is_contiguous() &&
                  v_cache.is_contiguous() && block_tables.is_contiguous() &&
                  plan_dev.is_contiguous() && plan_cpu.is_contiguous(),
              op, ": contiguous tensors");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16 &&
                  k_cache.scalar_type() == at::kBFloat16 &&
                  v_cache.scalar_type() == at::kBFloat16,
              op, ": bf16 only");
  TORCH_CHECK(q.dim() == 3, op, ": q must be [Ttot, Hq, DH]");
  TORCH_CHECK(k_cache.dim() == 4 && v_cache.dim() == 4,
              op, ": caches must be 4-d");
  TORCH_CHECK(block_tables.scalar_type() == at::kInt &&
                  block_tables.dim() == 2,
              op, ": block_tables must be int32 [B, maxb]");
  TORCH_CHECK(plan_cpu.is_cpu() && plan_cpu.scalar_type() == at::kInt &&
                  plan_dev.scalar_type() == at::kInt && plan_cpu.dim() == 1 &&
                  plan_dev.dim() == 1 && plan_dev.numel() == plan_cpu.numel(),
              op, ": plan must be int32 [n] on the host and the device");
  TORCH_CHECK(B >= 1 && B < (int64_t(1) << 20), op, ": B out of range");
  TORCH_CHECK(block_tables.size(0) == B,
              op, ": block_tables has ", block_tables.size(0),
              " rows, the plan ", B, " sequences");
  const int64_t n_plan = plan_cpu.numel();
  TORCH_CHECK(n_plan >= 2 * B + 1 && (n_plan - 2 * B - 1) % 2 == 0,
              op, ": malformed plan");
  const int64_t ntiles = (n_plan - 2 * B - 1) / 2;
  const int *pl = plan_cpu.data_ptr<int>();
  const int *cu = pl, *cx = pl + B + 1, *ts = cx + B, *tr = ts + ntiles;

  const int64_t Ttot = q.size(0), Hq = q.size(1), DH = q.size(2);
  const int64_t Hkv = k_cache.size(1);
  const int64_t maxb = block_tables.size(1);
  TORCH_CHECK(cu[0] == 0, op, ": malformed plan");
  int64_t tile = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t T = (int64_t)cu[b + 1] - cu[b], ctx = cx[b];
    TORCH_CHECK(T >= 1 && ctx >= 0, op, ": T_b >= 1, ctx_b >= 0 (sequence ",
                b, ": T ", T, ", ctx ", ctx, ")");
    TORCH_CHECK(ctx + T < (int64_t(1) << 30), op, ": sequence too long");
    TORCH_CHECK(maxb >= (ctx + T + CBS - 1) / CBS,
                op, ": block_tables narrower than ceil((ctx+T)/16) of "
                "sequence ", b);
    for (int64_t r0 = 0; r0 < T; r0 += 256, ++tile)
      TORCH_CHECK(tile < ntiles && ts[tile] == b && tr[tile] == r0,
                  op, ": malformed plan (tiles)");
  }
  TORCH_CHECK(tile == ntiles, op, ": malformed plan (tiles)");
  TORCH_CHECK(Ttot == cu[B], op, ": q has ", Ttot, " rows, the plan ", cu[B]);
  TORCH_CHECK(Ttot < (int64_t(1) << 30), op, ": too many packed rows");
  TORCH_CHECK(k_cache.size(2) == CBS && k_cache.size(3) == DH,
              op, ": k_cache must be [blk, Hkv, 16, DH]");
  TORCH_CHECK(Hkv >= 1 && Hq % Hkv == 0, op, ": Hq % Hkv");
  TORCH_CHECK(Hq <= 65535, op, ": too many heads");
  const bool vt = v_cache.size(2) == DH && v_cache.size(3) == CBS && DH != CBS;
  TORCH_CHECK(v_cache.size(0) == k_cache.size(0) && v_cache.size(1) == Hkv &&
                  (vt || (v_cache.size(2) == CBS && v_cache.size(3) == DH)),
              op, ": v_cache must be [blk, Hkv, 16, DH] or [blk, Hkv, DH, 16]");
  auto out = at::empty_like(q);
  const dim3 grid(ntiles, Hq);
  const int *pd = (const int *)plan_dev.data_ptr();

  rb::flash_dispatch_dh(DH, op, [&](auto dh) {
    constexpr int D = decltype(dh)::value;
    auto kernel = vt ? flash_prefill_paged_batch_kernel<D, true>
                     : flash_prefill_paged_batch_kernel<D, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(BLOCK), rb::flash_fwd_smem<D>(),
                       at::hip::getCurrentHIPStream(),
                       (const uint16_t *)q.data_ptr(),
                       (const uint16_t *)k_cache.data_ptr(),
                       (const uint16_t *)v_cache.data_ptr(),
                       (const int *)block_tables.data_ptr(),
                       (uint16_t *)out.data_ptr(), pd, pd + (B + 1),
                       pd + (2 * B + 1), pd + (2 * B + 1 + ntiles), (int)maxb,
                       (int)Hq, (int)Hkv, (float)scale);
  });
  return out;
}
