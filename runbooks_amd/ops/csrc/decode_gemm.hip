// Decode GEMM v2 for CDNA4 (gfx950): y[M,N] = x[M,K] @ W[N,K]^T,
// M <= 32 (decode batch), bf16 in / bf16 out, fp32 accumulate.
//
// The M<=32 decode GEMM is >99% W traffic, so the ONLY thing that
// matters is shaping the weight read as perfectly coalesced nontemporal
// bursts with enough in flight (MI355X ~6.3 TB/s achievable; hipBLASLt
// measured ~2.4 TB/s in the round-1 decode loop, and a fragment-shaped
// direct-load variant measured ~1.5 TB/s because every wave instruction
// became 32 scattered 32 B requests). This version therefore streams
// BOTH operands from layouts pre-swizzled into MFMA fragment-lane order:
//
//  * W is stored fragment-major at model-load time (decode_swizzle_w:
//    [N/32][K/16][lane][8] bf16) so each wave instruction is one 1 KiB
//    contiguous nontemporal read. 288 GB HBM3E per GPU makes the second
//    weight copy the right trade (same pattern as the fp8 registry);
//    prefill/training keep using the original [N,K] tensor via hipBLASLt.
//  * x (tiny: M*K <= 0.7 MB) is swizzled per call by decode_swizzle_x —
//    one extra ~microsecond kernel — into [K/16][lane][8] with zero
//    padding for m >= M; after that every wave reads the same contiguous
//    L2-resident stream.
//  * One wave owns 32 W rows x a DEEP contiguous k-range (K/(4*SPLIT)),
//    no LDS and no barrier in the main loop (hipcc pipelines the 2x8
//    ping-pong register ring freely; ~16 KB in flight per wave vs the
//    ~9 KB/CU Little's-law requirement at 24.6 GB/s/CU).
//  * 4 waves per WG take adjacent k-quarters; one 16 KB LDS reduction
//    combines them. SPLIT (1 for N>=16k, 2-4 for N=4096 shapes) adds
//    fp32 slabs [SPLIT,M,N] reduced by a combine kernel (~1 MB next to
//    the 32-90 MB W stream).
//
// Fragment maps (v_mfma_f32_32x32x16_bf16, A=W so C cols = m):
//   A lane l -> A[row=l&31][k=(l>>5)*8+i];  B lane l -> B[k][col=l&31];
//   C lane l -> C[row=(r&3)+8*(r>>2)+4*(l>>5)][col=l&31], r = 0..15.
// The swizzles bake exactly these maps into the storage order.
//
// Reference parity: replaces hipBLASLt for the decode hot loop the way
// the reference's external server image leans on cuBLAS
// (substratusai/runbooks docs/container-contract.md serving contract).

#include <stdlib.h>

#include <algorithm>

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

namespace {

constexpr int BLOCK = 256;   // 4 waves
constexpr int MMAX = 32;

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

// the 4-wave sum, rounded to bf16 exactly as the y store rounds it
#define RB_RED_BF16(ROW, M_)                                           \
  rb::f32_to_bf16(red[0][ROW][M_] + red[1][ROW][M_] + red[2][ROW][M_] + \
                  red[3][ROW][M_])

// One chunk of U k-steps. W nontemporal (streamed once, must not evict
// L2); x plain (re-read by every n-block: L2 is exactly where it wants
// to live). Both streams are lane*16B contiguous per instruction.
#define RB_LOAD_CHUNK(WB, XB, SBASE)                                   \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                      \
    WB[u] = nt_load8v(wseg + (int64_t)((SBASE) + u) * 512 + lane8);    \
    XB[u] = load8v(xs + (int64_t)((SBASE) + u) * 512 + lane8);         \
  }

#define RB_MFMA_CHUNK(WB, XB)                                          \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                      \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(WB[u], XB[u], acc,   \
                                                  0, 0, 0);            \
  }

// A tail chunk: the same U loads with the step index clamped to SLAST, the
// wave's last real step, so the load count stays static (counted vmcnt
// waits) and nothing outside the wave's own [s0, s1) is read; the repeats
// re-request one 1 KiB line. Only the first CNT registers are consumed.
#define RB_LOAD_CHUNK_CLAMP(WB, XB, SBASE, SLAST)                      \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                      \
    const int sc = min((SBASE) + u, (SLAST));                          \
    WB[u] = nt_load8v(wseg + (int64_t)sc * 512 + lane8);               \
    XB[u] = load8v(xs + (int64_t)sc * 512 + lane8);                    \
  }

// The first CNT (wave-uniform, <= U) k-steps of a chunk, in order. A step
// that does not exist is branched over, never fed a zero operand: adding
// +0 could turn a -0 sum into +0.
#define RB_MFMA_HEAD(WB, XB, CNT)                                      \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                      \
    if (u < (CNT)) {                                                   \
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(WB[u], XB[u], acc, \
                                                    0, 0, 0);          \
    }                                                                  \
  }

// STORE_BF16: write y bf16 directly (SPLIT == 1). Otherwise store an
// fp32 slab slice at slabs + kslice*M*N for decode_gemm_combine.
// U = k-steps (of 16) per unrolled chunk: 8 keeps 3 waves/SIMD, 12
// trades occupancy (2/SIMD) for a deeper in-flight ring (RB_DG_U=12).
// RING_TAIL: the t = (s1 - s0) % 2U steps the ring pairs leave over go
// through the ring as up to two clamped chunks, all their loads in flight
// at once (chunk 1 issued under the last B chunk's MFMAs). false keeps
// the one-step-at-a-time loop (tail = 0 / RB_DG_TAIL=0, for A/B runs and
// bisecting). Both run the same k-steps in the same order into the same
// accumulator, so the outputs are bit-identical.
template <bool STORE_BF16, int U = 8, int EPI = EPI_PLAIN,
          bool RING_TAIL = true>
__global__ __launch_bounds__(BLOCK, (RING_TAIL && U == 8) ? 3 : 1) void
decode_gemm_kernel(
    const uint16_t *__restrict__ xs, const uint16_t *__restrict__ ws,
    uint16_t *__restrict__ yp, float *__restrict__ slabs,
    int M, int N, int K, const EpiArgs ep) {
  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int hi = lane >> 5;
  const int col = lane & 31;
  const int lane8 = lane * 8;

  const int nblk = blockIdx.x;           // 32 W rows per WG
  const int kslice = blockIdx.y;
  const int split = gridDim.y;

  // k-step range (steps of 16) for this (kslice, wave) group; contiguous
  // per group so the W stream is one long sequential burst.
  const int steps_total = K / 16;
  const int ngroups = split * 4;
  const int spg = (steps_total + ngroups - 1) / ngroups;
  // The ring tail branches on its step counts and clamps step indices:
  // tell the compiler the wave index is uniform, so those are scalar
  // branches and scalar address arithmetic (the old tail keeps its code).
  const int g = kslice * 4 +
                (RING_TAIL ? __builtin_amdgcn_readfirstlane(wid) : wid);
  const int s0 = g * spg;
  const int s1 = min(steps_total, s0 + spg);

  const uint16_t *wseg = ws + (int64_t)nblk * steps_total * 512;

  // rope16 epilogue operands (slot, cos/sin of this thread's two pairs)
  // depend on nothing the GEMM computes: issue their loads now, so the
  // pos -> table dependent-load chain hides under the weight stream
  // instead of sitting on every workgroup's tail.
  int rp_slot = 0;
  float2 rp_c = make_float2(0.0f, 0.0f), rp_s = rp_c;
  if constexpr (EPI == EPI_ROPE || EPI == EPI_ROPE_VT) {
    const int em = tid >> 3;
    if (em < M) {
      rp_slot = ep.slots[em];
      if (nblk / (ep.dh / 32) < ep.hq + ep.hkv) {
        const int64_t toff = (int64_t)ep.pos[em] * (ep.dh / 2) +
                             16 * (nblk % (ep.dh / 32)) + (tid & 7) * 2;
        rp_c = *reinterpret_cast<const float2 *>(ep.cs + toff);
        rp_s = *reinterpret_cast<const float2 *>(ep.sn + toff);
      }
    }
  }

  f32x16v acc = (f32x16v)(0.0f);

  bf16x8v wA[U], xA[U], wB[U], xB[U];
  int s = s0;
  const int nmain = ((s1 - s0) / (2 * U)) * (2 * U);
  if constexpr (RING_TAIL) {
    const int smain = s0 + max(nmain, 0);
    const int t1 = min(s1 - smain, U);   // tail chunk 1: 0..U steps
    const int t2 = s1 - smain - U;       // tail chunk 2: > 0 when it exists
    const int slast = s1 - 1;
    if (nmain > 0) {
      RB_LOAD_CHUNK(wA, xA, s);
      for (; s + 2 * U < smain; s += 2 * U) {
        RB_LOAD_CHUNK(wB, xB, s + U);
        RB_MFMA_CHUNK(wA, xA);
        RB_LOAD_CHUNK(wA, xA, s + 2 * U);
        RB_MFMA_CHUNK(wB, xB);
      }
      // last pair: the A half it frees takes tail chunk 1, whose loads
      // fly under the B chunk's MFMAs
      RB_LOAD_CHUNK(wB, xB, s + U);
      RB_MFMA_CHUNK(wA, xA);
      if (t1 > 0) {
        RB_LOAD_CHUNK_CLAMP(wA, xA, smain, slast);
        RB_MFMA_CHUNK(wB, xB);
        if (t2 > 0) {
          RB_LOAD_CHUNK_CLAMP(wB, xB, smain + U, slast);
          RB_MFMA_HEAD(wA, xA, t1);
          RB_MFMA_HEAD(wB, xB, t2);
        } else {
          RB_MFMA_HEAD(wA, xA, t1);
        }
      } else {
        RB_MFMA_CHUNK(wB, xB);
      }
    } else if (t1 > 0) {                 // the whole range is tail
      RB_LOAD_CHUNK_CLAMP(wA, xA, s0, slast);
      if (t2 > 0) {
        RB_LOAD_CHUNK_CLAMP(wB, xB, s0 + U, slast);
        RB_MFMA_HEAD(wA, xA, t1);
        RB_MFMA_HEAD(wB, xB, t2);
      } else {
        RB_MFMA_HEAD(wA, xA, t1);
      }
    }
  } else {
    if (nmain > 0) {
      RB_LOAD_CHUNK(wA, xA, s);
      const int smain = s0 + nmain;
      for (; s + 2 * U <= smain; s += 2 * U) {
        if (s + U < smain) { RB_LOAD_CHUNK(wB, xB, s + U); }
        RB_MFMA_CHUNK(wA, xA);
        if (s + 2 * U < smain) { RB_LOAD_CHUNK(wA, xA, s + 2 * U); }
        if (s + U < smain) { RB_MFMA_CHUNK(wB, xB); }
      }
    }
    // tail: single k-steps, no prefetch (<= 2U-1 iterations)
    for (; s < s1; ++s) {
      bf16x8v w1 = nt_load8v(wseg + (int64_t)s * 512 + lane8);
      bf16x8v x1 = load8v(xs + (int64_t)s * 512 + lane8);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, x1, acc, 0, 0, 0);
    }
  }

  // ---- cross-wave reduction in LDS -------------------------------------
  __shared__ __attribute__((aligned(16))) float red[4][32][MMAX];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n_local = (r & 3) + 8 * (r >> 2) + 4 * hi;
    red[wid][n_local][col] = acc[r];
  }
  __syncthreads();

  if constexpr (EPI == EPI_SWIGLU || EPI == EPI_GEGLU) {
    // glu16 block -> k-step nblk of the down-proj operand: wave 0 writes
    // the 1 KiB chunk [lane = hi*32 + m][8], act(gate) * up of columns
    // 16*nblk + hi*8 + i. Rows m >= M stay unwritten (dropped downstream).
    const int m = tid & 31;
    if (tid < 64 && m < M) {
      const int r0 = (tid >> 5) * 8;
      union { uint16_t u[8]; u32x4v q; } o;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float gv = rb::bf16_to_f32(RB_RED_BF16(r0 + i, m));
        const float uv = rb::bf16_to_f32(RB_RED_BF16(16 + r0 + i, m));
        o.u[i] = rb::f32_to_bf16(EPI == EPI_GEGLU ? rb::gelu_tanh_mul(gv, uv)
                                                  : rb::silu_mul(gv, uv));
      }
      *reinterpret_cast<u32x4v *>(ep.swz + (int64_t)nblk * 512 + tid * 8) =
          o.q;
    }
    return;
  } else if constexpr (EPI == EPI_ROPE || EPI == EPI_ROPE_VT) {
    // rope16 block: uniformly a q, k or v block (head = nblk*32/Dh).
    const int em = tid >> 3;             // 0..31
    const int sub = tid & 7;
    if (em >= M) return;
    const int bph = ep.dh / 32;
    const int head = nblk / bph;
    const int j = nblk - head * bph;
    if (head < ep.hq + ep.hkv) {         // ---- q / k: 2 rotate-half pairs
      const int half = ep.dh / 2;
      const int p = sub * 2;
      const int d = 16 * j + p;
      uint16_t *dst;
      if (head < ep.hq) {
        dst = ep.q_out + ((int64_t)em * ep.hq + head) * ep.dh + d;
      } else {
        const int slot = rp_slot;
        if (slot < 0) return;
        dst = ep.k_cache +
              ((((int64_t)(slot / ep.bs) * ep.hkv + (head - ep.hq)) * ep.bs +
                slot % ep.bs) * ep.dh) + d;
      }
      const float2 c = rp_c, sn = rp_s;
      const float a0 = rb::bf16_to_f32(RB_RED_BF16(p, em));
      const float a1 = rb::bf16_to_f32(RB_RED_BF16(p + 1, em));
      const float b0 = rb::bf16_to_f32(RB_RED_BF16(16 + p, em));
      const float b1 = rb::bf16_to_f32(RB_RED_BF16(17 + p, em));
      float x0, y0, x1, y1;
      rb::rope_rot(a0, b0, c.x, sn.x, x0, y0);
      rb::rope_rot(a1, b1, c.y, sn.y, x1, y1);
      *reinterpret_cast<uint32_t *>(dst) =
          (uint32_t)rb::f32_to_bf16(x0) | ((uint32_t)rb::f32_to_bf16(x1) << 16);
      *reinterpret_cast<uint32_t *>(dst + half) =
          (uint32_t)rb::f32_to_bf16(y0) | ((uint32_t)rb::f32_to_bf16(y1) << 16);
    } else {                             // ---- v: copy into the cache
      const int slot = rp_slot;
      if (slot < 0) return;
      const int hv = head - ep.hq - ep.hkv;
      const int en = sub * 4;
      const int d = 32 * j + en;
      union { uint16_t u[4]; uint64_t q; } o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o.u[i] = RB_RED_BF16(en + i, em);
      if constexpr (EPI == EPI_ROPE_VT) {
        const int64_t vbase =
            ((int64_t)(slot / ep.bs) * ep.hkv + hv) * (int64_t)ep.dh * ep.bs;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          ep.v_cache[vbase + (int64_t)(d + i) * ep.bs + slot % ep.bs] = o.u[i];
      } else {
        *reinterpret_cast<uint64_t *>(
            ep.v_cache +
            ((((int64_t)(slot / ep.bs) * ep.hkv + hv) * ep.bs + slot % ep.bs) *
             ep.dh) + d) = o.q;
      }
    }
    return;
  }

  // 1024 outputs, 4 per thread, n fastest so bf16 stores coalesce 8 B.
  const int em = tid >> 3;               // 0..31
  const int en = (tid & 7) * 4;          // 0,4,..,28
  if (em < M) {
    float sum[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sum[j] = red[0][en + j][em] + red[1][en + j][em] +
               red[2][en + j][em] + red[3][en + j][em];
    }
    if (STORE_BF16) {
      union { uint16_t u[4]; uint64_t q; } o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o.u[j] = rb::f32_to_bf16(sum[j]);
      *reinterpret_cast<uint64_t *>(
          yp + (int64_t)em * N + epi_col<EPI>(nblk, en, ep)) = o.q;
    } else {
      float *slab = slabs + ((int64_t)kslice * M + em) * N +
                    epi_col<EPI>(nblk, en, ep);
      *reinterpret_cast<float4 *>(slab) =
          make_float4(sum[0], sum[1], sum[2], sum[3]);
    }
  }
}

// slabs [SPLIT, M, N] f32 -> y [M, N] bf16
__global__ void decode_gemm_combine_kernel(
    const float *__restrict__ slabs, uint16_t *__restrict__ yp,
    int split, int64_t mn) {
  const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
  for (int64_t i = i0; i < mn; i += stride) {
    float4 s = *reinterpret_cast<const float4 *>(slabs + i);
    for (int k = 1; k < split; ++k) {
      float4 t = *reinterpret_cast<const float4 *>(slabs + (int64_t)k * mn + i);
      s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    union { uint16_t u[4]; uint64_t q; } o;
    o.u[0] = rb::f32_to_bf16(s.x); o.u[1] = rb::f32_to_bf16(s.y);
    o.u[2] = rb::f32_to_bf16(s.z); o.u[3] = rb::f32_to_bf16(s.w);
    *reinterpret_cast<uint64_t *>(yp + i) = o.q;
  }
}

// x [M, K] row-major -> xs [K/16][64 lanes][8] bf16 (B-fragment lane
// order: lane = hi*32 + m, elems = x[m][s*16 + hi*8 + i]; zeros for
// m >= M). One scattered read pass of <= 0.7 MB, coalesced writes.
__global__ void decode_swizzle_x_kernel(
    const uint16_t *__restrict__ xp, uint16_t *__restrict__ xs,
    int M, int K) {
  const int steps = K / 16;
  const int64_t total = (int64_t)steps * 64;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += stride) {
    const int s = (int)(idx >> 6);
    const int l = (int)(idx & 63);
    const int m = l & 31;
    const int hi = l >> 5;
    rb::bf16x8 v;
    if (m < M) {
      v = *reinterpret_cast<const rb::bf16x8 *>(
          xp + (int64_t)m * K + s * 16 + hi * 8);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v.v[e] = 0;
    }
    *reinterpret_cast<rb::bf16x8 *>(xs + idx * 8) = v;
  }
}

}  // namespace

// Pick the cross-WG k-split by LOAD BALANCE: the kernel is a pure
// weight stream, so wall time = (WG waves over the 256 CUs) = ceil(
// nWG/256) rounds, and utilization = nWG / (256 * rounds). Measured
// r5 microbench tracks this exactly: 384 WGs -> 75% -> 4.2 TB/s,
// 688 -> 90% -> 4.7, 1000 -> 98% -> 5.2. Score each legal split and
// keep the best; ties go to fewer splits (a split adds a slab round
// trip + combine kernel ~5-6 us inside the captured graph).
int64_t decode_gemm_split(int64_t N, int64_t K) {
  // Split only when the grid cannot cover the 256 CUs (o_proj/down_proj
  // N=4096 -> 128 WGs). Measured r5/r6: splitting an already-covering
  // grid loses (gateup 688 WGs split 4: -10%; qkv 384 split 2 gained
  // ~2% on the kernel but pays a combine launch inside the graph).
  const int64_t nblocks = N / 32;
  int64_t split = 1;
  while (split < 8 && nblocks * split < 256 &&
         (K / 16) % (split * 4) == 0 && K / (split * 2) >= 1024) {
    split *= 2;
  }
  return split;
}

bool decode_gemm_supported(int64_t M, int64_t N, int64_t K) {
  return M >= 1 && M <= MMAX && N % 32 == 0 && K % 16 == 0 && K >= 1024;
}

// One-time weight swizzle (host-side tensor ops): [N,K] ->
// [N/32][K/16][2][32][8] = fragment-lane-major chunks of 1 KiB.
at::Tensor decode_swizzle_w(at::Tensor w) {
  TORCH_CHECK(w.dim() == 2 && w.scalar_type() == at::kBFloat16 &&
              w.is_contiguous(), "decode_swizzle_w: contiguous bf16 [N,K]");
  const int64_t N = w.size(0), K = w.size(1);
  TORCH_CHECK(N % 32 == 0 && K % 16 == 0, "decode_swizzle_w: shape");
  return w.view({N / 32, 32, K / 16, 2, 8})
      .permute({0, 2, 3, 1, 4}).contiguous();
}

at::Tensor decode_swizzle_x(at::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous() &&
              x.scalar_type() == at::kBFloat16, "decode_swizzle_x: x");
  const int M = x.size(0), K = x.size(1);
  TORCH_CHECK(M <= MMAX && K % 16 == 0, "decode_swizzle_x: shape");
  auto xs = at::empty({(int64_t)(K / 16) * 512}, x.options());
  auto stream = at::cuda::getCurrentHIPStream();
  const int grid = rb::rb_grid_1d((int64_t)(K / 16) * 64, 256);
  hipLaunchKernelGGL(decode_swizzle_x_kernel, dim3(grid), dim3(256), 0,
                     stream, (const uint16_t *)x.data_ptr(),
                     (uint16_t *)xs.data_ptr(), M, K);
  return xs;
}

static int dg_u() {
  static int u = [] {
    const char *e = getenv("RB_DG_U");
    return (e != nullptr && atoi(e) == 12) ? 12 : 8;
  }();
  return u;
}

// RB_DG_TAIL=0 (exactly "0"; anything else keeps the default): the
// one-step-at-a-time K tail (see RING_TAIL) for the raw, glu and rope entry
// points and for the tail = -1 default of decode_gemm / decode_gemm_w4.
// Read once.
bool rb::dg_ring_tail() {
  static bool t = [] {
    const char *e = getenv("RB_DG_TAIL");
    return !(e != nullptr && e[0] == '0' && e[1] == '\0');
  }();
  return t;
}

namespace {

template <bool STORE_BF16, int U, int EPI>
void launch_dg_u(bool ring_tail, const dim3 &grid, hipStream_t stream,
                 const at::Tensor &xs, const at::Tensor &ws, uint16_t *y,
                 float *slabs, int64_t M, int64_t N, int64_t K,
                 const EpiArgs &ep) {
  if (ring_tail)
    hipLaunchKernelGGL((decode_gemm_kernel<STORE_BF16, U, EPI, true>), grid,
                       dim3(BLOCK), 0, stream,
                       (const uint16_t *)xs.data_ptr(),
                       (const uint16_t *)ws.data_ptr(), y, slabs,
                       (int)M, (int)N, (int)K, ep);
  else
    hipLaunchKernelGGL((decode_gemm_kernel<STORE_BF16, U, EPI, false>), grid,
                       dim3(BLOCK), 0, stream,
                       (const uint16_t *)xs.data_ptr(),
                       (const uint16_t *)ws.data_ptr(), y, slabs,
                       (int)M, (int)N, (int)K, ep);
}

// Does any (kslice, wave) group of this launch have a K tail, i.e. a step
// count that is no multiple of the ring pair 2U? The kernel's partition.
bool dg_has_tail(int64_t K, int split, int u) {
  const int steps_total = (int)(K / 16), ngroups = split * 4;
  const int spg = (steps_total + ngroups - 1) / ngroups;
  for (int g = 0; g < ngroups; ++g) {
    const int n = std::min(steps_total, g * spg + spg) - g * spg;
    if (n > 0 && n % (2 * u) != 0) return true;
  }
  return false;
}

// The ring-tail instantiation is launched only where some wave has a tail:
// a launch without one (qkv, gate-up, o_proj, lm_head at U = 8) keeps the
// kernel, and so the main-loop schedule, it had before the ring tail.
template <bool STORE_BF16, int EPI>
void launch_dg(int u, bool ring_tail, int split, hipStream_t stream,
               const at::Tensor &xs, const at::Tensor &ws, uint16_t *y,
               float *slabs, int64_t M, int64_t N, int64_t K,
               const EpiArgs &ep) {
  const dim3 grid(N / 32, split);
  ring_tail = ring_tail && dg_has_tail(K, split, u == 12 ? 12 : 8);
  if (u == 12)
    launch_dg_u<STORE_BF16, 12, EPI>(ring_tail, grid, stream, xs, ws, y,
                                     slabs, M, N, K, ep);
  else
    launch_dg_u<STORE_BF16, 8, EPI>(ring_tail, grid, stream, xs, ws, y,
                                    slabs, M, N, K, ep);
}

// un-permuting (or plain) store, by layout tag
template <bool STORE_BF16>
void launch_dg_store(int64_t layout, int u, bool ring_tail, int split,
                     hipStream_t stream, const at::Tensor &xs,
                     const at::Tensor &ws, uint16_t *y, float *slabs,
                     int64_t M, int64_t N, int64_t K, const EpiArgs &ep) {
  if (layout == LAYOUT_GLU16)
    launch_dg<STORE_BF16, EPI_GLU_STORE>(u, ring_tail, split, stream, xs, ws,
                                         y, slabs, M, N, K, ep);
  else if (layout == LAYOUT_ROPE16)
    launch_dg<STORE_BF16, EPI_ROPE_STORE>(u, ring_tail, split, stream, xs, ws,
                                          y, slabs, M, N, K, ep);
  else
    launch_dg<STORE_BF16, EPI_PLAIN>(u, ring_tail, split, stream, xs, ws, y,
                                     slabs, M, N, K, ep);
}

EpiArgs layout_args(int64_t layout, int64_t N, int64_t hq, int64_t hkv,
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

void check_operands(const at::Tensor &xs, const at::Tensor &ws, int64_t M,
                    int64_t N, int64_t K, const char *who) {
  TORCH_CHECK(xs.is_cuda() && ws.is_cuda() && xs.is_contiguous() &&
              ws.is_contiguous() && xs.scalar_type() == at::kBFloat16 &&
              ws.scalar_type() == at::kBFloat16, who, ": inputs");
  TORCH_CHECK(xs.numel() == (K / 16) * 512 && ws.numel() == N * K &&
              decode_gemm_supported(M, N, K), who, ": shape");
}

}  // namespace

// One-time permuted weight swizzle for a layout tag: row r of the
// permuted matrix is row perm[r] of w, built from the same block rules
// the kernel's epilogues invert (LAYOUT_* above).
at::Tensor decode_swizzle_w_layout(at::Tensor w, int64_t layout, int64_t hq,
                                   int64_t hkv, int64_t dh) {
  TORCH_CHECK(w.dim() == 2, "decode_swizzle_w_layout: [N,K]");
  const int64_t N = w.size(0);
  layout_args(layout, N, hq, hkv, dh);
  if (layout == LAYOUT_PLAIN) return decode_swizzle_w(w);
  auto perm = at::empty({N}, at::TensorOptions().dtype(at::kLong));
  int64_t *p = perm.data_ptr<int64_t>();
  for (int64_t r = 0; r < N; ++r) {
    const int64_t b = r / 32, l = r % 32;
    if (layout == LAYOUT_GLU16) {
      p[r] = (l < 16 ? 0 : N / 2 - 16) + 16 * b + l;
    } else {
      const int64_t bph = dh / 32, head = b / bph, j = b % bph;
      p[r] = head >= hq + hkv
                 ? r
                 : head * dh + 16 * j + (l & 15) + (l < 16 ? 0 : dh / 2);
    }
  }
  return decode_swizzle_w(w.index_select(0, perm.to(w.device())));
}

// Raw variant for fused consumers: split == 1 returns y bf16 [M, N];
// split > 1 returns the fp32 slab [split, M, N] UNCOMBINED — the
// consumer kernel (rmsnorm_res_slab_fwd_dec) folds the slices while it
// reads, saving the combine launch inside the decode graph.
at::Tensor decode_gemm_raw(at::Tensor xs, at::Tensor ws, int64_t M,
                           int64_t N, int64_t K, int64_t layout, int64_t hq,
                           int64_t hkv, int64_t dh) {
  check_operands(xs, ws, M, N, K, "decode_gemm_raw");
  const EpiArgs ep = layout_args(layout, N, hq, hkv, dh);
  auto stream = at::cuda::getCurrentHIPStream();
  const int split = (int)decode_gemm_split(N, K);
  if (split == 1) {
    auto y = at::empty({M, N}, xs.options());
    launch_dg_store<true>(layout, dg_u(), rb::dg_ring_tail(), 1, stream, xs, ws,
                          (uint16_t *)y.data_ptr(), nullptr, M, N, K, ep);
    return y;
  }
  auto slabs = at::empty({split, M, N}, xs.options().dtype(at::kFloat));
  launch_dg_store<false>(layout, dg_u(), rb::dg_ring_tail(), split, stream,
                         xs, ws, nullptr, (float *)slabs.data_ptr(), M, N, K,
                         ep);
  return slabs;
}

// xs from decode_swizzle_x, ws from decode_swizzle_w(_layout); M/N/K of
// the ORIGINAL y[M,N] = x[M,K] @ W[N,K]^T problem. y is row-major in the
// original column order whatever the weight layout.
// u picks the k-steps per ring half: 0 = the default 8, 12 = the deeper
// ring that RB_DG_U=12 gives the raw/fused entry points. tail picks the K
// tail: 0 = the one-step loop, > 0 = through the ring, < 0 (default) =
// what RB_DG_TAIL says (the ring unless it is 0).
at::Tensor decode_gemm(at::Tensor xs, at::Tensor ws, int64_t M, int64_t N,
                       int64_t K, int64_t force_split, int64_t layout,
                       int64_t hq, int64_t hkv, int64_t dh, int64_t u,
                       int64_t tail) {
  TORCH_CHECK(xs.is_cuda() && ws.is_cuda() && xs.is_contiguous() &&
              ws.is_contiguous(), "decode_gemm: contiguous GPU tensors");
  TORCH_CHECK(xs.scalar_type() == at::kBFloat16 &&
              ws.scalar_type() == at::kBFloat16, "decode_gemm: bf16 only");
  TORCH_CHECK(xs.numel() == (K / 16) * 512, "decode_gemm: xs size");
  TORCH_CHECK(ws.numel() == N * K, "decode_gemm: ws size");
  TORCH_CHECK(decode_gemm_supported(M, N, K),
              "decode_gemm: unsupported shape ", M, "x", N, "x", K);
  TORCH_CHECK(force_split <= 8, "decode_gemm: force_split <= 8");
  TORCH_CHECK(u == 0 || u == 12, "decode_gemm: u must be 0 (8) or 12, got ",
              u);
  const int ring = u == 12 ? 12 : 8;
  const bool ring_tail = tail < 0 ? rb::dg_ring_tail() : tail != 0;
  const EpiArgs ep = layout_args(layout, N, hq, hkv, dh);

  auto stream = at::cuda::getCurrentHIPStream();
  auto y = at::empty({M, N}, xs.options());
  const int split = force_split > 0 ? (int)force_split
                                    : (int)decode_gemm_split(N, K);
  if (split == 1) {
    launch_dg_store<true>(layout, ring, ring_tail, 1, stream, xs, ws,
                          (uint16_t *)y.data_ptr(), nullptr, M, N, K, ep);
  } else {
    auto slabs = at::empty({split, M, N}, xs.options().dtype(at::kFloat));
    launch_dg_store<false>(layout, ring, ring_tail, split, stream, xs, ws,
                           nullptr, (float *)slabs.data_ptr(), M, N, K, ep);
    const int64_t mn = M * N;
    const int grid = rb::rb_grid_1d(mn / 4, 256);
    hipLaunchKernelGGL(decode_gemm_combine_kernel, dim3(grid), dim3(256),
                       0, stream, (const float *)slabs.data_ptr(),
                       (uint16_t *)y.data_ptr(), split, mn);
  }
  return y;
}

// Gate-up decode GEMM on a glu16 weight with the activation fused into
// the epilogue: returns the down-proj operand ([I/16][64][8] bf16, the
// layout decode_swizzle_x builds) of act(x Wg^T) * (x Wu^T). Values are
// those of swiglu/geglu_packed_dec(decode_gemm(...)); the row-major
// [M, I] tensor is not produced.
at::Tensor decode_gemm_glu(at::Tensor xs, at::Tensor ws, int64_t M,
                           int64_t N, int64_t K, bool gelu) {
  check_operands(xs, ws, M, N, K, "decode_gemm_glu");
  TORCH_CHECK(decode_gemm_split(N, K) == 1,
              "decode_gemm_glu: fused epilogue needs split == 1");
  EpiArgs ep = layout_args(LAYOUT_GLU16, N, 0, 0, 0);
  auto swz = at::empty({(N / 32) * 512}, xs.options());
  ep.swz = (uint16_t *)swz.data_ptr();
  auto stream = at::cuda::getCurrentHIPStream();
  if (gelu)
    launch_dg<true, EPI_GEGLU>(dg_u(), rb::dg_ring_tail(), 1, stream, xs, ws,
                               nullptr, nullptr, M, N, K, ep);
  else
    launch_dg<true, EPI_SWIGLU>(dg_u(), rb::dg_ring_tail(), 1, stream, xs, ws,
                                nullptr, nullptr, M, N, K, ep);
  return swz;
}

// qkv decode GEMM on a rope16 weight with RoPE + KV append fused into
// the epilogue: returns RoPE'd q [M, Hq, Dh]; RoPE'd k and plain v go
// straight into the paged bf16 cache (rows with slot < 0 skipped). Same
// values and cache layouts as qkv_rope_append(decode_gemm(...)).
at::Tensor decode_gemm_rope_append(at::Tensor xs, at::Tensor ws, int64_t M,
                                   int64_t N, int64_t K, at::Tensor cos,
                                   at::Tensor sin, at::Tensor positions,
                                   at::Tensor k_cache, at::Tensor v_cache,
                                   at::Tensor slot_mapping, int64_t hq) {
  check_operands(xs, ws, M, N, K, "decode_gemm_rope_append");
  TORCH_CHECK(decode_gemm_split(N, K) == 1,
              "decode_gemm_rope_append: fused epilogue needs split == 1");
  TORCH_CHECK(k_cache.is_cuda() && v_cache.is_cuda() && k_cache.dim() == 4 &&
              v_cache.dim() == 4 && k_cache.is_contiguous() &&
              v_cache.is_contiguous() &&
              k_cache.scalar_type() == at::kBFloat16 &&
              v_cache.scalar_type() == at::kBFloat16 &&
              v_cache.numel() == k_cache.numel(),
              "decode_gemm_rope_append: bf16 paged cache");
  const int64_t hkv = k_cache.size(1), bs = k_cache.size(2),
                dh = k_cache.size(3);
  EpiArgs ep = layout_args(LAYOUT_ROPE16, N, hq, hkv, dh);
  TORCH_CHECK(positions.is_cuda() && slot_mapping.is_cuda() &&
              positions.scalar_type() == at::kInt &&
              slot_mapping.scalar_type() == at::kInt &&
              positions.is_contiguous() && slot_mapping.is_contiguous() &&
              positions.numel() >= M && slot_mapping.numel() >= M,
              "decode_gemm_rope_append: idx");
  TORCH_CHECK(cos.is_cuda() && sin.is_cuda() &&
              cos.scalar_type() == at::kFloat &&
              sin.scalar_type() == at::kFloat && cos.is_contiguous() &&
              sin.is_contiguous() && cos.dim() == 2 &&
              cos.size(1) == dh / 2 && sin.sizes() == cos.sizes(),
              "decode_gemm_rope_append: rope tables [P, Dh/2] f32");
  auto q = at::empty({M, hq, dh}, xs.options());
  ep.bs = (int)bs;
  ep.q_out = (uint16_t *)q.data_ptr();
  ep.k_cache = (uint16_t *)k_cache.data_ptr();
  ep.v_cache = (uint16_t *)v_cache.data_ptr();
  ep.cs = cos.data_ptr<float>();
  ep.sn = sin.data_ptr<float>();
  ep.pos = positions.data_ptr<int32_t>();
  ep.slots = slot_mapping.data_ptr<int32_t>();
  const bool vt = v_cache.size(2) == dh && v_cache.size(3) == bs && dh != bs;
  auto stream = at::cuda::getCurrentHIPStream();
  if (vt)
    launch_dg<true, EPI_ROPE_VT>(dg_u(), rb::dg_ring_tail(), 1, stream, xs, ws,
                                 nullptr, nullptr, M, N, K, ep);
  else
    launch_dg<true, EPI_ROPE>(dg_u(), rb::dg_ring_tail(), 1, stream, xs, ws,
                              nullptr, nullptr, M, N, K, ep);
  return q;
}
