// fp8 (OCP e4m3) weight-only decode GEMM for CDNA4 (gfx950):
//   y[M,N] = bf16_rne( scale[n] * sum_k x[m,k] * e4m3(W8[n,k]) ),
// M <= 32 (decode batch), N % 32 == 0, K % 32 == 0, bf16 activations /
// bf16 out, fp32 accumulate, f32 per-output-channel scale. Serves the
// container contract's MODEL_LOAD_IN_8BIT (reference examples llama2-7b /
// llama2-70b server.yaml) on the canonical pair ops/linear.py quantize_fp8
// produces: one byte per weight plus 4 bytes per row.
//
// The fp8 member of the weight-stream family. Same skeleton as
// decode_gemm.hip and decode_gemm_w4.hip (read their headers first): one
// wave owns 32 W rows x a deep contiguous k-range, 4 waves per WG on
// adjacent k-ranges, a raw-byte register ping-pong ring, one 16 KiB LDS
// reduce at the end, optional cross-WG split with fp32 slabs + combine. No
// LDS and no barrier in the main loop; weights are converted at use, never
// at load. It replaces skinny_gemm.hip's fp8 tile kernel, which stages W
// through LDS behind a barrier, on the decode path.
//
// Layouts:
//  * w8_swz [N/32][K/32][64 lanes][16 B], built once at load by w8_swizzle:
//    bytes 0..7 of lane l are A-fragment elements i = 0..7 of row l&31 at
//    k = kb*32 + (l>>5)*8 + i, bytes 8..15 the same elements at k + 16. One
//    16 B load per lane = one contiguous 1 KiB nontemporal burst per wave
//    = two mfma_f32_32x32x16_bf16 k-steps. A pure byte permutation of the
//    canonical [N, K] bytes.
//  * scale: the canonical f32 [N], untouched.
//  * xs: decode_swizzle_x's [K/16][lane][8] bf16 (zero rows for m >= M),
//    so every _rb_swz producer feeds this kernel unchanged. Plain loads: x
//    is re-read by every n-block and lives in L2.
//
// Dequant: v_cvt_pk_f32_fp8 (gfx950 converts OCP e4m3 natively; the same
// builtin skinny_gemm.hip uses) turns two codes into two f32, and one byte
// permute packs the two high halves into a bf16 pair: 8 ops per 8 weights.
// e4m3 has 3 mantissa bits and its exponent range sits inside bf16's, so
// the truncation drops only zero bits: exact for all 254 finite codes,
// subnormals and -0 included. quantize_fp8 never emits the two NaN codes
// (0x7f, 0xff): torch's float8_e4m3fn cast saturates finite inputs. A NaN
// code would still arrive as a bf16 NaN.
//
// Scale: NOT applied to the weights. It is per output channel, i.e.
// constant along the k-sum, so it multiplies the fp32 sum once, after the
// 4-wave LDS reduce (split 1) or after the combine kernel has added the
// slab slices in slice order (split > 1); then one RNE to bf16. An
// output's summation order depends on (N, K, split) alone, there are no
// atomics, reruns are bit-identical.
//
// Ring depth. A ring block is 32 k: one 16 B W load (4 VGPRs) and two x
// fragments (8 VGPRs). Per k, x costs what it costs in the bf16 kernel
// while W costs half, so x bounds the depth. hipcc -O3, gfx950,
// -Rpass-analysis=kernel-resource-usage, <STORE_BF16 = true> (the slab
// variants are within 2 VGPRs):
//
//   U  W in ring/wave  <*, true> ring tail              <*, false> loop
//   4   8 KiB          142 VGPRs, scratch 0, 3 waves/SIMD  138, 0, 3
//   6  12 KiB          192 VGPRs, scratch 0, 2 waves/SIMD  186, 0, 2
//   8  16 KiB          256 VGPRs, scratch 76 B/lane, 2     238, 0, 2
//
// all with no AGPRs and 16 KiB LDS; the combine kernel takes 19 VGPRs.
// U = 8 spills, so it is out. U = 4 is built: 2 x 4 blocks = 256 k per
// wave in flight, the k-depth of the bf16 ring (2 x 8 steps of 16), 8 KiB
// of W + 16 KiB of x per wave, and the only depth that keeps 3
// waves/SIMD, which the wide shapes (gate-up: 688 WGs on 256 CUs) want.
// Little's law asks for ~9 KB per CU at 24.6 GB/s/CU; one WG has 32 KiB
// of W in flight. U = 6 has not been timed.
//
// Out of scope here: fused SwiGLU / RoPE-append epilogues for fp8, the
// slab hand-off to the rmsnorm, and quantizing activations to use the fp8
// MFMA - this is weight-only by design. M > 32 on the same resident copy
// is gemm_w8.hip.
//
// Fragment maps: see decode_gemm.hip (A = W, so C cols = m).

#include <algorithm>

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"
#include "w8_dequant.h"

namespace {

constexpr int BLOCK = 256;   // 4 waves
constexpr int MMAX = 32;
constexpr int U = 4;         // blocks (of 32 k) per ring half: 2x4 KiB W/wave

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8v;
typedef __attribute__((ext_vector_type(16))) float f32x16v;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4v;

__device__ __forceinline__ bf16x8v load8v(const uint16_t *p) {
  union { u32x4v u; bf16x8v v; } c;
  c.u = *reinterpret_cast<const u32x4v *>(p);
  return c.v;
}

// e4m3 -> bf16 at use: w8_dequant.h, shared with gemm_w8.hip
using rb::w8_dequant8;

// One ring half = U blocks: raw weight bytes (nontemporal: streamed once,
// must not evict L2) and the 2 x fragments per block (plain loads).
#define RB_W8_LOAD(WB, XB, BBASE)                                        \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                        \
    WB[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4v *>( \
        wseg + (int64_t)((BBASE) + u) * 1024 + lane * 16));              \
    XB[u * 2] = load8v(xs + (int64_t)((BBASE) + u) * 1024 + lane8);      \
    XB[u * 2 + 1] =                                                      \
        load8v(xs + (int64_t)((BBASE) + u) * 1024 + 512 + lane8);        \
  }

#define RB_W8_MFMA1(W, X0, X1)                                           \
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(                         \
      w8_dequant8(W[0], W[1]), X0, acc, 0, 0, 0);                        \
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(                         \
      w8_dequant8(W[2], W[3]), X1, acc, 0, 0, 0);

#define RB_W8_MFMA(WB, XB)                                               \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                        \
    RB_W8_MFMA1(WB[u], XB[u * 2], XB[u * 2 + 1])                         \
  }

// A tail chunk: the same U block loads with the block index clamped to
// BLAST, the wave's last real block, so the load count stays static
// (counted vmcnt waits) and nothing outside the wave's own [b0, b1) is
// read. Only the first CNT blocks are consumed.
#define RB_W8_LOAD_CLAMP(WB, XB, BBASE, BLAST)                           \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                        \
    const int bc = min((BBASE) + u, (BLAST));                            \
    WB[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4v *>( \
        wseg + (int64_t)bc * 1024 + lane * 16));                         \
    XB[u * 2] = load8v(xs + (int64_t)bc * 1024 + lane8);                 \
    XB[u * 2 + 1] = load8v(xs + (int64_t)bc * 1024 + 512 + lane8);       \
  }

// The first CNT (wave-uniform, <= U) blocks of a chunk, in order. A block
// that does not exist is branched over, never fed a zero operand.
#define RB_W8_MFMA_HEAD(WB, XB, CNT)                                     \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                        \
    if (u < (CNT)) { RB_W8_MFMA1(WB[u], XB[u * 2], XB[u * 2 + 1]) }      \
  }

// STORE_BF16: scale and write y bf16 directly (split == 1). Otherwise
// store an UNSCALED fp32 slab slice at slabs + kslice*M*N for the combine
// kernel. RING_TAIL: as in the siblings, over blocks: the (b1 - b0) % 2U
// blocks the ring pairs leave over go through the ring as up to two
// clamped chunks with all their loads in flight at once; false keeps the
// one-block-at-a-time loop (tail = 0 / RB_DG_TAIL=0). Same blocks, same
// order, same accumulator: bit-identical outputs.
template <bool STORE_BF16, bool RING_TAIL>
RB_W8_NO_PK __global__ __launch_bounds__(BLOCK, 2) void decode_gemm_w8_kernel(
    const uint16_t *__restrict__ xs, const uint8_t *__restrict__ w8,
    const float *__restrict__ scale, uint16_t *__restrict__ yp,
    float *__restrict__ slabs, int M, int N, int K) {
  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int hi = lane >> 5;
  const int col = lane & 31;
  const int lane8 = lane * 8;

  const int nblk = blockIdx.x;           // 32 W rows per WG
  const int kslice = blockIdx.y;
  const int split = gridDim.y;

  // block range (blocks of 32 k) for this (kslice, wave); contiguous per
  // wave so the W stream is one long sequential burst. The last waves may
  // get a short or EMPTY range (blocks_total not a multiple of 4*split):
  // they contribute zeros to the reduce.
  const int blocks_total = K / 32;
  const int nranges = split * 4;
  const int bpr = (blocks_total + nranges - 1) / nranges;
  // uniform wave index for the ring tail's scalar branches and clamps
  const int wu = RING_TAIL ? __builtin_amdgcn_readfirstlane(wid) : wid;
  const int b0 = min(blocks_total, (kslice * 4 + wu) * bpr);
  const int b1 = min(blocks_total, b0 + bpr);

  const uint8_t *wseg = w8 + (int64_t)nblk * blocks_total * 1024;

  f32x16v acc = (f32x16v)(0.0f);

  u32x4v wA[U], wB[U];
  bf16x8v xA[2 * U], xB[2 * U];
  int b = b0;
  const int nmain = ((b1 - b0) / (2 * U)) * (2 * U);
  if constexpr (RING_TAIL) {
    const int bmain = b0 + nmain;
    const int t1 = min(b1 - bmain, U);   // tail chunk 1: 0..U blocks
    const int t2 = b1 - bmain - U;       // tail chunk 2: > 0 when it exists
    const int blast = b1 - 1;
    if (nmain > 0) {
      RB_W8_LOAD(wA, xA, b);
      for (; b + 2 * U < bmain; b += 2 * U) {
        RB_W8_LOAD(wB, xB, b + U);
        RB_W8_MFMA(wA, xA);
        RB_W8_LOAD(wA, xA, b + 2 * U);
        RB_W8_MFMA(wB, xB);
      }
      // last pair: the A half it frees takes tail chunk 1, whose loads
      // fly under the B chunk's MFMAs
      RB_W8_LOAD(wB, xB, b + U);
      RB_W8_MFMA(wA, xA);
      if (t1 > 0) {
        RB_W8_LOAD_CLAMP(wA, xA, bmain, blast);
        RB_W8_MFMA(wB, xB);
        if (t2 > 0) {
          RB_W8_LOAD_CLAMP(wB, xB, bmain + U, blast);
          RB_W8_MFMA_HEAD(wA, xA, t1);
          RB_W8_MFMA_HEAD(wB, xB, t2);
        } else {
          RB_W8_MFMA_HEAD(wA, xA, t1);
        }
      } else {
        RB_W8_MFMA(wB, xB);
      }
    } else if (t1 > 0) {                 // the whole range is tail
      RB_W8_LOAD_CLAMP(wA, xA, b0, blast);
      if (t2 > 0) {
        RB_W8_LOAD_CLAMP(wB, xB, b0 + U, blast);
        RB_W8_MFMA_HEAD(wA, xA, t1);
        RB_W8_MFMA_HEAD(wB, xB, t2);
      } else {
        RB_W8_MFMA_HEAD(wA, xA, t1);
      }
    }
  } else {
    if (nmain > 0) {
      RB_W8_LOAD(wA, xA, b);
      const int bmain = b0 + nmain;
      for (; b + 2 * U <= bmain; b += 2 * U) {
        RB_W8_LOAD(wB, xB, b + U);
        RB_W8_MFMA(wA, xA);
        if (b + 2 * U < bmain) { RB_W8_LOAD(wA, xA, b + 2 * U); }
        RB_W8_MFMA(wB, xB);
      }
    }
    // tail: single blocks, no prefetch (<= 2U-1 iterations)
    for (; b < b1; ++b) {
      const u32x4v w1 = __builtin_nontemporal_load(
          reinterpret_cast<const u32x4v *>(wseg + (int64_t)b * 1024 +
                                           lane * 16));
      const bf16x8v x0 = load8v(xs + (int64_t)b * 1024 + lane8);
      const bf16x8v x1 = load8v(xs + (int64_t)b * 1024 + 512 + lane8);
      RB_W8_MFMA1(w1, x0, x1)
    }
  }

  // ---- cross-wave reduction in LDS -------------------------------------
  // 1024 outputs, 4 per thread, n fastest so bf16 stores coalesce 8 B.
  const int em = tid >> 3;               // 0..31
  const int en = (tid & 7) * 4;          // 0,4,..,28
  float4 sc = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
  if (STORE_BF16) {                      // lands under the barrier
    sc = *reinterpret_cast<const float4 *>(scale + nblk * 32 + en);
  }
  __shared__ __attribute__((aligned(16))) float red[4][32][MMAX];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n_local = (r & 3) + 8 * (r >> 2) + 4 * hi;
    red[wid][n_local][col] = acc[r];
  }
  __syncthreads();

  if (em < M) {
    float sum[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sum[j] = red[0][en + j][em] + red[1][en + j][em] +
               red[2][en + j][em] + red[3][en + j][em];
    }
    if (STORE_BF16) {
      union { uint16_t u[4]; uint64_t q; } o;
      o.u[0] = rb::f32_to_bf16(sum[0] * sc.x);
      o.u[1] = rb::f32_to_bf16(sum[1] * sc.y);
      o.u[2] = rb::f32_to_bf16(sum[2] * sc.z);
      o.u[3] = rb::f32_to_bf16(sum[3] * sc.w);
      *reinterpret_cast<uint64_t *>(
          yp + (int64_t)em * N + nblk * 32 + en) = o.q;
    } else {
      float *slab = slabs + ((int64_t)kslice * M + em) * N + nblk * 32 + en;
      *reinterpret_cast<float4 *>(slab) =
          make_float4(sum[0], sum[1], sum[2], sum[3]);
    }
  }
}

// slabs [SPLIT, M, N] f32 -> y [M, N] bf16: slices added in slice order,
// then the channel scale, then one rounding. N % 4 == 0, so the 4 outputs
// of a thread share a row and its scales are one float4.
RB_W8_NO_PK __global__ void decode_gemm_w8_combine_kernel(
    const float *__restrict__ slabs, const float *__restrict__ scale,
    uint16_t *__restrict__ yp, int split, int N, int64_t mn) {
  const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
  for (int64_t i = i0; i < mn; i += stride) {
    float4 s = *reinterpret_cast<const float4 *>(slabs + i);
    for (int k = 1; k < split; ++k) {
      float4 t = *reinterpret_cast<const float4 *>(slabs + (int64_t)k * mn + i);
      s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    const float4 c = *reinterpret_cast<const float4 *>(scale + i % N);
    union { uint16_t u[4]; uint64_t q; } o;
    o.u[0] = rb::f32_to_bf16(s.x * c.x); o.u[1] = rb::f32_to_bf16(s.y * c.y);
    o.u[2] = rb::f32_to_bf16(s.z * c.z); o.u[3] = rb::f32_to_bf16(s.w * c.w);
    *reinterpret_cast<uint64_t *>(yp + i) = o.q;
  }
}

// Does any (kslice, wave) range of this launch have a K tail, i.e. a block
// count that is no multiple of the ring pair 2U? The kernel's partition.
bool w8_has_tail(int64_t K, int split) {
  const int blocks_total = (int)(K / 32), nranges = split * 4;
  const int bpr = (blocks_total + nranges - 1) / nranges;
  for (int r = 0; r < nranges; ++r) {
    const int b0 = std::min(blocks_total, r * bpr);
    const int n = std::min(blocks_total, b0 + bpr) - b0;
    if (n % (2 * U) != 0) return true;
  }
  return false;
}

// The ring-tail instantiation is launched only where some wave has a tail.
template <bool STORE_BF16>
void launch_w8(bool ring_tail, const dim3 &grid, hipStream_t stream,
               const at::Tensor &xs, const at::Tensor &w8_swz,
               const at::Tensor &scale, uint16_t *y, float *slabs,
               int64_t M, int64_t N, int64_t K) {
  if (ring_tail && w8_has_tail(K, (int)grid.y))
    hipLaunchKernelGGL((decode_gemm_w8_kernel<STORE_BF16, true>), grid,
                       dim3(BLOCK), 0, stream,
                       (const uint16_t *)xs.data_ptr(),
                       (const uint8_t *)w8_swz.data_ptr(),
                       (const float *)scale.data_ptr(), y, slabs,
                       (int)M, (int)N, (int)K);
  else
    hipLaunchKernelGGL((decode_gemm_w8_kernel<STORE_BF16, false>), grid,
                       dim3(BLOCK), 0, stream,
                       (const uint16_t *)xs.data_ptr(),
                       (const uint8_t *)w8_swz.data_ptr(),
                       (const float *)scale.data_ptr(), y, slabs,
                       (int)M, (int)N, (int)K);
}

}  // namespace

// Cross-WG k-split, decode_gemm_w4_split's policy in this kernel's units:
// split only while the grid cannot cover the 256 CUs, and only while every
// wave keeps at least one full ring (2U blocks) of k-range. No
// divisibility requirement: the kernel handles uneven and empty ranges.
// One measured addition (the force_split sweep in profiles/README.md):
// a split grid whose waves would still keep two full rings each after
// another doubling takes it, up to 2 WGs per CU. That is down-proj
// (4096 x 11008: split 4, 19.4 us against 20.8 us at split 2); o_proj
// (4096 x 4096) stays at 2, which the sweep also found best.
int64_t decode_gemm_w8_split(int64_t N, int64_t K) {
  const int64_t nblocks = N / 32;
  int64_t split = 1;
  while (split < 8 && nblocks * split < 256 &&
         K / 32 >= 2 * U * 4 * (split * 2)) {
    split *= 2;
  }
  if (split > 1 && split < 8 && nblocks * split < 512 &&
      K / 32 >= 2 * (2 * U * 4 * (split * 2))) {
    split *= 2;
  }
  return split;
}

bool decode_gemm_w8_supported(int64_t M, int64_t N, int64_t K) {
  return M >= 1 && M <= MMAX && N >= 32 && N % 32 == 0 && K >= 32 &&
         K % 32 == 0;
}

// One-time layout build (device-side tensor ops): canonical e4m3 bytes
// [N, K] uint8 -> w8_swz as documented above.
at::Tensor w8_swizzle(at::Tensor w8) {
  TORCH_CHECK(w8.dim() == 2 && w8.scalar_type() == at::kByte &&
              w8.is_contiguous(), "w8_swizzle: contiguous uint8 w8 [N,K]");
  const int64_t N = w8.size(0), K = w8.size(1);
  TORCH_CHECK(N >= 32 && N % 32 == 0 && K >= 32 && K % 32 == 0,
              "w8_swizzle: shape");
  // bytes as [nb][row][kb][k+16][hi][8 B] -> [nb][kb][hi][row][k+16][8 B]
  return w8.view({N / 32, 32, K / 32, 2, 2, 8})
      .permute({0, 2, 4, 1, 3, 5}).contiguous()
      .view({N / 32, K / 32, 64, 16});
}

// xs from decode_swizzle_x (or any _rb_swz producer), w8_swz from
// w8_swizzle, scale the canonical f32 [N]; M/N/K of the ORIGINAL
// y[M,N] = x[M,K] @ W[N,K]^T problem. Workspaces (y, slabs) come from the
// caching allocator like decode_gemm's, so they are pointer-stable under
// hipGraph capture. tail: 0 = the one-block loop, > 0 = through the ring,
// < 0 (default) = what RB_DG_TAIL says (the ring unless it is 0).
at::Tensor decode_gemm_w8(at::Tensor xs, at::Tensor w8_swz, at::Tensor scale,
                          int64_t M, int64_t N, int64_t K,
                          int64_t force_split, int64_t tail) {
  TORCH_CHECK(xs.is_cuda() && w8_swz.is_cuda() && scale.is_cuda() &&
              xs.is_contiguous() && w8_swz.is_contiguous() &&
              scale.is_contiguous(),
              "decode_gemm_w8: contiguous GPU tensors");
  TORCH_CHECK(xs.scalar_type() == at::kBFloat16 &&
              w8_swz.scalar_type() == at::kByte &&
              scale.scalar_type() == at::kFloat,
              "decode_gemm_w8: dtypes");
  TORCH_CHECK(decode_gemm_w8_supported(M, N, K),
              "decode_gemm_w8: unsupported shape ", M, "x", N, "x", K);
  TORCH_CHECK(xs.numel() == (K / 16) * 512, "decode_gemm_w8: xs size");
  TORCH_CHECK(w8_swz.numel() == N * K, "decode_gemm_w8: w8_swz size");
  TORCH_CHECK(scale.numel() == N, "decode_gemm_w8: scale size");
  TORCH_CHECK(force_split <= 8, "decode_gemm_w8: force_split <= 8");
  const bool ring_tail = tail < 0 ? rb::dg_ring_tail() : tail != 0;

  auto stream = at::cuda::getCurrentHIPStream();
  auto y = at::empty({M, N}, xs.options());
  const int split = force_split > 0 ? (int)force_split
                                    : (int)decode_gemm_w8_split(N, K);
  if (split == 1) {
    launch_w8<true>(ring_tail, dim3(N / 32, 1), stream, xs, w8_swz, scale,
                    (uint16_t *)y.data_ptr(), nullptr, M, N, K);
  } else {
    auto slabs = at::empty({split, M, N}, xs.options().dtype(at::kFloat));
    launch_w8<false>(ring_tail, dim3(N / 32, split), stream, xs, w8_swz,
                     scale, nullptr, (float *)slabs.data_ptr(), M, N, K);
    const int64_t mn = M * N;
    const int grid = rb::rb_grid_1d(mn / 4, 256);
    hipLaunchKernelGGL(decode_gemm_w8_combine_kernel, dim3(grid), dim3(256),
                       0, stream, (const float *)slabs.data_ptr(),
                       (const float *)scale.data_ptr(),
                       (uint16_t *)y.data_ptr(), split, (int)N, mn);
  }
  return y;
}
