// int4 weight-only decode GEMM for CDNA4 (gfx950):
//   y[M,N] = x[M,K] @ dequant(Wq[N,K])^T, M <= 32 (decode batch),
// bf16 activations / bf16 out, fp32 accumulate. Serves the container
// contract's MODEL_LOAD_IN_4BIT (reference examples llama2-70b / falcon-40b
// server.yaml): the decode weight stream drops to 4.25 bits per weight.
//
// Quantization (ops/linear.py quantize_int4): symmetric, groups of 64
// along K, scale[n][g] = bf16(absmax/7), stored nibble = code + 8.
// dequantize_int4(..., bf16) is this kernel's EXACT weight reference:
// (nibble - 8) * float(scale) in fp32, then round-to-nearest-even bf16.
//
// Same skeleton as decode_gemm.hip (read its header first): one wave owns
// 32 W rows x a deep contiguous k-range, 4 waves per WG on adjacent
// k-ranges, a raw-byte register ping-pong ring, one LDS reduce at the
// end, optional cross-WG split with fp32 slabs + combine. No LDS and no
// barrier in the main loop; weights are converted at use, never at load.
//
// Layouts (private to this extension; w4_swizzle builds them once at
// load, tests/test_w4_cpu.py mirrors them lane by lane):
//  * wq_swz [N/32][K/64][64 lanes][16 B]: dword j (0..3) of lane l holds
//    the 8 nibbles (nibble i in bits 4i..4i+3) of A-fragment elements
//    i = 0..7 for row l&31, k = kb*64 + j*16 + (l>>5)*8 + i. One 16 B
//    load per lane = one contiguous 1 KiB nontemporal burst per wave =
//    four mfma_f32_32x32x16_bf16 k-steps of ONE quantization group.
//    (Against the canonical [N,K/2] bytes this is a pure byte permutation:
//    dword j is canonical bytes [row][(kb*64 + j*16 + (l>>5)*8)/2 .. +3].)
//  * sc_swz [N/32][K/64][32] bf16: 64 B per group, lane l reads l&31.
//  * xs: decode_swizzle_x's [K/16][lane][8] bf16 (zero rows for m >= M),
//    so every _rb_swz producer feeds this kernel unchanged.
//
// Dequant is plain C++ in registers: mask the even/odd nibbles of a dword
// into bytes (3 ops per 8 weights), one byte permute per weight builds
// the f32 128 + n, one fma with the group scale ((n - 8) * s ==
// fma(128 + n, s, -136 s) exactly: every term fits 16 significant bits),
// RNE to bf16 - about 2.4 VALU ops per weight against a budget of ~3 per
// weight per lane at full HBM rate. The scale is applied to the weights,
// not the accumulators: C rows differ per accumulator register, so a
// post-MFMA scale would cost 16 FMAs with 16 different scales per group.
//
// Fragment maps: see decode_gemm.hip (A = W, so C cols = m).
//
// Resource usage (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage):
//   decode_gemm_w4_kernel<*, true> (ring tail): 165 VGPRs, accumulator
//   included, no AGPRs, private segment (scratch) 0, 16 KiB LDS, 3
//   waves/SIMD; <*, false> (one-group tail loop): 202 VGPRs + 16 AGPRs,
//   scratch 0, 2 waves/SIMD. The grid puts at most a few waves on a SIMD;
//   the ring, not occupancy, keeps the bytes in flight.

#include <algorithm>

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"
#include "w4_dequant.h"

namespace {

constexpr int BLOCK = 256;   // 4 waves
constexpr int MMAX = 32;
constexpr int U = 4;         // groups (of 64 k) per ring half: 2x4 KiB W/wave

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8v;
typedef __attribute__((ext_vector_type(16))) float f32x16v;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4v;

__device__ __forceinline__ bf16x8v load8v(const uint16_t *p) {
  union { u32x4v u; bf16x8v v; } c;
  c.u = *reinterpret_cast<const u32x4v *>(p);
  return c.v;
}

// w4_byte_to_f32 / w4_dequant8: w4_dequant.h (shared with gemm_w4.hip).
using rb::w4_dequant8;

// One ring half = U groups: raw weight bytes (nontemporal: streamed once,
// must not evict L2), raw scale, and the 4 x fragments per group (plain
// loads: re-read by every n-block, L2 is where they want to live).
#define RB_W4_LOAD(WB, SB, XB, GBASE)                                    \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                        \
    WB[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4v *>( \
        wseg + (int64_t)((GBASE) + u) * 1024 + lane * 16));              \
    SB[u] = sseg[(int64_t)((GBASE) + u) * 32 + col];                     \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                      \
      XB[u * 4 + j] =                                                    \
          load8v(xs + ((int64_t)((GBASE) + u) * 4 + j) * 512 + lane8);   \
    }                                                                    \
  }

#define RB_W4_MFMA(WB, SB, XB)                                           \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                        \
    const float s = rb::bf16_to_f32(SB[u]);                              \
    const float nb = -136.0f * s;                                        \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                      \
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(                     \
          w4_dequant8(WB[u][j], s, nb), XB[u * 4 + j], acc, 0, 0, 0);    \
    }                                                                    \
  }

// A tail chunk: the same U group loads with the group index clamped to
// GLAST, the wave's last real group, so the load count stays static
// (counted vmcnt waits) and nothing outside the wave's own [g0, g1) is
// read. Only the first CNT groups are consumed.
#define RB_W4_LOAD_CLAMP(WB, SB, XB, GBASE, GLAST)                       \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                        \
    const int gc = min((GBASE) + u, (GLAST));                            \
    WB[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4v *>( \
        wseg + (int64_t)gc * 1024 + lane * 16));                         \
    SB[u] = sseg[(int64_t)gc * 32 + col];                                \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                      \
      XB[u * 4 + j] = load8v(xs + ((int64_t)gc * 4 + j) * 512 + lane8);  \
    }                                                                    \
  }

// The first CNT (wave-uniform, <= U) groups of a chunk, in order. A group
// that does not exist is branched over, never fed a zero operand.
#define RB_W4_MFMA_HEAD(WB, SB, XB, CNT)                                 \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                        \
    if (u < (CNT)) {                                                     \
      const float s = rb::bf16_to_f32(SB[u]);                            \
      const float nb = -136.0f * s;                                      \
      _Pragma("unroll") for (int j = 0; j < 4; ++j) {                    \
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(                   \
            w4_dequant8(WB[u][j], s, nb), XB[u * 4 + j], acc, 0, 0, 0);  \
      }                                                                  \
    }                                                                    \
  }

// STORE_BF16: write y bf16 directly (split == 1). Otherwise store an fp32
// slab slice at slabs + kslice*M*N for the combine kernel.
// RING_TAIL: as in decode_gemm.hip, over groups: the (g1 - g0) % 2U groups
// the ring pairs leave over go through the ring as up to two clamped
// chunks with all their loads in flight at once; false keeps the
// one-group-at-a-time loop (tail = 0 / RB_DG_TAIL=0). Same groups, same
// order, same accumulator: bit-identical outputs.
template <bool STORE_BF16, bool RING_TAIL>
__global__ __launch_bounds__(BLOCK, RING_TAIL ? 2 : 1) void
decode_gemm_w4_kernel(
    const uint16_t *__restrict__ xs, const uint8_t *__restrict__ wq,
    const uint16_t *__restrict__ sc, uint16_t *__restrict__ yp,
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

  // group range (groups of 64 k) for this (kslice, wave); contiguous per
  // wave so the W stream is one long sequential burst. The last waves
  // may get a short or EMPTY range (groups_total not a multiple of
  // 4*split): they contribute zeros to the reduce.
  const int groups_total = K / 64;
  const int nranges = split * 4;
  const int gpr = (groups_total + nranges - 1) / nranges;
  // uniform wave index for the ring tail's scalar branches and clamps
  const int wu = RING_TAIL ? __builtin_amdgcn_readfirstlane(wid) : wid;
  const int g0 = min(groups_total, (kslice * 4 + wu) * gpr);
  const int g1 = min(groups_total, g0 + gpr);

  const uint8_t *wseg = wq + (int64_t)nblk * groups_total * 1024;
  const uint16_t *sseg = sc + (int64_t)nblk * groups_total * 32;

  f32x16v acc = (f32x16v)(0.0f);

  u32x4v wA[U], wB[U];
  uint16_t sA[U], sB[U];
  bf16x8v xA[4 * U], xB[4 * U];
  int g = g0;
  const int nmain = ((g1 - g0) / (2 * U)) * (2 * U);
  if constexpr (RING_TAIL) {
    const int gmain = g0 + nmain;
    const int t1 = min(g1 - gmain, U);   // tail chunk 1: 0..U groups
    const int t2 = g1 - gmain - U;       // tail chunk 2: > 0 when it exists
    const int glast = g1 - 1;
    if (nmain > 0) {
      RB_W4_LOAD(wA, sA, xA, g);
      for (; g + 2 * U < gmain; g += 2 * U) {
        RB_W4_LOAD(wB, sB, xB, g + U);
        RB_W4_MFMA(wA, sA, xA);
        RB_W4_LOAD(wA, sA, xA, g + 2 * U);
        RB_W4_MFMA(wB, sB, xB);
      }
      // last pair: the A half it frees takes tail chunk 1, whose loads
      // fly under the B chunk's MFMAs
      RB_W4_LOAD(wB, sB, xB, g + U);
      RB_W4_MFMA(wA, sA, xA);
      if (t1 > 0) {
        RB_W4_LOAD_CLAMP(wA, sA, xA, gmain, glast);
        RB_W4_MFMA(wB, sB, xB);
        if (t2 > 0) {
          RB_W4_LOAD_CLAMP(wB, sB, xB, gmain + U, glast);
          RB_W4_MFMA_HEAD(wA, sA, xA, t1);
          RB_W4_MFMA_HEAD(wB, sB, xB, t2);
        } else {
          RB_W4_MFMA_HEAD(wA, sA, xA, t1);
        }
      } else {
        RB_W4_MFMA(wB, sB, xB);
      }
    } else if (t1 > 0) {                 // the whole range is tail
      RB_W4_LOAD_CLAMP(wA, sA, xA, g0, glast);
      if (t2 > 0) {
        RB_W4_LOAD_CLAMP(wB, sB, xB, g0 + U, glast);
        RB_W4_MFMA_HEAD(wA, sA, xA, t1);
        RB_W4_MFMA_HEAD(wB, sB, xB, t2);
      } else {
        RB_W4_MFMA_HEAD(wA, sA, xA, t1);
      }
    }
  } else {
    if (nmain > 0) {
      RB_W4_LOAD(wA, sA, xA, g);
      const int gmain = g0 + nmain;
      for (; g + 2 * U <= gmain; g += 2 * U) {
        RB_W4_LOAD(wB, sB, xB, g + U);
        RB_W4_MFMA(wA, sA, xA);
        if (g + 2 * U < gmain) { RB_W4_LOAD(wA, sA, xA, g + 2 * U); }
        RB_W4_MFMA(wB, sB, xB);
      }
    }
    // tail: single groups, no prefetch (<= 2U-1 iterations)
    for (; g < g1; ++g) {
      const u32x4v w1 = __builtin_nontemporal_load(
          reinterpret_cast<const u32x4v *>(wseg + (int64_t)g * 1024 +
                                           lane * 16));
      const float s = rb::bf16_to_f32(sseg[(int64_t)g * 32 + col]);
      const float nb = -136.0f * s;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16x8v x1 = load8v(xs + ((int64_t)g * 4 + j) * 512 + lane8);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            w4_dequant8(w1[j], s, nb), x1, acc, 0, 0, 0);
      }
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
          yp + (int64_t)em * N + nblk * 32 + en) = o.q;
    } else {
      float *slab = slabs + ((int64_t)kslice * M + em) * N + nblk * 32 + en;
      *reinterpret_cast<float4 *>(slab) =
          make_float4(sum[0], sum[1], sum[2], sum[3]);
    }
  }
}

// slabs [SPLIT, M, N] f32 -> y [M, N] bf16
__global__ void decode_gemm_w4_combine_kernel(
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

// Does any (kslice, wave) range of this launch have a K tail, i.e. a group
// count that is no multiple of the ring pair 2U? The kernel's partition.
bool w4_has_tail(int64_t K, int split) {
  const int groups_total = (int)(K / 64), nranges = split * 4;
  const int gpr = (groups_total + nranges - 1) / nranges;
  for (int r = 0; r < nranges; ++r) {
    const int g0 = std::min(groups_total, r * gpr);
    const int n = std::min(groups_total, g0 + gpr) - g0;
    if (n % (2 * U) != 0) return true;
  }
  return false;
}

// The ring-tail instantiation is launched only where some wave has a tail;
// a launch without one keeps the kernel it had before the ring tail.
template <bool STORE_BF16>
void launch_w4(bool ring_tail, const dim3 &grid, hipStream_t stream,
               const at::Tensor &xs, const at::Tensor &wq_swz,
               const at::Tensor &sc_swz, uint16_t *y, float *slabs,
               int64_t M, int64_t N, int64_t K) {
  if (ring_tail && w4_has_tail(K, (int)grid.y))
    hipLaunchKernelGGL((decode_gemm_w4_kernel<STORE_BF16, true>), grid,
                       dim3(BLOCK), 0, stream,
                       (const uint16_t *)xs.data_ptr(),
                       (const uint8_t *)wq_swz.data_ptr(),
                       (const uint16_t *)sc_swz.data_ptr(), y, slabs,
                       (int)M, (int)N, (int)K);
  else
    hipLaunchKernelGGL((decode_gemm_w4_kernel<STORE_BF16, false>), grid,
                       dim3(BLOCK), 0, stream,
                       (const uint16_t *)xs.data_ptr(),
                       (const uint8_t *)wq_swz.data_ptr(),
                       (const uint16_t *)sc_swz.data_ptr(), y, slabs,
                       (int)M, (int)N, (int)K);
}

}  // namespace

// Cross-WG k-split, same load-balance reasoning as decode_gemm_split:
// split only while the grid cannot cover the 256 CUs, and only while
// every wave keeps at least one full ring (2U groups) of k-range. No
// divisibility requirement: the kernel handles uneven and empty ranges.
int64_t decode_gemm_w4_split(int64_t N, int64_t K) {
  const int64_t nblocks = N / 32;
  int64_t split = 1;
  while (split < 8 && nblocks * split < 256 &&
         K / 64 >= 2 * U * 4 * (split * 2)) {
    split *= 2;
  }
  return split;
}

bool decode_gemm_w4_supported(int64_t M, int64_t N, int64_t K) {
  return M >= 1 && M <= MMAX && N >= 32 && N % 32 == 0 && K >= 64 &&
         K % 64 == 0;
}

// One-time layout build (device-side tensor ops): canonical q [N, K/2]
// uint8 + scales [N, K/64] bf16 -> (wq_swz, sc_swz) as documented above.
std::vector<at::Tensor> w4_swizzle(at::Tensor q, at::Tensor scales) {
  TORCH_CHECK(q.dim() == 2 && q.scalar_type() == at::kByte &&
              q.is_contiguous(), "w4_swizzle: contiguous uint8 q [N,K/2]");
  const int64_t N = q.size(0), K = q.size(1) * 2;
  TORCH_CHECK(N >= 32 && N % 32 == 0 && K >= 64 && K % 64 == 0,
              "w4_swizzle: shape");
  TORCH_CHECK(scales.dim() == 2 && scales.scalar_type() == at::kBFloat16 &&
              scales.is_contiguous() && scales.size(0) == N &&
              scales.size(1) == K / 64,
              "w4_swizzle: contiguous bf16 scales [N,K/64]");
  // q bytes as [nb][row][kb][j][hi][4 B] -> [nb][kb][hi][row][j][4 B]
  auto wq = q.view({N / 32, 32, K / 64, 4, 2, 4})
                .permute({0, 2, 4, 1, 3, 5}).contiguous()
                .view({N / 32, K / 64, 64, 16});
  auto sc = scales.view({N / 32, 32, K / 64}).permute({0, 2, 1}).contiguous();
  return {wq, sc};
}

// xs from decode_swizzle_x (or any _rb_swz producer), wq_swz / sc_swz from
// w4_swizzle; M/N/K of the ORIGINAL y[M,N] = x[M,K] @ W[N,K]^T problem.
// Workspaces (y, slabs) come from the caching allocator like
// decode_gemm's, so they are pointer-stable under hipGraph capture.
// tail: 0 = the one-group loop, > 0 = through the ring, < 0 (default) =
// what RB_DG_TAIL says (the ring unless it is 0).
at::Tensor decode_gemm_w4(at::Tensor xs, at::Tensor wq_swz, at::Tensor sc_swz,
                          int64_t M, int64_t N, int64_t K,
                          int64_t force_split, int64_t tail) {
  TORCH_CHECK(xs.is_cuda() && wq_swz.is_cuda() && sc_swz.is_cuda() &&
              xs.is_contiguous() && wq_swz.is_contiguous() &&
              sc_swz.is_contiguous(),
              "decode_gemm_w4: contiguous GPU tensors");
  TORCH_CHECK(xs.scalar_type() == at::kBFloat16 &&
              wq_swz.scalar_type() == at::kByte &&
              sc_swz.scalar_type() == at::kBFloat16,
              "decode_gemm_w4: dtypes");
  TORCH_CHECK(decode_gemm_w4_supported(M, N, K),
              "decode_gemm_w4: unsupported shape ", M, "x", N, "x", K);
  TORCH_CHECK(xs.numel() == (K / 16) * 512, "decode_gemm_w4: xs size");
  TORCH_CHECK(wq_swz.numel() == N * K / 2, "decode_gemm_w4: wq_swz size");
  TORCH_CHECK(sc_swz.numel() == N * (K / 64), "decode_gemm_w4: sc_swz size");
  TORCH_CHECK(force_split <= 8, "decode_gemm_w4: force_split <= 8");
  const bool ring_tail = tail < 0 ? rb::dg_ring_tail() : tail != 0;

  auto stream = at::cuda::getCurrentHIPStream();
  auto y = at::empty({M, N}, xs.options());
  const int split = force_split > 0 ? (int)force_split
                                    : (int)decode_gemm_w4_split(N, K);
  if (split == 1) {
    launch_w4<true>(ring_tail, dim3(N / 32, 1), stream, xs, wq_swz, sc_swz,
                    (uint16_t *)y.data_ptr(), nullptr, M, N, K);
  } else {
    auto slabs = at::empty({split, M, N}, xs.options().dtype(at::kFloat));
    launch_w4<false>(ring_tail, dim3(N / 32, split), stream, xs, wq_swz,
                     sc_swz, nullptr, (float *)slabs.data_ptr(), M, N, K);
    const int64_t mn = M * N;
    const int grid = rb::rb_grid_1d(mn / 4, 256);
    hipLaunchKernelGGL(decode_gemm_w4_combine_kernel, dim3(grid), dim3(256),
                       0, stream, (const float *)slabs.data_ptr(),
                       (uint16_t *)y.data_ptr(), split, mn);
  }
  return y;
}
