// int4 weight-only MFMA GEMM for CDNA4 (gfx950), any M:
//   y[M,N] = x[M,K] @ dequant(Wq[N,K])^T,
// x bf16 [M,K] row-major, y bf16 [M,N], fp32 accumulate. The large-M
// companion of decode_gemm_w4.hip (M <= 32): prefill, chunked and batched
// prefill of a MODEL_LOAD_IN_4BIT model run here, so such a model needs no
// bf16 master weights (ops/linear.py release_w4_masters).
//
// Operands: the SAME stored copy the decode kernel streams, wq_swz
// [N/32][K/64][64 lanes][16 B] and sc_swz [N/32][K/64][32] bf16 exactly
// as w4_swizzle builds them (layout: decode_gemm_w4.hip header), and x
// as plain row-major rows (no _rb_swz operand protocol at large M).
// Weights are dequantized in registers by w4_dequant.h, the decode
// kernel's expressions, so dequantize_int4(q, s, bf16) is the exact
// weight reference here too.
//
// Structure (A = W, so C columns = m; fragment maps: mfma_frag.h):
//  * one workgroup = 4 waves = 128 W rows x (MT * 32) x rows; wave w owns
//    the 32-row n-block 4 * blockIdx.x + w and ALL MT m-tiles, as MT
//    separate f32x16 accumulators. One 16 B load per lane is one 1 KiB
//    burst = the four 32x32x16 k-steps of one quantization group; each
//    dequantized fragment is used by MT MFMAs (MT = 4 for M > 64, so the
//    ~2.4 VALU ops per weight are paid once per 128 output rows).
//  * the x tile of one group ([MT*32][64] bf16) is staged through LDS by
//    the whole workgroup in full 128 B lines (8 lanes x 16 B per row),
//    double-buffered, rows padded to 144 B: the B-fragment ds_read_b128
//    of 16 consecutive rows then lands on 16 distinct 16 B bank slots.
//  * both streams are software-pipelined through registers: W and scales
//    two groups ahead, x one group ahead in registers + one in LDS; one
//    barrier per group. Loads past the last group re-read the last group
//    (in bounds, unused) instead of branching around the load.
//  * rows >= M of a ragged m-tile are never loaded: their address is
//    clamped to row M-1 and zeros are written to LDS in their place.
//    A wave whose n-block is past N/32 (ragged n-tile) streams the last
//    valid block and stores nothing.
//
// Determinism / row independence: no k-split, no atomics. Every output
// element is one accumulator column fed k = 0, 16, 32, ... in order, so
// its summation order depends on K alone, never on M, the tile a row
// falls in, or MT: gemm_w4(x)[:r] is bit-identical to gemm_w4(x[:r]).
//
// Offsets into x and y are 32-bit element offsets (the launcher checks
// M*K and M*N against INT32_MAX); the W / scale bases are 64-bit.
//
// Resource usage (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage):
//   gemm_w4_kernel<4> (M > 64):   138 VGPRs, 0 AGPRs, 36864 B LDS, scratch 0,
//                                 occupancy 3 waves/SIMD
//   gemm_w4_kernel<2> (M <= 64):   86 VGPRs, 0 AGPRs, 18432 B LDS, scratch 0,
//                                 occupancy 5 waves/SIMD
//   gemm_w4_kernel<1> (M <= 32):   66 VGPRs, 0 AGPRs,  9216 B LDS, scratch 0,
//                                 occupancy 7 waves/SIMD
// The k loop's waits are counted (vmcnt(5)..vmcnt(2) ahead of the LDS
// writes, lgkmcnt(1..2) ahead of the MFMAs); the only vmcnt(0) is in the
// prologue.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"
#include "w4_dequant.h"

namespace {

constexpr int BLOCK = 256;        // 4 waves
constexpr int NWAVE = 4;          // n-blocks (of 32 W rows) per workgroup
constexpr int XSTRIDE = 64 + 8;   // LDS row stride in bf16: 144 B

typedef __attribute__((ext_vector_type(16))) float f32x16v;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4v;

template <int MT>
__global__ __launch_bounds__(BLOCK, 2) void gemm_w4_kernel(
    const uint16_t *__restrict__ x, const uint8_t *__restrict__ wq,
    const uint16_t *__restrict__ sc, uint16_t *__restrict__ y, int M, int N,
    int K) {
  // the only LDS object: x tiles of two consecutive groups
  __shared__ __attribute__((aligned(16))) uint16_t xl[2][MT * 32][XSTRIDE];

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int hi = lane >> 5;
  const int col = lane & 31;

  const int nblocks = N / 32;
  const int nblk = blockIdx.x * NWAVE + wid;
  const bool nvalid = nblk < nblocks;
  const int nblk_c = nvalid ? nblk : nblocks - 1;
  const int m0 = blockIdx.y * (MT * 32);
  const int G = K / 64;

  const uint8_t *wseg = wq + (int64_t)nblk_c * G * 1024 + lane * 16;
  const uint16_t *sseg = sc + (int64_t)nblk_c * G * 32 + col;

  // x staging: thread -> (row xr + 32 i, 16 B chunk xc) of the tile
  const int xr = tid >> 3;
  const int xc = (tid & 7) * 8;
  int xoff[MT];
  bool xok[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int row = m0 + xr + 32 * i;
    xok[i] = row < M;
    xoff[i] = min(row, M - 1) * K + xc;
  }

  f32x16v acc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) acc[i] = (f32x16v)(0.0f);

  u32x4v xv[MT];
  u32x4v w_cur, w_nxt, w_n2;
  uint16_t s_cur, s_nxt, s_n2;

#define RB_GW4_LOAD_X(G_)                                                \
  _Pragma("unroll") for (int i = 0; i < MT; ++i) {                       \
    xv[i] = *reinterpret_cast<const u32x4v *>(x + xoff[i] + (G_) * 64);  \
  }
#define RB_GW4_WRITE_X(BUF)                                              \
  _Pragma("unroll") for (int i = 0; i < MT; ++i) {                       \
    *reinterpret_cast<u32x4v *>(&xl[BUF][xr + 32 * i][xc]) =             \
        xok[i] ? xv[i] : (u32x4v)(0u);                                   \
  }
#define RB_GW4_LOAD_W(WB, SB, G_)                                        \
  WB = *reinterpret_cast<const u32x4v *>(wseg + (int64_t)(G_) * 1024);   \
  SB = sseg[(int64_t)(G_) * 32];

  // prologue: x(0) -> LDS buffer 0, x(1) in registers, W(0), W(1) loaded
  RB_GW4_LOAD_X(0);
  RB_GW4_LOAD_W(w_cur, s_cur, 0);
  RB_GW4_LOAD_W(w_nxt, s_nxt, min(1, G - 1));
  RB_GW4_WRITE_X(0);
  RB_GW4_LOAD_X(min(1, G - 1));
  __syncthreads();

  for (int g = 0; g < G; ++g) {
    const int buf = g & 1;
    RB_GW4_LOAD_W(w_n2, s_n2, min(g + 2, G - 1));

    const float s = rb::bf16_to_f32(s_cur);
    const float nb = -136.0f * s;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const rb::w4_bf16x8v a = rb::w4_dequant8(w_cur[j], s, nb);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const rb::w4_bf16x8v b = *reinterpret_cast<const rb::w4_bf16x8v *>(
            &xl[buf][mt * 32 + col][j * 16 + hi * 8]);
        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[mt], 0,
                                                          0, 0);
      }
    }

    // x(g+1) -> the other buffer (last read in iteration g-1, before the
    // barrier every wave has passed), then x(g+2) into the registers
    if (g + 1 < G) { RB_GW4_WRITE_X(buf ^ 1); }
    RB_GW4_LOAD_X(min(g + 2, G - 1));
    __syncthreads();
    w_cur = w_nxt; s_cur = s_nxt;
    w_nxt = w_n2; s_nxt = s_n2;
  }
#undef RB_GW4_LOAD_X
#undef RB_GW4_WRITE_X
#undef RB_GW4_LOAD_W

  // C[i = n][j = m]: lane column m, registers 4q..4q+3 = n 8q + 4hi + 0..3
  if (nvalid) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = m0 + mt * 32 + col;
      if (m < M) {
        uint16_t *yrow = y + m * N + nblk * 32 + 4 * hi;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          union { uint16_t u[4]; uint64_t v; } o;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            o.u[e] = rb::f32_to_bf16(acc[mt][4 * q + e]);
          *reinterpret_cast<uint64_t *>(yrow + 8 * q) = o.v;
        }
      }
    }
  }
}

template <int MT>
void launch(const at::Tensor &x, const at::Tensor &wq_swz,
            const at::Tensor &sc_swz, at::Tensor &y, int M, int N, int K) {
  const dim3 grid((N / 32 + NWAVE - 1) / NWAVE, (M + MT * 32 - 1) / (MT * 32));
  hipLaunchKernelGGL((gemm_w4_kernel<MT>), grid, dim3(BLOCK), 0,
                     at::cuda::getCurrentHIPStream(),
                     (const uint16_t *)x.data_ptr(),
                     (const uint8_t *)wq_swz.data_ptr(),
                     (const uint16_t *)sc_swz.data_ptr(),
                     (uint16_t *)y.data_ptr(), M, N, K);
}

}  // namespace

bool gemm_w4_supported(int64_t M, int64_t N, int64_t K) {
  return M >= 1 && N >= 32 && N % 32 == 0 && K >= 64 && K % 64 == 0 &&
         M * N <= INT32_MAX && M * K <= INT32_MAX && (M + 31) / 32 <= 65535;
}

// x [M, K] bf16 row-major; wq_swz / sc_swz from w4_swizzle; N, K of the
// quantized weight. y comes from the caching allocator; nothing here
// waits for the device.
at::Tensor gemm_w4(at::Tensor x, at::Tensor wq_swz, at::Tensor sc_swz,
                   int64_t N, int64_t K) {
  TORCH_CHECK(x.is_cuda() && wq_swz.is_cuda() && sc_swz.is_cuda() &&
              x.device() == wq_swz.device() && x.device() == sc_swz.device(),
              "gemm_w4: x, wq_swz and sc_swz must be on one GPU");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "gemm_w4: x must be bf16");
  TORCH_CHECK(wq_swz.scalar_type() == at::kByte &&
              sc_swz.scalar_type() == at::kBFloat16,
              "gemm_w4: wq_swz uint8, sc_swz bf16");
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous(),
              "gemm_w4: x must be a contiguous [M, K] matrix");
  TORCH_CHECK(wq_swz.is_contiguous() && sc_swz.is_contiguous(),
              "gemm_w4: contiguous weight tensors");
  const int64_t M = x.size(0);
  TORCH_CHECK(x.size(1) == K, "gemm_w4: x has K = ", x.size(1),
              ", weight has K = ", K);
  TORCH_CHECK(gemm_w4_supported(M, N, K), "gemm_w4: unsupported shape ", M,
              "x", N, "x", K);
  TORCH_CHECK(wq_swz.numel() == N * K / 2, "gemm_w4: wq_swz holds ",
              wq_swz.numel(), " bytes, N*K/2 = ", N * K / 2);
  TORCH_CHECK(sc_swz.numel() == N * (K / 64), "gemm_w4: sc_swz holds ",
              sc_swz.numel(), " scales, N*K/64 = ", N * (K / 64));

  auto y = at::empty({M, N}, x.options());
  if (M <= 32) {
    launch<1>(x, wq_swz, sc_swz, y, (int)M, (int)N, (int)K);
  } else if (M <= 64) {
    launch<2>(x, wq_swz, sc_swz, y, (int)M, (int)N, (int)K);
  } else {
    launch<4>(x, wq_swz, sc_swz, y, (int)M, (int)N, (int)K);
  }
  return y;
}
