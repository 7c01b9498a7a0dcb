// fp8 (OCP e4m3) weight-only MFMA GEMM for CDNA4 (gfx950), any M:
//   y[M,N] = bf16_rne( scale[n] * sum_k x[m,k] * e4m3(W8[n,k]) ),
// x bf16 [M,K] row-major, y bf16 [M,N], fp32 accumulate, f32 per-output-
// channel scale. The large-M companion of decode_gemm_w8.hip (M <= 32):
// prefill, chunked and batched prefill, the T*B rows of a speculative
// verify and decode at B > 32 of a MODEL_LOAD_IN_8BIT model run here, so
// such a model needs no bf16 master weights (ops/linear.py
// release_w8_placeholder, models/transformer.py release_w8_masters).
//
// Operands: the SAME stored copy the decode kernel streams, w8_swz
// [N/32][K/32][64 lanes][16 B] exactly as w8_swizzle builds it (layout:
// decode_gemm_w8.hip header) and the canonical f32 scale [N]; x as plain
// row-major rows. N % 32 == 0, K % 64 == 0 (the decode kernel also takes
// K % 64 == 32; such a weight keeps its master). Weights are converted at
// use by w8_dequant.h, the decode kernel's expressions, and the scale is
// applied once to the fp32 sum, then one RNE: the decode kernel's
// expression and rounding point.
//
// Structure (A = W, so C columns = m; fragment maps: mfma_frag.h):
//  * k-group: one pipeline unit is 64 k = two adjacent w8 blocks = two
//    16 B loads per lane (2 KiB contiguous per wave, nontemporal) = four
//    mfma_f32_32x32x16_bf16 k-steps in ascending k: block 2g bytes 0..7,
//    bytes 8..15, then block 2g+1 the same.
//  * the x tile of one group ([MT*32][64] bf16) is staged through LDS by
//    the whole workgroup in full 128 B lines (8 lanes x 16 B per row),
//    double-buffered, rows padded to 144 B: the B-fragment ds_read_b128
//    of 16 consecutive rows then lands on 16 distinct 16 B bank slots
//    (gemm_w4.hip's image).
//  * both streams are software-pipelined through registers: W two groups
//    ahead, x one group ahead in registers + one in LDS; one barrier per
//    group. Loads past the last group re-read the last group (in bounds,
//    unused) instead of branching around the load.
//  * rows >= M of a ragged m-tile are never loaded: their address is
//    clamped to row M-1 and zeros are written to LDS in their place. A
//    wave whose n-block is past N/32 (ragged n-tile) streams the last
//    valid block and stores nothing.
//  * the four float4 of scales a lane's accumulator rows need (registers
//    4q..4q+3 = n 32*nblk + 8q + 4*hi + 0..3) are loaded before the k
//    loop and are long home when the epilogue multiplies.
//
// Two workgroup forms, one body, template <MT, NBW>: a workgroup of 4
// waves covers NBW n-blocks x MT m-tiles; 4/NBW waves share one n-block
// and deal its MT m-tiles among themselves.
//  * wide, NBW = 4: one n-block x all MT m-tiles per wave (gemm_w4's
//    split). Every weight is converted once per MT*32 x-rows. Grid
//    (ceil(N/128), ceil(M/(32 MT))).
//  * narrow, NBW = 4/MT: MT = 4 -> one n-block per workgroup, one m-tile
//    per wave; MT = 2 -> two n-blocks x two waves. The waves of an n-block
//    load and convert the same W fragments: one HBM read, the rest from
//    cache, up to 4x redundant conversion, which fp8's one VALU op per
//    weight affords. MT x as many workgroups on the same shared x image,
//    for shapes whose wide grid underfills the chip (N = 4096, M <= 128:
//    32 workgroups on 256 CUs). At MT = 1 the forms coincide.
//
// Determinism / row independence: no k-split, no atomics. In both forms
// an output element is one accumulator column fed k = 0, 16, 32, ... in
// order, so its summation order depends on K alone, never on M, the tile
// a row falls in, MT or the form: gemm_w8(x)[:r] is bit-identical to
// gemm_w8(x[:r]), and the forms are bit-identical to each other.
//
// Offsets into x and y are 32-bit element offsets (the launcher checks
// M*K and M*N against INT32_MAX); the W base is 64-bit.
//
// Resource usage (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage),
// <MT, NBW>; no AGPRs and no scratch anywhere:
//   <4, 4> wide,   M > 64:  152 VGPRs, 36864 B LDS, 3 waves/SIMD
//   <4, 1> narrow, M > 64:   98 VGPRs, 36864 B LDS, 4 waves/SIMD
//   <2, 4> wide,   M <= 64: 100 VGPRs, 18432 B LDS, 4 waves/SIMD
//   <2, 2> narrow, M <= 64:  87 VGPRs, 18432 B LDS, 5 waves/SIMD
//   <1, 4>         M <= 32:  82 VGPRs,  9216 B LDS, 5 waves/SIMD
// The k loop's waits are counted (vmcnt(2..4) ahead of the LDS writes,
// lgkmcnt(0..2) ahead of the MFMAs); the only vmcnt(0) is in the prologue.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"
#include "w8_dequant.h"

namespace {

constexpr int BLOCK = 256;        // 4 waves
constexpr int NWAVE = 4;
constexpr int XSTRIDE = 64 + 8;   // LDS row stride in bf16: 144 B
constexpr int NUM_CU = 256;       // MI355X

typedef __attribute__((ext_vector_type(16))) float f32x16v;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4v;

template <int MT, int NBW>
RB_W8_NO_PK __global__ __launch_bounds__(BLOCK, 2) void gemm_w8_kernel(
    const uint16_t *__restrict__ x, const uint8_t *__restrict__ w8,
    const float *__restrict__ scale, uint16_t *__restrict__ y, int M, int N,
    int K) {
  constexpr int WPN = NWAVE / NBW;   // waves sharing one n-block
  constexpr int MTW = MT / WPN;      // m-tiles per wave
  static_assert(NBW * WPN == NWAVE && MTW * WPN == MT, "wave tiling");

  // the only LDS object: x tiles of two consecutive groups
  __shared__ __attribute__((aligned(16))) uint16_t xl[2][MT * 32][XSTRIDE];

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int hi = lane >> 5;
  const int col = lane & 31;

  const int nblocks = N / 32;
  const int nblk = blockIdx.x * NBW + wid / WPN;
  const bool nvalid = nblk < nblocks;
  const int nblk_c = nvalid ? nblk : nblocks - 1;
  const int mt0 = (wid % WPN) * MTW;      // this wave's first m-tile
  const int m0 = blockIdx.y * (MT * 32);
  const int G = K / 64;

  const uint8_t *wseg = w8 + (int64_t)nblk_c * G * 2048 + lane * 16;

  // accumulator registers 4q..4q+3 <-> output channels 8q + 4hi + 0..3
  float4 sc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    sc[q] = *reinterpret_cast<const float4 *>(scale + nblk_c * 32 + 8 * q +
                                              4 * hi);

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

  f32x16v acc[MTW];
#pragma unroll
  for (int i = 0; i < MTW; ++i) acc[i] = (f32x16v)(0.0f);

  u32x4v xv[MT];
  u32x4v w_cur[2], w_nxt[2], w_n2[2];

#define RB_GW8_LOAD_X(G_)                                                \
  _Pragma("unroll") for (int i = 0; i < MT; ++i) {                       \
    xv[i] = *reinterpret_cast<const u32x4v *>(x + xoff[i] + (G_) * 64);  \
  }
#define RB_GW8_WRITE_X(BUF)                                              \
  _Pragma("unroll") for (int i = 0; i < MT; ++i) {                       \
    *reinterpret_cast<u32x4v *>(&xl[BUF][xr + 32 * i][xc]) =             \
        xok[i] ? xv[i] : (u32x4v)(0u);                                   \
  }
#define RB_GW8_LOAD_W(WB, G_)                                            \
  _Pragma("unroll") for (int b = 0; b < 2; ++b) {                        \
    WB[b] = __builtin_nontemporal_load(reinterpret_cast<const u32x4v *>( \
        wseg + (int64_t)(G_) * 2048 + b * 1024));                        \
  }

  // prologue: x(0) -> LDS buffer 0, x(1) in registers, W(0), W(1) loaded
  RB_GW8_LOAD_X(0);
  RB_GW8_LOAD_W(w_cur, 0);
  RB_GW8_LOAD_W(w_nxt, min(1, G - 1));
  RB_GW8_WRITE_X(0);
  RB_GW8_LOAD_X(min(1, G - 1));
  __syncthreads();

  for (int g = 0; g < G; ++g) {
    const int buf = g & 1;
    RB_GW8_LOAD_W(w_n2, min(g + 2, G - 1));

#pragma unroll
    for (int j = 0; j < 4; ++j) {
      // k-step j: k = 64 g + 16 j + 8 hi + 0..7
      const rb::w8_bf16x8v a = rb::w8_dequant8(w_cur[j >> 1][2 * (j & 1)],
                                               w_cur[j >> 1][2 * (j & 1) + 1]);
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt) {
        const rb::w8_bf16x8v b = *reinterpret_cast<const rb::w8_bf16x8v *>(
            &xl[buf][(mt0 + mt) * 32 + col][j * 16 + hi * 8]);
        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[mt], 0,
                                                          0, 0);
      }
    }

    // x(g+1) -> the other buffer (last read in iteration g-1, before the
    // barrier every wave has passed), then x(g+2) into the registers
    if (g + 1 < G) { RB_GW8_WRITE_X(buf ^ 1); }
    RB_GW8_LOAD_X(min(g + 2, G - 1));
    __syncthreads();
    w_cur[0] = w_nxt[0]; w_cur[1] = w_nxt[1];
    w_nxt[0] = w_n2[0]; w_nxt[1] = w_n2[1];
  }
#undef RB_GW8_LOAD_X
#undef RB_GW8_WRITE_X
#undef RB_GW8_LOAD_W

  // C[i = n][j = m]: lane column m, registers 4q..4q+3 = n 8q + 4hi + 0..3
  if (nvalid) {
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) {
      const int m = m0 + (mt0 + mt) * 32 + col;
      if (m < M) {
        uint16_t *yrow = y + m * N + nblk * 32 + 4 * hi;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          union { uint16_t u[4]; uint64_t v; } o;
          o.u[0] = rb::f32_to_bf16(acc[mt][4 * q + 0] * sc[q].x);
          o.u[1] = rb::f32_to_bf16(acc[mt][4 * q + 1] * sc[q].y);
          o.u[2] = rb::f32_to_bf16(acc[mt][4 * q + 2] * sc[q].z);
          o.u[3] = rb::f32_to_bf16(acc[mt][4 * q + 3] * sc[q].w);
          *reinterpret_cast<uint64_t *>(yrow + 8 * q) = o.v;
        }
      }
    }
  }
}

template <int MT, int NBW>
void launch(const at::Tensor &x, const at::Tensor &w8_swz,
            const at::Tensor &scale, at::Tensor &y, int M, int N, int K) {
  const dim3 grid((N / 32 + NBW - 1) / NBW, (M + MT * 32 - 1) / (MT * 32));
  hipLaunchKernelGGL((gemm_w8_kernel<MT, NBW>), grid, dim3(BLOCK), 0,
                     at::cuda::getCurrentHIPStream(),
                     (const uint16_t *)x.data_ptr(),
                     (const uint8_t *)w8_swz.data_ptr(),
                     (const float *)scale.data_ptr(),
                     (uint16_t *)y.data_ptr(), M, N, K);
}

// m-tiles per workgroup: 1 / 2 / 4 for M <= 32 / <= 64 / larger
int m_tiles(int64_t M) { return M <= 32 ? 1 : M <= 64 ? 2 : 4; }

}  // namespace

bool gemm_w8_supported(int64_t M, int64_t N, int64_t K) {
  return M >= 1 && N >= 32 && N % 32 == 0 && K >= 64 && K % 64 == 0 &&
         M * N <= INT32_MAX && M * K <= INT32_MAX && (M + 31) / 32 <= 65535;
}

// Workgroup form for an [M, N] output: 0 = wide, 1 = narrow. A function of
// (M, N) alone: narrow while the wide grid cannot cover the CUs. Measured
// on the five llama2-7b shapes at M = 33..2048 (profiles/README.md,
// "gemm_w8"): at MT = 2 (2x redundant conversion) narrow won every cell,
// up to 250 wide workgroups; at MT = 4 (4x) it won by 15-31 % at 32..128
// wide workgroups, by 2 % at 172 and 192, and lost by 25 % at 250, so
// there it is taken only up to three quarters of the CUs. Every cell of
// 256 or more wide workgroups went to wide, by 1.5-2x.
int64_t gemm_w8_form(int64_t M, int64_t N) {
  const int mt = m_tiles(M);
  if (mt == 1) return 0;               // the forms coincide
  const int64_t wide_wgs = ((N + 127) / 128) * ((M + 32 * mt - 1) / (32 * mt));
  if (mt == 2) return wide_wgs < NUM_CU ? 1 : 0;
  return wide_wgs * 4 <= NUM_CU * 3 ? 1 : 0;
}

// x [M, K] bf16 row-major; w8_swz from w8_swizzle, scale the canonical f32
// [N]; N, K of the quantized weight. form: -1 = gemm_w8_form's choice,
// 0 = wide, 1 = narrow (same bits either way). y comes from the caching
// allocator; nothing here waits for the device.
at::Tensor gemm_w8(at::Tensor x, at::Tensor w8_swz, at::Tensor scale,
                   int64_t N, int64_t K, int64_t form) {
  TORCH_CHECK(x.is_cuda() && w8_swz.is_cuda() && scale.is_cuda() &&
              x.device() == w8_swz.device() && x.device() == scale.device(),
              "gemm_w8: x, w8_swz and scale must be on one GPU");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "gemm_w8: x must be bf16");
  TORCH_CHECK(w8_swz.scalar_type() == at::kByte &&
              scale.scalar_type() == at::kFloat,
              "gemm_w8: w8_swz uint8, scale f32");
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous(),
              "gemm_w8: x must be a contiguous [M, K] matrix");
  TORCH_CHECK(w8_swz.is_contiguous() && scale.is_contiguous(),
              "gemm_w8: contiguous weight tensors");
  TORCH_CHECK(form >= -1 && form <= 1, "gemm_w8: form is -1, 0 or 1");
  const int64_t M = x.size(0);
  TORCH_CHECK(x.size(1) == K, "gemm_w8: x has K = ", x.size(1),
              ", weight has K = ", K);
  TORCH_CHECK(gemm_w8_supported(M, N, K), "gemm_w8: unsupported shape ", M,
              "x", N, "x", K);
  TORCH_CHECK(w8_swz.numel() == N * K, "gemm_w8: w8_swz holds ",
              w8_swz.numel(), " bytes, N*K = ", N * K);
  TORCH_CHECK(scale.numel() == N, "gemm_w8: scale holds ", scale.numel(),
              " values, N = ", N);

  auto y = at::empty({M, N}, x.options());
  const bool narrow = (form < 0 ? gemm_w8_form(M, N) : form) == 1;
  const int mt = m_tiles(M);
  if (mt == 1) {
    launch<1, 4>(x, w8_swz, scale, y, (int)M, (int)N, (int)K);
  } else if (mt == 2) {
    if (narrow) launch<2, 2>(x, w8_swz, scale, y, (int)M, (int)N, (int)K);
    else launch<2, 4>(x, w8_swz, scale, y, (int)M, (int)N, (int)K);
  } else {
    if (narrow) launch<4, 1>(x, w8_swz, scale, y, (int)M, (int)N, (int)K);
    else launch<4, 4>(x, w8_swz, scale, y, (int)M, (int)N, (int)K);
  }
  return y;
}
