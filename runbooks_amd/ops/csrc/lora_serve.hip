// Batched per-row LoRA for the decode step on CDNA4 (gfx950): every row
// of a decode batch may carry a different adapter (or none), picked by a
// slot index into preallocated per-site stacks (serve/lora.py).
//
//   lora_shrink   t[m, j]  = sum_k x[m, k] * a_stack[idx[m], j, k]
//   lora_expand_  y[m, n] += scales[idx[m]] *
//                            sum_j t[m, seg(n)*R + j] * b_stack[idx[m], n, j]
//
// A GEMM site has S segments (fused qkv 3, gate-up 2, o/down 1) that share
// the input x; a_stack stacks the segments' A matrices along rows, b_stack
// row n belongs to the segment that owns output column n.
//
// Both kernels are latency-shaped, not bandwidth-shaped: a whole llama2-7b
// r=16 adapter site is <= 1 MB and the batch has <= 32 rows. So the
// decomposition buys parallelism across (row, segment) / (row, column
// tile) and nothing else: no LDS, no atomics, no k split across
// workgroups, one fixed reduction order. Row m's result depends on row m
// alone, so it is bit-identical whatever the batch around it.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / RB_WAVE;

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4v;
typedef __attribute__((ext_vector_type(4))) float f32x4v;

// low / high bf16 of a packed pair, as f32
RB_DEV float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
RB_DEV float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// acc += dot(8 bf16 of a, 8 bf16 of b), products exact in f32
RB_DEV float dot8(u32x4v a, u32x4v b, float acc) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc = __builtin_fmaf(bf_lo(a[i]), bf_lo(b[i]), acc);
    acc = __builtin_fmaf(bf_hi(a[i]), bf_hi(b[i]), acc);
  }
  return acc;
}

// ---------------------------------------------------------------------------
// shrink: one workgroup per (row m, segment s); wave w owns outputs
// [w*NJ, (w+1)*NJ) of the segment's R = 16*R16 rows of A. Per k step a lane
// loads ONE 16 B chunk of x and NJ chunks of A (NJ+1 independent loads in
// flight), so x is read once per wave, not once per output. Lanes stride k
// by 512 elements; K % 8 == 0 makes every lane's chunk whole or absent.
// The 64 partial sums fold with the fixed xor-shuffle tree.
// ---------------------------------------------------------------------------
template <int R16>
__global__ __launch_bounds__(BLOCK) void lora_shrink_kernel(
    const uint16_t *__restrict__ x, const uint16_t *__restrict__ a_stack,
    const int *__restrict__ idx, float *__restrict__ t, int K, int S,
    int n_slots) {
  constexpr int R = 16 * R16;
  constexpr int NJ = R / WAVES;
  const int m = blockIdx.x;
  const int s = blockIdx.y;
  const int lane = (int)threadIdx.x & 63;
  const int wid = (int)threadIdx.x >> 6;
  const int slot = idx[m];
  float *trow = t + ((int64_t)m * S + s) * R + wid * NJ;

  if (slot < 0 || slot >= n_slots) {   // no adapter: zeros, A never read
    if (lane < NJ) trow[lane] = 0.0f;
    return;
  }
  const uint16_t *xr = x + (int64_t)m * K;
  const uint16_t *ar =
      a_stack + (((int64_t)slot * S + s) * R + wid * NJ) * (int64_t)K;

  float acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = 0.0f;

#pragma unroll 2
  for (int k = lane * 8; k < K; k += RB_WAVE * 8) {
    const u32x4v xv = *reinterpret_cast<const u32x4v *>(xr + k);
    u32x4v av[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      av[j] = *reinterpret_cast<const u32x4v *>(ar + (int64_t)j * K + k);
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = dot8(xv, av[j], acc[j]);
  }

  float mine = 0.0f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const float r = rb::wave_reduce_sum(acc[j]);   // same value on all lanes
    if (lane == j) mine = r;
  }
  if (lane < NJ) trow[lane] = mine;
}

// ---------------------------------------------------------------------------
// expand: one workgroup per (256-column tile, row m); each lane owns one
// whole column n: its b_stack row is 2*R contiguous bytes (R/8 16 B
// loads), adjacent lanes take adjacent rows, so a wave streams one
// contiguous 128*R byte span. The segment is picked per COLUMN (a
// boundary such as llama2-7b's gate-up 11008 falls inside a tile); the t
// segment is 4*R contiguous bytes that all lanes of a segment share.
// ---------------------------------------------------------------------------
template <int R16>
__global__ __launch_bounds__(BLOCK) void lora_expand_kernel(
    uint16_t *__restrict__ y, const float *__restrict__ t,
    const uint16_t *__restrict__ b_stack, const float *__restrict__ scales,
    const int *__restrict__ idx, int N, int S, int end0, int end1,
    int n_slots) {
  constexpr int R = 16 * R16;
  const int m = blockIdx.y;
  const int n = blockIdx.x * BLOCK + (int)threadIdx.x;
  const int slot = idx[m];
  if (slot < 0 || slot >= n_slots || n >= N) return;   // row left untouched

  // end0/end1 are N when the site has fewer segments
  const int s = (n >= end0) + (n >= end1);
  const uint16_t *br = b_stack + ((int64_t)slot * N + n) * R;
  const float *tr = t + ((int64_t)m * S + s) * R;
  uint16_t *yp = y + (int64_t)m * N + n;

  u32x4v bv[R / 8];
#pragma unroll
  for (int c = 0; c < R / 8; ++c)
    bv[c] = *reinterpret_cast<const u32x4v *>(br + c * 8);
  const float y0 = rb::bf16_to_f32(*yp);
  const float scale = scales[slot];

  float sum = 0.0f;
#pragma unroll
  for (int c = 0; c < R / 8; ++c) {
    const f32x4v t0 = *reinterpret_cast<const f32x4v *>(tr + c * 8);
    const f32x4v t1 = *reinterpret_cast<const f32x4v *>(tr + c * 8 + 4);
    sum = __builtin_fmaf(t0[0], bf_lo(bv[c][0]), sum);
    sum = __builtin_fmaf(t0[1], bf_hi(bv[c][0]), sum);
    sum = __builtin_fmaf(t0[2], bf_lo(bv[c][1]), sum);
    sum = __builtin_fmaf(t0[3], bf_hi(bv[c][1]), sum);
    sum = __builtin_fmaf(t1[0], bf_lo(bv[c][2]), sum);
    sum = __builtin_fmaf(t1[1], bf_hi(bv[c][2]), sum);
    sum = __builtin_fmaf(t1[2], bf_lo(bv[c][3]), sum);
    sum = __builtin_fmaf(t1[3], bf_hi(bv[c][3]), sum);
  }
  *yp = rb::f32_to_bf16(__builtin_fmaf(scale, sum, y0));
}

void check_idx(const at::Tensor &idx, int64_t M, const char *who) {
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == at::kInt &&
              idx.is_contiguous() && idx.dim() == 1 && idx.size(0) == M,
              who, ": idx must be a contiguous int32 GPU tensor [M]");
}

}  // namespace

// t[M, S*R] (fp32) = x[M, K] @ a_stack[idx[m]]^T; rows with idx < 0 get
// zeros. a_stack bf16 [n_slots, S*R, K]; R in {16, 32, 48, 64}.
at::Tensor lora_shrink(at::Tensor x, at::Tensor a_stack, at::Tensor idx,
                       int64_t S) {
  TORCH_CHECK(x.is_cuda() && a_stack.is_cuda() && x.is_contiguous() &&
              a_stack.is_contiguous(), "lora_shrink: contiguous GPU tensors");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
              a_stack.scalar_type() == at::kBFloat16, "lora_shrink: bf16");
  TORCH_CHECK(x.dim() == 2 && a_stack.dim() == 3, "lora_shrink: x [M, K], "
              "a_stack [n_slots, S*R, K]");
  const int64_t M = x.size(0), K = x.size(1);
  const int64_t SR = a_stack.size(1);
  TORCH_CHECK(S >= 1 && S <= 3 && SR % S == 0, "lora_shrink: S in 1..3 "
              "dividing a_stack rows");
  const int64_t R = SR / S;
  TORCH_CHECK(R % 16 == 0 && R >= 16 && R <= 64,
              "lora_shrink: pool rank must be 16, 32, 48 or 64, got ", R);
  TORCH_CHECK(a_stack.size(2) == K && K % 8 == 0 && K < (1 << 30),
              "lora_shrink: K must match a_stack and be a multiple of 8");
  TORCH_CHECK(a_stack.size(0) >= 1 && M < (1LL << 31), "lora_shrink: sizes");
  check_idx(idx, M, "lora_shrink");
  auto t = at::empty({M, SR}, x.options().dtype(at::kFloat));
  if (M == 0) return t;
  auto stream = at::cuda::getCurrentHIPStream();
  const dim3 grid((unsigned)M, (unsigned)S);
#define RB_SHRINK(R16V)                                                   \
  hipLaunchKernelGGL((lora_shrink_kernel<R16V>), grid, dim3(BLOCK), 0,    \
                     stream, (const uint16_t *)x.data_ptr(),              \
                     (const uint16_t *)a_stack.data_ptr(),                \
                     (const int *)idx.data_ptr(), (float *)t.data_ptr(),  \
                     (int)K, (int)S, (int)a_stack.size(0))
  switch (R / 16) {
    case 1: RB_SHRINK(1); break;
    case 2: RB_SHRINK(2); break;
    case 3: RB_SHRINK(3); break;
    default: RB_SHRINK(4); break;
  }
#undef RB_SHRINK
  return t;
}

// In place on bf16 y[M, N]; rows with idx < 0 are not written. seg_ends:
// 1..3 ascending column ends, the last equal to N.
at::Tensor lora_expand_(at::Tensor y, at::Tensor t, at::Tensor b_stack,
                        at::Tensor scales, at::Tensor idx,
                        std::vector<int64_t> seg_ends) {
  TORCH_CHECK(y.is_cuda() && t.is_cuda() && b_stack.is_cuda() &&
              scales.is_cuda() && y.is_contiguous() && t.is_contiguous() &&
              b_stack.is_contiguous() && scales.is_contiguous(),
              "lora_expand_: contiguous GPU tensors");
  TORCH_CHECK(y.scalar_type() == at::kBFloat16 &&
              b_stack.scalar_type() == at::kBFloat16 &&
              t.scalar_type() == at::kFloat &&
              scales.scalar_type() == at::kFloat,
              "lora_expand_: y, b_stack bf16; t, scales fp32");
  TORCH_CHECK(y.dim() == 2 && t.dim() == 2 && b_stack.dim() == 3 &&
              scales.dim() == 1, "lora_expand_: y [M, N], t [M, S*R], "
              "b_stack [n_slots, N, R], scales [n_slots]");
  const int64_t M = y.size(0), N = y.size(1);
  const int64_t S = (int64_t)seg_ends.size();
  const int64_t R = b_stack.size(2);
  TORCH_CHECK(S >= 1 && S <= 3, "lora_expand_: 1..3 segments");
  int64_t prev = 0;
  for (int64_t e : seg_ends) {
    TORCH_CHECK(e > prev, "lora_expand_: seg_ends must ascend");
    prev = e;
  }
  TORCH_CHECK(prev == N, "lora_expand_: last seg_end must equal N");
  TORCH_CHECK(N % 8 == 0 && N < (1 << 30), "lora_expand_: N % 8 == 0");
  TORCH_CHECK(R % 16 == 0 && R >= 16 && R <= 64,
              "lora_expand_: pool rank must be 16, 32, 48 or 64, got ", R);
  TORCH_CHECK(b_stack.size(1) == N && t.size(0) == M && t.size(1) == S * R &&
              scales.size(0) == b_stack.size(0) && b_stack.size(0) >= 1 &&
              M <= 65535, "lora_expand_: shape mismatch");
  check_idx(idx, M, "lora_expand_");
  if (M == 0) return y;
  const int end0 = S > 1 ? (int)seg_ends[0] : (int)N;
  const int end1 = S > 2 ? (int)seg_ends[1] : (int)N;
  auto stream = at::cuda::getCurrentHIPStream();
  const dim3 grid((unsigned)((N + BLOCK - 1) / BLOCK), (unsigned)M);
#define RB_EXPAND(R16V)                                                   \
  hipLaunchKernelGGL((lora_expand_kernel<R16V>), grid, dim3(BLOCK), 0,    \
                     stream, (uint16_t *)y.data_ptr(),                    \
                     (const float *)t.data_ptr(),                         \
                     (const uint16_t *)b_stack.data_ptr(),                \
                     (const float *)scales.data_ptr(),                    \
                     (const int *)idx.data_ptr(), (int)N, (int)S, end0,   \
                     end1, (int)b_stack.size(0))
  switch (R / 16) {
    case 1: RB_EXPAND(1); break;
    case 2: RB_EXPAND(2); break;
    case 3: RB_EXPAND(3); break;
    default: RB_EXPAND(4); break;
  }
#undef RB_EXPAND
  return y;
}
