// M-tiled weight-stream GEMM for CDNA4 (gfx950): y[M,N] = x[M,K] @ W[N,K]^T
// for 32 < M <= 256 (speculative verify, decode at B > 32, short prompt
// chunks), bf16 in / bf16 out, fp32 accumulate.
//
// These row counts are as weight-bound as decode: one 32-row W fragment
// (1 KiB per wave instruction) feeds MT = ceil(M/32) MFMAs, and even at
// MT = 8 the matrix cores need about half the time the weights take to
// arrive. So the kernel keeps decode_gemm.hip's skeleton and reads the SAME
// swizzled weight copy ([N/32][K/16][lane][8], decode_swizzle_w(_layout)):
//
//  * one workgroup = one 32-row n-block x one k-slice, 4 waves on adjacent
//    k-quarters, wave ranges from the same spg / s0 / s1 arithmetic, the
//    cross-WG split from decode_gemm_split(N, K) (no dependence on M);
//  * k-steps ascend within a wave into one f32x16 accumulator per m-tile,
//    the 4 waves are summed red[0]+red[1]+red[2]+red[3], split > 1 goes
//    through fp32 slabs [split, M, N] and decode_gemm_combine_kernel.
//
// Every output's summation order is therefore a function of (N, K) alone:
// row r is bit-identical to row r of decode_gemm on any 32 rows holding it,
// and to row r of this kernel at any other M.
//
// Operand: decode_swizzle_x_mt turns the row-major x into
// [K/16][MT][64][8]; tile t of step s is rows 32t..32t+31 in the B-fragment
// lane order of decode_swizzle_x_kernel (rows >= M zero), so a wave's x for
// one k-step is MT contiguous KiB. x is re-read from L2 by every n-block
// (plain loads); W is streamed once (nontemporal loads).
//
// Registers: loads return in issue order, so a wait for an x fragment
// is also a wait for every W fragment requested before it: a W ring deeper
// than the x ring buys nothing (a first cut with decode_gemm's 2 x 8 W ring
// and x one step ahead exposed the L2 latency at every k-step and lost to
// hipBLASLt on every shape, docs/kernels.md). Both streams therefore share
// ONE ring of DX k-steps, DX * (1 + MT) ~ 48 raw 16 B fragments: 16 steps
// at MT = 2 (decode_gemm's 16 KiB of W in flight per wave), 5 at MT = 8.
//
// Reduce: the 4 waves' accumulators of ONE m-tile go through a 16 KiB LDS
// image, two images alternating so that each m-tile costs one barrier.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"
#include "decode_gemm_common.h"

int64_t decode_gemm_split(int64_t N, int64_t K);
bool decode_gemm_supported(int64_t M, int64_t N, int64_t K);

namespace {

constexpr int BLOCK = 256;   // 4 waves
constexpr int MT_MAX = 8;    // M <= 256

// The device code of this file is built without packed fp32 instructions
// (the 4-wave sums below would otherwise pair up into v_pk_add_f32). A
// function with its own target features only inlines always_inline callees,
// so the kernels use builtins and forceinline helpers, nothing else.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                          \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

typedef __attribute__((ext_vector_type(4))) float f32x4v;

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }

// __syncthreads() spelled out
__device__ __forceinline__ void wg_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// k-steps in flight per wave: DX * (1 + MT) fragments of 16 B per lane, about
// 48 (192 VGPRs), and at most the 63 loads a counted vmcnt wait can name.
template <int MT> struct Depth {
  static constexpr int DX = MT == 2 ? 16 : MT == 3 ? 12 : MT <= 5 ? 8
                          : MT <= 7 ? 6 : 5;
};

// Slot U of the ring <- k-step S: the W fragment (nontemporal) and the MT x
// fragments (plain: every n-block re-reads them from L2).
#define RB_MT_LOAD(U_, S)                                              \
  {                                                                    \
    const int64_t st_ = (S);                                           \
    wr[U_] = nt_load8v(wseg + st_ * 512 + lane8);                      \
    _Pragma("unroll") for (int t = 0; t < MT; ++t) {                   \
      xr[U_][t] = load8v(xs + (st_ * MT + t) * 512 + lane8);           \
    }                                                                  \
  }

#define RB_MT_MFMA(U_)                                                 \
  _Pragma("unroll") for (int t = 0; t < MT; ++t) {                     \
    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(                  \
        wr[U_], xr[U_][t], acc[t], 0, 0, 0);                           \
  }

// slabs == nullptr: write y bf16 directly (split == 1). Otherwise store the
// fp32 slab slice at slabs + kslice*M*N for decode_gemm_combine_kernel.
// layout picks the un-permuting column map (epi_col) at the store.
template <int MT>
__global__ __launch_bounds__(BLOCK) void decode_gemm_mt_kernel(
    const uint16_t *__restrict__ xs, const uint16_t *__restrict__ ws,
    uint16_t *__restrict__ yp, float *__restrict__ slabs,
    int M, int N, int K, int split, int layout, const EpiArgs ep) {
  constexpr int DX = Depth<MT>::DX;
  const int tid = __builtin_amdgcn_workitem_id_x();
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int hi = lane >> 5;
  const int col = lane & 31;
  const int lane8 = lane * 8;

  const int nblk = __builtin_amdgcn_workgroup_id_x();   // 32 W rows per WG
  const int kslice = __builtin_amdgcn_workgroup_id_y();  // of `split`

  // the partition of decode_gemm_kernel: k-step range of this (kslice,
  // wave) group; s1 - s0 may be <= 0 (an empty wave adds +0 to the reduce,
  // there as here)
  const int steps_total = K / 16;
  const int ngroups = split * 4;
  const int spg = (steps_total + ngroups - 1) / ngroups;
  const int g = kslice * 4 + __builtin_amdgcn_readfirstlane(wid);
  const int s0 = g * spg;
  const int s1 = imin(steps_total, s0 + spg);
  const int slast = s1 - 1;

  const uint16_t *wseg = ws + (int64_t)nblk * steps_total * 512;

  f32x16v acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = (f32x16v)(0.0f);

  // One software pipeline for both streams: slot u holds k-step s + u, and
  // is refilled with step s + u + DX as soon as its MFMAs are issued. The
  // step index is clamped to the wave's last step, so every round issues
  // the same DX * (1 + MT) loads (counted vmcnt waits, no drain), nothing
  // outside [s0, s1) is read, and the repeats re-request one line. A step
  // that does not exist is branched over, never fed a zero operand.
  if (s0 < s1) {
    bf16x8v wr[DX], xr[DX][MT];
#pragma unroll
    for (int u = 0; u < DX; ++u) RB_MT_LOAD(u, imin(s0 + u, slast));
    int s = s0;
    for (; s + DX <= s1; s += DX) {
#pragma unroll
      for (int u = 0; u < DX; ++u) {
        RB_MT_MFMA(u);
        RB_MT_LOAD(u, imin(s + u + DX, slast));
      }
    }
    const int rem = s1 - s;              // < DX, wave-uniform
#pragma unroll
    for (int u = 0; u < DX; ++u) {
      if (u < rem) RB_MT_MFMA(u);
    }
  }

  // ---- cross-wave reduction in LDS, one m-tile per pass ------------------
  // Pass t writes image t & 1; a wave that runs ahead into pass t + 1
  // writes the other image, whose readers (pass t - 1) all passed the
  // barrier of pass t. The per-element order is that of RB_RED_BF16.
  __shared__ __attribute__((aligned(16))) float red[2][4][32][32];
  const int em = tid >> 3;               // 0..31: row inside the m-tile
  const int en = (tid & 7) * 4;          // 0,4,..,28: local W row
  int ycol;
  if (layout == LAYOUT_GLU16)
    ycol = epi_col<EPI_GLU_STORE>(nblk, en, ep);
  else if (layout == LAYOUT_ROPE16)
    ycol = epi_col<EPI_ROPE_STORE>(nblk, en, ep);
  else
    ycol = epi_col<EPI_PLAIN>(nblk, en, ep);
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    float (*img)[32][32] = red[t & 1];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n_local = (r & 3) + 8 * (r >> 2) + 4 * hi;
      img[wid][n_local][col] = acc[t][r];
    }
    wg_barrier();
    const int row = t * 32 + em;
    if (row < M) {
      float sum[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sum[j] = img[0][en + j][em] + img[1][en + j][em] +
                 img[2][en + j][em] + img[3][en + j][em];
      }
      if (slabs == nullptr) {
        union { uint16_t u[4]; uint64_t q; } o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o.u[j] = rb::f32_to_bf16(sum[j]);
        *reinterpret_cast<uint64_t *>(yp + (int64_t)row * N + ycol) = o.q;
      } else {
        float *slab = slabs + ((int64_t)kslice * M + row) * N + ycol;
        f32x4v o;
        o[0] = sum[0]; o[1] = sum[1]; o[2] = sum[2]; o[3] = sum[3];
        *reinterpret_cast<f32x4v *>(slab) = o;
      }
    }
  }
}

// x [M, K] row-major -> xs [K/16][MT][64 lanes][8] bf16: tile t of step s
// in B-fragment lane order (lane = hi*32 + m, elems = x[32t + m][s*16 +
// hi*8 + i]; zeros for rows >= M).
__global__ void decode_swizzle_x_mt_kernel(
    const uint16_t *__restrict__ xp, uint16_t *__restrict__ xs,
    int M, int K, int MT, int nblocks) {
  const int64_t total = (int64_t)(K / 16) * MT * 64;
  // 256 threads per block, `nblocks` blocks (builtins only, see above)
  const int64_t stride = (int64_t)nblocks * 256;
  for (int64_t idx = (int64_t)__builtin_amdgcn_workgroup_id_x() * 256 +
                     __builtin_amdgcn_workitem_id_x();
       idx < total; idx += stride) {
    const int l = (int)(idx & 63);
    const int64_t st = idx >> 6;
    const int t = (int)(st % MT);
    const int s = (int)(st / MT);
    const int m = t * 32 + (l & 31);
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

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

template <int MT>
void launch_mt(const dim3 &grid, hipStream_t stream, const at::Tensor &xs,
               const at::Tensor &ws, uint16_t *y, float *slabs, int64_t M,
               int64_t N, int64_t K, int64_t layout, const EpiArgs &ep) {
  hipLaunchKernelGGL((decode_gemm_mt_kernel<MT>), grid, dim3(BLOCK), 0,
                     stream, (const uint16_t *)xs.data_ptr(),
                     (const uint16_t *)ws.data_ptr(), y, slabs, (int)M, (int)N,
                     (int)K, (int)grid.y, (int)layout, ep);
}

void check_x(const at::Tensor &x, const char *who) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous(), who,
              ": x must be a contiguous GPU [M,K] tensor");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, who, ": bf16 only");
}

}  // namespace

bool decode_gemm_mt_supported(int64_t M, int64_t N, int64_t K) {
  return M > 32 && M <= 32 * MT_MAX && decode_gemm_supported(32, N, K);
}

at::Tensor decode_swizzle_x_mt(at::Tensor x) {
  check_x(x, "decode_swizzle_x_mt");
  const int64_t M = x.size(0), K = x.size(1);
  TORCH_CHECK(M >= 1 && M <= 32 * MT_MAX && K >= 16 && K % 16 == 0,
              "decode_swizzle_x_mt: unsupported shape ", M, "x", K);
  const int64_t MT = (M + 31) / 32;
  auto xs = at::empty({(K / 16) * MT * 512}, x.options());
  const int grid = rb::rb_grid_1d((K / 16) * MT * 64, 256);
  hipLaunchKernelGGL(decode_swizzle_x_mt_kernel, dim3(grid), dim3(256), 0,
                     at::cuda::getCurrentHIPStream(),
                     (const uint16_t *)x.data_ptr(), (uint16_t *)xs.data_ptr(),
                     (int)M, (int)K, (int)MT, grid);
  return xs;
}

// x [M,K] row-major bf16, 32 < M <= 256; ws from decode_swizzle_w(_layout)
// for an [n,k] weight. y is row-major in the original column order
// whatever the weight layout.
at::Tensor decode_gemm_mt(at::Tensor x, at::Tensor ws, int64_t n, int64_t k,
                          int64_t layout, int64_t hq, int64_t hkv, int64_t dh,
                          int64_t force_split) {
  check_x(x, "decode_gemm_mt");
  TORCH_CHECK(ws.is_cuda() && ws.is_contiguous() &&
              ws.scalar_type() == at::kBFloat16 &&
              ws.device() == x.device(),
              "decode_gemm_mt: ws must be a contiguous bf16 tensor on x's GPU");
  const int64_t M = x.size(0);
  TORCH_CHECK(x.size(1) == k, "decode_gemm_mt: x has K = ", x.size(1),
              ", weight has ", k);
  TORCH_CHECK(decode_gemm_mt_supported(M, n, k),
              "decode_gemm_mt: unsupported shape ", M, "x", n, "x", k);
  TORCH_CHECK(ws.numel() == n * k, "decode_gemm_mt: ws size");
  TORCH_CHECK(force_split <= 8, "decode_gemm_mt: force_split <= 8");
  const EpiArgs ep = layout_args(layout, n, hq, hkv, dh);

  auto xs = decode_swizzle_x_mt(x);
  auto stream = at::cuda::getCurrentHIPStream();
  auto y = at::empty({M, n}, x.options());
  const int split = force_split > 0 ? (int)force_split
                                    : (int)decode_gemm_split(n, k);
  at::Tensor slabs;
  float *sp = nullptr;
  if (split > 1) {
    slabs = at::empty({split, M, n}, x.options().dtype(at::kFloat));
    sp = (float *)slabs.data_ptr();
  }
  uint16_t *yp = split > 1 ? nullptr : (uint16_t *)y.data_ptr();
  const dim3 grid(n / 32, split);
  switch ((M + 31) / 32) {
#define RB_MT_CASE(MT_)                                                \
  case MT_:                                                            \
    launch_mt<MT_>(grid, stream, xs, ws, yp, sp, M, n, k, layout, ep); \
    break;
    RB_MT_CASE(2) RB_MT_CASE(3) RB_MT_CASE(4) RB_MT_CASE(5)
    RB_MT_CASE(6) RB_MT_CASE(7) RB_MT_CASE(8)
#undef RB_MT_CASE
    default:
      TORCH_CHECK(false, "decode_gemm_mt: no instantiation for M = ", M);
  }
  if (split > 1) {
    rb::dg_combine(sp, (uint16_t *)y.data_ptr(), split, M * n, stream);
  }
  return y;
}
