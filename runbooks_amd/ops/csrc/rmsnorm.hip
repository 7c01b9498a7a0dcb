// Fused RMSNorm forward/backward for CDNA4 (gfx950).
//
// Replaces the eager 4-kernel torch sequence (pow/mean/rsqrt/mul) with one
// HBM-bound pass per direction. Reference semantics match the plain
// PyTorch fp32 RMSNorm used by the test-suite reference models
// (llama-family norm; the reference platform delegates this to external
// HuggingFace trainer images — see SURVEY.md §2b).
//
// Layout: x [N, D] row-major. One workgroup (256 threads) per row,
// grid-strided. All math in fp32; bf16 IO vectorized 8-wide (16 B/lane).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdlib>
#include <cstring>

#include "common.h"

namespace {

constexpr int BLOCK = 256;

// swz (optional, bf16 only): ALSO write the normed row into the decode
// GEMM's B-fragment lane order ([D/16][2][32][8], csrc/decode_gemm.hip)
// so the decode path needs no separate x-swizzle launch. Each thread's
// 8-element vector IS one swizzled 16 B slot: pos = (k/16)*512 +
// ((k/8)&1)*256 + row*8.
// res/sum_out (optional, together): normalize x + res instead of x and
// also write the sum — fuses the decode loop's residual add into the
// norm (one launch instead of two; the sum feeds the NEXT residual).
// res32/rsplit (optional, bf16 path): the residual arrives as the
// UNCOMBINED fp32 split-K slab [rsplit, n_rows, D] straight from
// decode_gemm_raw — folding the slices here saves the combine launch.
template <typename T>
__global__ void rmsnorm_fwd_kernel(const T *__restrict__ x,
                                   const T *__restrict__ res,
                                   const float *__restrict__ res32,
                                   int rsplit,
                                   T *__restrict__ sum_out,
                                   const T *__restrict__ w,
                                   T *__restrict__ y,
                                   float *__restrict__ inv_rms,
                                   uint16_t *__restrict__ swz,
                                   int64_t n_rows, int D, float eps) {
  constexpr int W = rb::VIO<T>::W;
  __shared__ float red[BLOCK / RB_WAVE];
  const int nvec = D / W;

  for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const T *xr = x + row * D;
    T *yr = y + row * D;

    float ss = 0.0f;
    for (int i = threadIdx.x; i < nvec; i += BLOCK) {
      float f[W];
      rb::VIO<T>::load(xr + i * W, f);
      if (res != nullptr || res32 != nullptr) {
        if (res != nullptr) {
          float r[W];
          rb::VIO<T>::load(res + row * D + i * W, r);
#pragma unroll
          for (int k = 0; k < W; ++k) f[k] += r[k];
        } else {
          for (int sl = 0; sl < rsplit; ++sl) {
            const float *rp = res32 + ((int64_t)sl * n_rows + row) * D + i * W;
#pragma unroll
            for (int k = 0; k < W; k += 4) {
              float4 a = *reinterpret_cast<const float4 *>(rp + k);
              f[k] += a.x; f[k + 1] += a.y; f[k + 2] += a.z; f[k + 3] += a.w;
            }
          }
        }
        if (sum_out != nullptr)
          rb::VIO<T>::store(sum_out + row * D + i * W, f);
      }
#pragma unroll
      for (int k = 0; k < W; ++k) ss += f[k] * f[k];
    }
    ss = rb::block_reduce_sum(ss, red);
    const float ir = rsqrtf(ss / (float)D + eps);
    if (threadIdx.x == 0 && inv_rms != nullptr) inv_rms[row] = ir;

    for (int i = threadIdx.x; i < nvec; i += BLOCK) {
      float f[W], g[W];
      rb::VIO<T>::load(xr + i * W, f);     // L1-resident second read
      if (res != nullptr) {
        float r[W];
        rb::VIO<T>::load(res + row * D + i * W, r);
#pragma unroll
        for (int k = 0; k < W; ++k) f[k] += r[k];
      } else if (res32 != nullptr) {
        for (int sl = 0; sl < rsplit; ++sl) {
          const float *rp = res32 + ((int64_t)sl * n_rows + row) * D + i * W;
#pragma unroll
          for (int k = 0; k < W; k += 4) {
            float4 a = *reinterpret_cast<const float4 *>(rp + k);
            f[k] += a.x; f[k + 1] += a.y; f[k + 2] += a.z; f[k + 3] += a.w;
          }
        }
      }
      rb::VIO<T>::load(w + i * W, g);
#pragma unroll
      for (int k = 0; k < W; ++k) f[k] = f[k] * ir * g[k];
      rb::VIO<T>::store(yr + i * W, f);
      if constexpr (sizeof(T) == 2) {
        if (swz != nullptr) {
          const int k0 = i * 8;
          rb::VIO<T>::store(reinterpret_cast<T *>(swz) +
                            (k0 >> 4) * 512 + ((k0 >> 3) & 1) * 256 +
                            row * 8, f);
        }
      }
    }
    __syncthreads();
  }
}

// Decode-loop norm (n_rows <= 32, one workgroup per row, grid == n_rows)
// for D == NV * BLOCK * 8 exactly. The generic kernel above spends its
// time on dependent memory round trips, not bytes: x, then each slab slice
// inside a runtime loop, a block reduce, then all of it again plus w. Here
// NV and the residual MODE are template ints, so every load is an unguarded
// 16 B load issued before the first use; f is built once and stays in
// registers across the reduce, and sum_out / y / swz are stored from it.
//
// Results are bit-identical to rmsnorm_fwd_kernel<uint16_t>: same fp32 add
// order (x, then res or slab 0, 1, ...), same per-thread sum-of-squares
// order (v, then k), same block reduce and rsqrtf expression. The generic
// kernel's ISA squares with v_pk_mul_f32 and accumulates with v_add_f32 —
// the compiler did NOT contract `ss += f*f` there — so contraction is
// switched off for this body to keep each square rounded on its own.
enum : int { DEC_NONE = 0, DEC_RES = 1, DEC_SLAB2 = 2, DEC_SLAB4 = 4,
             DEC_SLAB8 = 8 };   // DEC_SLABn: n fp32 split-K slices

typedef __attribute__((ext_vector_type(4))) unsigned int dec_u32x4;

RB_DEV void dec_unpack(const dec_u32x4 &r, float *f) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = rb::bf16_to_f32((uint16_t)(r[j] & 0xFFFFu));
    f[2 * j + 1] = rb::bf16_to_f32((uint16_t)(r[j] >> 16));
  }
}

RB_DEV dec_u32x4 dec_pack(const float *f) {
  dec_u32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    r[j] = (uint32_t)rb::f32_to_bf16(f[2 * j]) |
           ((uint32_t)rb::f32_to_bf16(f[2 * j + 1]) << 16);
  return r;
}

template <int NV, int MODE>
__global__ __launch_bounds__(BLOCK) void rmsnorm_dec_kernel(
    const uint16_t *__restrict__ x, const uint16_t *__restrict__ res,
    const float *__restrict__ res32, uint16_t *__restrict__ sum_out,
    const uint16_t *__restrict__ w, uint16_t *__restrict__ y,
    uint16_t *__restrict__ swz, int n_rows, int D, float eps) {
#pragma clang fp contract(off)
  constexpr int NSL = MODE >= DEC_SLAB2 ? MODE : 0;
  __shared__ float red[BLOCK / RB_WAVE];
  const int64_t row = blockIdx.x;
  const int64_t rowoff = row * D;

  // every load of the row, back to back
  dec_u32x4 xr[NV], wr[NV], rr[MODE == DEC_RES ? NV : 1];
  float4 sr[NSL > 0 ? NV : 1][NSL > 0 ? NSL : 1][2];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int col = (v * BLOCK + threadIdx.x) * 8;
    xr[v] = *reinterpret_cast<const dec_u32x4 *>(x + rowoff + col);
    if constexpr (MODE == DEC_RES)
      rr[v] = *reinterpret_cast<const dec_u32x4 *>(res + rowoff + col);
    if constexpr (NSL > 0) {
#pragma unroll
      for (int sl = 0; sl < NSL; ++sl) {
        const float *rp = res32 + ((int64_t)sl * n_rows + row) * D + col;
        sr[v][sl][0] = *reinterpret_cast<const float4 *>(rp);
        sr[v][sl][1] = *reinterpret_cast<const float4 *>(rp + 4);
      }
    }
    wr[v] = *reinterpret_cast<const dec_u32x4 *>(w + col);
  }

  float f[NV][8];
  float ss = 0.0f;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    dec_unpack(xr[v], f[v]);
    if constexpr (MODE == DEC_RES) {
      float r[8];
      dec_unpack(rr[v], r);
#pragma unroll
      for (int k = 0; k < 8; ++k) f[v][k] += r[k];
    }
    if constexpr (NSL > 0) {
#pragma unroll
      for (int sl = 0; sl < NSL; ++sl) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const float4 a = sr[v][sl][h];
          f[v][4 * h] += a.x; f[v][4 * h + 1] += a.y;
          f[v][4 * h + 2] += a.z; f[v][4 * h + 3] += a.w;
        }
      }
    }
    if constexpr (MODE != DEC_NONE) {
      const int col = (v * BLOCK + threadIdx.x) * 8;
      *reinterpret_cast<dec_u32x4 *>(sum_out + rowoff + col) = dec_pack(f[v]);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) ss += f[v][k] * f[v][k];
  }
  ss = rb::block_reduce_sum(ss, red);
  const float ir = rsqrtf(ss / (float)D + eps);

#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int col = (v * BLOCK + threadIdx.x) * 8;
    float g[8], o[8];
    dec_unpack(wr[v], g);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = f[v][k] * ir * g[k];
    const dec_u32x4 p = dec_pack(o);
    *reinterpret_cast<dec_u32x4 *>(y + rowoff + col) = p;
    *reinterpret_cast<dec_u32x4 *>(swz + (col >> 4) * 512 +
                                   ((col >> 3) & 1) * 256 + row * 8) = p;
  }
}

// RB_DEC_NORM=0 sends the decode entry points through the generic kernel
// (A/B switch and test reference). Read per call, like the Python knobs.
bool dec_norm_enabled() {
  const char *e = getenv("RB_DEC_NORM");
  return e == nullptr || strcmp(e, "1") == 0;
}

template <int NV, int MODE>
void launch_dec(hipStream_t stream, const uint16_t *x, const uint16_t *res,
                const float *res32, uint16_t *sum, const uint16_t *w,
                uint16_t *y, uint16_t *swz, int n_rows, int D, float eps) {
  hipLaunchKernelGGL((rmsnorm_dec_kernel<NV, MODE>), dim3(n_rows), dim3(BLOCK),
                     0, stream, x, res, res32, sum, w, y, swz, n_rows, D, eps);
}

// Launches rmsnorm_dec_kernel when the shape has an instantiation
// (D in {2048, 4096, 8192}; slab splits 2/4/8) and the knob is on; false
// means the caller runs the generic kernel.
bool try_launch_dec(hipStream_t stream, int mode, const uint16_t *x,
                    const uint16_t *res, const float *res32, uint16_t *sum,
                    const uint16_t *w, uint16_t *y, uint16_t *swz,
                    int64_t n_rows, int D, float eps) {
  if (n_rows < 1 || D % (BLOCK * 8) != 0 || !dec_norm_enabled()) return false;
  const int nv = D / (BLOCK * 8);
  if (nv != 1 && nv != 2 && nv != 4) return false;
  if (mode != DEC_NONE && mode != DEC_RES && mode != DEC_SLAB2 &&
      mode != DEC_SLAB4 && mode != DEC_SLAB8)
    return false;
#define RB_DEC_CASE(NV_, MODE_)                                              \
  if (nv == NV_ && mode == MODE_) {                                          \
    launch_dec<NV_, MODE_>(stream, x, res, res32, sum, w, y, swz,            \
                           (int)n_rows, D, eps);                             \
    return true;                                                             \
  }
#define RB_DEC_MODES(NV_)                                                    \
  RB_DEC_CASE(NV_, DEC_NONE) RB_DEC_CASE(NV_, DEC_RES)                       \
  RB_DEC_CASE(NV_, DEC_SLAB2) RB_DEC_CASE(NV_, DEC_SLAB4)                    \
  RB_DEC_CASE(NV_, DEC_SLAB8)
  RB_DEC_MODES(1) RB_DEC_MODES(2) RB_DEC_MODES(4)
#undef RB_DEC_MODES
#undef RB_DEC_CASE
  return false;
}

// Backward: one workgroup per row (grid sized to give every row its own
// WG), dx in one pass. dw: each thread's column set is FIXED across its
// rows (i strides by BLOCK), so the per-thread dw partials live in
// REGISTERS (<= RB_RN_MAXV vectors = 32 floats at D=8192) and hit
// global memory once via atomicAdd at the end. The round-1 version
// accumulated dw element-wise in LDS — 16 scalar ds ops per 16 B of
// input made LDS the bottleneck (65 us on [2048,4096] vs ~14 ideal).
// D > 8*BLOCK*RB_RN_MAXV falls back to the LDS path.
// Register-dw variant, D == NV * BLOCK * W exactly (llama 4096 -> NV=2
// bf16). NV is a template int so every load is UNGUARDED — a runtime
// `if (i < nvec)` around unrolled loads makes hipcc branch per element
// and drain vmcnt(0) each time (cdna_hip_programming.md §5 trap (c));
// the first cut of this kernel did exactly that and ran 7x slower than
// the LDS version it meant to replace (r11: 472 us vs 65).
template <typename T, int NV>
__global__ void rmsnorm_bwd_reg_kernel(const T *__restrict__ x,
                                       const T *__restrict__ w,
                                       const T *__restrict__ dy,
                                       const float *__restrict__ inv_rms,
                                       T *__restrict__ dx,
                                       float *__restrict__ dw,
                                       int64_t n_rows, int D) {
  constexpr int W = rb::VIO<T>::W;
  __shared__ float red[BLOCK / RB_WAVE];

  float dwacc[NV][W];
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int k = 0; k < W; ++k) dwacc[v][k] = 0.0f;

  float wf[NV][W];
#pragma unroll
  for (int v = 0; v < NV; ++v)
    rb::VIO<T>::load(w + (v * BLOCK + threadIdx.x) * W, wf[v]);

  for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const T *xr = x + row * D;
    const T *dyr = dy + row * D;
    T *dxr = dx + row * D;
    const float ir = inv_rms[row];

    float xf[NV][W], df[NV][W];
    float s = 0.0f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int i = v * BLOCK + threadIdx.x;
      rb::VIO<T>::load(xr + i * W, xf[v]);
      rb::VIO<T>::load(dyr + i * W, df[v]);
#pragma unroll
      for (int k = 0; k < W; ++k) s += df[v][k] * wf[v][k] * xf[v][k];
    }
    s = rb::block_reduce_sum(s, red);
    const float c = ir * ir * ir * s / (float)D;

#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int i = v * BLOCK + threadIdx.x;
      float o[W];
#pragma unroll
      for (int k = 0; k < W; ++k) {
        o[k] = ir * wf[v][k] * df[v][k] - c * xf[v][k];
        dwacc[v][k] += df[v][k] * xf[v][k] * ir;
      }
      rb::VIO<T>::store(dxr + i * W, o);
    }
  }

#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int i = v * BLOCK + threadIdx.x;
#pragma unroll
    for (int k = 0; k < W; ++k)
      if (dwacc[v][k] != 0.0f) atomicAdd(dw + i * W + k, dwacc[v][k]);
  }
}

template <typename T>
__global__ void rmsnorm_bwd_kernel(const T *__restrict__ x,
                                           const T *__restrict__ w,
                                           const T *__restrict__ dy,
                                           const float *__restrict__ inv_rms,
                                           T *__restrict__ dx,
                                           float *__restrict__ dw,
                                           int64_t n_rows, int D) {
  constexpr int W = rb::VIO<T>::W;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *dw_loc = reinterpret_cast<float *>(smem);          // D floats
  float *red = dw_loc + D;                                  // BLOCK/64 floats
  const int nvec = D / W;

  for (int i = threadIdx.x; i < D; i += BLOCK) dw_loc[i] = 0.0f;
  __syncthreads();

  for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const T *xr = x + row * D;
    const T *dyr = dy + row * D;
    T *dxr = dx + row * D;
    const float ir = inv_rms[row];

    float s = 0.0f;
    for (int i = threadIdx.x; i < nvec; i += BLOCK) {
      float xf[W], wf[W], df[W];
      rb::VIO<T>::load(xr + i * W, xf);
      rb::VIO<T>::load(w + i * W, wf);
      rb::VIO<T>::load(dyr + i * W, df);
#pragma unroll
      for (int k = 0; k < W; ++k) s += df[k] * wf[k] * xf[k];
    }
    s = rb::block_reduce_sum(s, red);
    const float c = ir * ir * ir * s / (float)D;

    for (int i = threadIdx.x; i < nvec; i += BLOCK) {
      float xf[W], wf[W], df[W], o[W];
      rb::VIO<T>::load(xr + i * W, xf);
      rb::VIO<T>::load(w + i * W, wf);
      rb::VIO<T>::load(dyr + i * W, df);
#pragma unroll
      for (int k = 0; k < W; ++k) {
        o[k] = ir * wf[k] * df[k] - c * xf[k];
        dw_loc[i * W + k] += df[k] * xf[k] * ir;
      }
      rb::VIO<T>::store(dxr + i * W, o);
    }
    __syncthreads();
  }

  __syncthreads();
  for (int i = threadIdx.x; i < D; i += BLOCK)
    if (dw_loc[i] != 0.0f) atomicAdd(dw + i, dw_loc[i]);
}

}  // namespace

std::vector<at::Tensor> rmsnorm_fwd(at::Tensor x, at::Tensor w, double eps) {
  TORCH_CHECK(x.is_cuda() && w.is_cuda(), "rmsnorm: tensors must be on GPU");
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous(), "rmsnorm: contiguous only");
  const int D = (int)x.size(-1);
  const int64_t n_rows = x.numel() / D;
  auto y = at::empty_like(x);
  auto inv_rms = at::empty({n_rows}, x.options().dtype(at::kFloat));
  auto stream = at::hip::getCurrentHIPStream();

  if (x.scalar_type() == at::kBFloat16) {
    TORCH_CHECK(D % 8 == 0, "rmsnorm bf16: D must be a multiple of 8");
    hipLaunchKernelGGL(rmsnorm_fwd_kernel<uint16_t>, dim3(std::min<int64_t>(n_rows, 2048)),
                       dim3(BLOCK), 0, stream,
                       (const uint16_t *)x.data_ptr(),
                       (const uint16_t *)nullptr, (const float *)nullptr, 0,
                       (uint16_t *)nullptr,
                       (const uint16_t *)w.data_ptr(),
                       (uint16_t *)y.data_ptr(), inv_rms.data_ptr<float>(),
                       (uint16_t *)nullptr, n_rows, D, (float)eps);
  } else if (x.scalar_type() == at::kFloat) {
    TORCH_CHECK(D % 4 == 0, "rmsnorm f32: D must be a multiple of 4");
    hipLaunchKernelGGL(rmsnorm_fwd_kernel<float>, dim3(std::min<int64_t>(n_rows, 2048)),
                       dim3(BLOCK), 0, stream,
                       x.data_ptr<float>(), (const float *)nullptr,
                       (const float *)nullptr, 0,
                       (float *)nullptr, w.data_ptr<float>(),
                       y.data_ptr<float>(),
                       inv_rms.data_ptr<float>(), (uint16_t *)nullptr,
                       n_rows, D, (float)eps);
  } else {
    TORCH_CHECK(false, "rmsnorm: unsupported dtype");
  }
  return {y, inv_rms};
}

// Decode-path variant: returns {y, y_swz} where y_swz is the decode
// GEMM's pre-swizzled B-operand ([D/16]x512 bf16, rows m >= n_rows left
// uninitialized: decode_gemm drops their outputs at the epilogue).
std::vector<at::Tensor> rmsnorm_fwd_dec(at::Tensor x, at::Tensor w,
                                        double eps) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && w.is_contiguous(),
              "rmsnorm_fwd_dec: contiguous GPU tensors");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "rmsnorm_fwd_dec: bf16");
  const int64_t n_rows = x.numel() / x.size(-1);
  const int D = (int)x.size(-1);
  TORCH_CHECK(n_rows <= 32 && D % 16 == 0, "rmsnorm_fwd_dec: shape");
  auto y = at::empty_like(x);
  auto swz = at::empty({(int64_t)(D / 16) * 512}, x.options());
  auto stream = at::cuda::getCurrentHIPStream();
  if (try_launch_dec(stream, DEC_NONE, (const uint16_t *)x.data_ptr(), nullptr,
                     nullptr, nullptr, (const uint16_t *)w.data_ptr(),
                     (uint16_t *)y.data_ptr(), (uint16_t *)swz.data_ptr(),
                     n_rows, D, (float)eps))
    return {y, swz};
  hipLaunchKernelGGL(rmsnorm_fwd_kernel<uint16_t>, dim3(n_rows),
                     dim3(BLOCK), 0, stream,
                     (const uint16_t *)x.data_ptr(),
                     (const uint16_t *)nullptr, (const float *)nullptr, 0,
                     (uint16_t *)nullptr,
                     (const uint16_t *)w.data_ptr(),
                     (uint16_t *)y.data_ptr(), (float *)nullptr,
                     (uint16_t *)swz.data_ptr(), n_rows, D, (float)eps);
  return {y, swz};
}

// Fused residual + norm + swizzle for the decode loop: returns
// {sum = x + res, y = rmsnorm(sum) * w, y_swz}. One launch replaces the
// eager residual add + the norm + the operand swizzle.
std::vector<at::Tensor> rmsnorm_res_fwd_dec(at::Tensor x, at::Tensor res,
                                            at::Tensor w, double eps) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && res.is_contiguous() &&
              w.is_contiguous(), "rmsnorm_res_fwd_dec: contiguous");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
              res.scalar_type() == at::kBFloat16, "rmsnorm_res_fwd_dec: bf16");
  TORCH_CHECK(x.sizes() == res.sizes(), "rmsnorm_res_fwd_dec: shape");
  const int64_t n_rows = x.numel() / x.size(-1);
  const int D = (int)x.size(-1);
  TORCH_CHECK(n_rows <= 32 && D % 16 == 0, "rmsnorm_res_fwd_dec: shape");
  auto sum = at::empty_like(x);
  auto y = at::empty_like(x);
  auto swz = at::empty({(int64_t)(D / 16) * 512}, x.options());
  auto stream = at::cuda::getCurrentHIPStream();
  if (try_launch_dec(stream, DEC_RES, (const uint16_t *)x.data_ptr(),
                     (const uint16_t *)res.data_ptr(), nullptr,
                     (uint16_t *)sum.data_ptr(),
                     (const uint16_t *)w.data_ptr(), (uint16_t *)y.data_ptr(),
                     (uint16_t *)swz.data_ptr(), n_rows, D, (float)eps))
    return {sum, y, swz};
  hipLaunchKernelGGL(rmsnorm_fwd_kernel<uint16_t>, dim3(n_rows),
                     dim3(BLOCK), 0, stream,
                     (const uint16_t *)x.data_ptr(),
                     (const uint16_t *)res.data_ptr(),
                     (const float *)nullptr, 0,
                     (uint16_t *)sum.data_ptr(),
                     (const uint16_t *)w.data_ptr(),
                     (uint16_t *)y.data_ptr(), (float *)nullptr,
                     (uint16_t *)swz.data_ptr(), n_rows, D, (float)eps);
  return {sum, y, swz};
}

// Same, with the residual as an UNCOMBINED fp32 split-K slab
// [split, n_rows, D] from decode_gemm_raw.
std::vector<at::Tensor> rmsnorm_res_slab_fwd_dec(at::Tensor x,
                                                 at::Tensor slabs,
                                                 at::Tensor w, double eps) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && slabs.is_contiguous() &&
              w.is_contiguous(), "rmsnorm_res_slab_fwd_dec: contiguous");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 &&
              slabs.scalar_type() == at::kFloat &&
              slabs.dim() == 3, "rmsnorm_res_slab_fwd_dec: dtypes");
  const int64_t n_rows = x.numel() / x.size(-1);
  const int D = (int)x.size(-1);
  TORCH_CHECK(slabs.size(1) == n_rows && slabs.size(2) == D &&
              n_rows <= 32 && D % 16 == 0, "rmsnorm_res_slab_fwd_dec: shape");
  auto sum = at::empty_like(x);
  auto y = at::empty_like(x);
  auto swz = at::empty({(int64_t)(D / 16) * 512}, x.options());
  auto stream = at::cuda::getCurrentHIPStream();
  const int64_t split = slabs.size(0);
  if ((split == 2 || split == 4 || split == 8) &&
      try_launch_dec(stream, (int)split, (const uint16_t *)x.data_ptr(),
                     nullptr, (const float *)slabs.data_ptr(),
                     (uint16_t *)sum.data_ptr(),
                     (const uint16_t *)w.data_ptr(), (uint16_t *)y.data_ptr(),
                     (uint16_t *)swz.data_ptr(), n_rows, D, (float)eps))
    return {sum, y, swz};
  hipLaunchKernelGGL(rmsnorm_fwd_kernel<uint16_t>, dim3(n_rows),
                     dim3(BLOCK), 0, stream,
                     (const uint16_t *)x.data_ptr(),
                     (const uint16_t *)nullptr,
                     (const float *)slabs.data_ptr(), (int)slabs.size(0),
                     (uint16_t *)sum.data_ptr(),
                     (const uint16_t *)w.data_ptr(),
                     (uint16_t *)y.data_ptr(), (float *)nullptr,
                     (uint16_t *)swz.data_ptr(), n_rows, D, (float)eps);
  return {sum, y, swz};
}

std::vector<at::Tensor> rmsnorm_bwd(at::Tensor x, at::Tensor w, at::Tensor dy,
                                    at::Tensor inv_rms) {
  TORCH_CHECK(x.is_cuda() && dy.is_contiguous() && x.is_contiguous(), "rmsnorm_bwd: bad args");
  const int D = (int)x.size(-1);
  const int64_t n_rows = x.numel() / D;
  auto dx = at::empty_like(x);
  auto dw = at::zeros({D}, x.options().dtype(at::kFloat));
  auto stream = at::hip::getCurrentHIPStream();
  const int nwg = (int)std::min<int64_t>(n_rows, 4096);
  const size_t shmem = (size_t)D * sizeof(float) + (BLOCK / RB_WAVE) * sizeof(float);
  TORCH_CHECK(shmem <= 160 * 1024, "rmsnorm_bwd: D too large for LDS accumulation");

  // The register-dw variant measured 7x SLOWER than this LDS path on
  // [2048,4096] (472 vs 65 us, r11/r13) despite clean ISA (no spills,
  // 95 VGPR, 5 waves/SIMD) — root cause unidentified; the LDS
  // accumulate stays the shipped path.
  const int nv = 0;
  if (x.scalar_type() == at::kBFloat16) {
    auto a = (const uint16_t *)x.data_ptr();
    auto b = (const uint16_t *)w.data_ptr();
    auto c = (const uint16_t *)dy.data_ptr();
    auto irp = inv_rms.data_ptr<float>();
    auto dxp = (uint16_t *)dx.data_ptr();
    auto dwp = dw.data_ptr<float>();
    if (nv == 1)
      hipLaunchKernelGGL((rmsnorm_bwd_reg_kernel<uint16_t, 1>), dim3(nwg),
                         dim3(BLOCK), 0, stream, a, b, c, irp, dxp, dwp, n_rows, D);
    else if (nv == 2)
      hipLaunchKernelGGL((rmsnorm_bwd_reg_kernel<uint16_t, 2>), dim3(nwg),
                         dim3(BLOCK), 0, stream, a, b, c, irp, dxp, dwp, n_rows, D);
    else if (nv == 4)
      hipLaunchKernelGGL((rmsnorm_bwd_reg_kernel<uint16_t, 4>), dim3(nwg),
                         dim3(BLOCK), 0, stream, a, b, c, irp, dxp, dwp, n_rows, D);
    else
      hipLaunchKernelGGL(rmsnorm_bwd_kernel<uint16_t>, dim3(nwg), dim3(BLOCK),
                         shmem, stream, a, b, c, irp, dxp, dwp, n_rows, D);
  } else if (x.scalar_type() == at::kFloat) {
    auto a = x.data_ptr<float>();
    auto b = w.data_ptr<float>();
    auto c = dy.data_ptr<float>();
    auto irp = inv_rms.data_ptr<float>();
    auto dxp = dx.data_ptr<float>();
    auto dwp = dw.data_ptr<float>();
    if (nv == 1)
      hipLaunchKernelGGL((rmsnorm_bwd_reg_kernel<float, 1>), dim3(nwg),
                         dim3(BLOCK), 0, stream, a, b, c, irp, dxp, dwp, n_rows, D);
    else if (nv == 2)
      hipLaunchKernelGGL((rmsnorm_bwd_reg_kernel<float, 2>), dim3(nwg),
                         dim3(BLOCK), 0, stream, a, b, c, irp, dxp, dwp, n_rows, D);
    else if (nv == 4)
      hipLaunchKernelGGL((rmsnorm_bwd_reg_kernel<float, 4>), dim3(nwg),
                         dim3(BLOCK), 0, stream, a, b, c, irp, dxp, dwp, n_rows, D);
    else
      hipLaunchKernelGGL(rmsnorm_bwd_kernel<float>, dim3(nwg), dim3(BLOCK),
                         shmem, stream, a, b, c, irp, dxp, dwp, n_rows, D);
  } else {
    TORCH_CHECK(false, "rmsnorm_bwd: unsupported dtype");
  }
  return {dx, dw};
}
