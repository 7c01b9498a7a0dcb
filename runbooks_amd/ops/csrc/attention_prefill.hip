// Flash-attention prefill (causal, GQA/MQA, bf16) for CDNA4 (gfx950) over
// dense token-major tensors; also the training forward (saves the LSE).
//
// The kernel is flash_fwd_rows + flash_fwd_store (flash_fwd_core.h:
// geometry, softmax, PV and epilogue) fed by DenseKV below; this file owns
// the dense staging, the [B, S, H, DH] row mapping, the host entry points
// and the MFMA layout probe.
//
// q,k,v,out: [B, S, H, DH] bf16 token-major. DH in {64, 128, 256}.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "flash_fwd_core.h"

namespace {

using rb::bf16x8v;
using rb::f32x16v;

constexpr int BLOCK = rb::FLASH_BLOCK;
constexpr int KVB = rb::FLASH_KVB;

// KV source: k, v [B, S, Hkv, DH], batch b, kv head h_kv.
struct DenseKV {
  const uint16_t *__restrict__ kp;
  const uint16_t *__restrict__ vp;
  int b, S, Hkv, h_kv;

  template <int DH>
  RB_DEV void stage(int kt, char *k_img, char *v_img) const {
    constexpr int K_STRIDE = DH * 2 + 16;
    constexpr int V_STRIDE = KVB * 2 + 16;
    const int tid = threadIdx.x;
    const int kbase = kt * KVB;

    // ---- stage K tile: [key][d] rows, each thread 16 elems ---------------
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
          val = *reinterpret_cast<const rb::bf16x8 *>(
              kp + ((int64_t)(b * S + gk) * Hkv + h_kv) * DH + d0);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) val.v[e] = 0;
        }
        *reinterpret_cast<rb::bf16x8 *>(k_img + key * K_STRIDE + d0 * 2) = val;
      }
    }
    // ---- stage V tile transposed: thread owns column d, KPG keys ---------
    {
      constexpr int GRPS = BLOCK / DH;      // thread groups over keys
      constexpr int KPG = KVB / GRPS;       // keys per group (16 @DH=128)
      const int d = tid % DH;
      const int kg0 = (tid / DH) * KPG;
      uint16_t tmp[KPG];
#pragma unroll
      for (int e = 0; e < KPG; ++e) {
        const int gk = kbase + kg0 + e;
        tmp[e] = (gk < S)
            ? vp[((int64_t)(b * S + gk) * Hkv + h_kv) * DH + d]
            : (uint16_t)0;
      }
#pragma unroll
      for (int c8 = 0; c8 < KPG / 8; ++c8)
        *reinterpret_cast<rb::bf16x8 *>(v_img + d * V_STRIDE + (kg0 + c8 * 8) * 2) =
            *reinterpret_cast<rb::bf16x8 *>(&tmp[c8 * 8]);
    }
  }
};

template <int DH>
__global__ __launch_bounds__(BLOCK, 2) void flash_prefill_kernel(
    const uint16_t *__restrict__ qp, const uint16_t *__restrict__ kp,
    const uint16_t *__restrict__ vp, uint16_t *__restrict__ op,
    float *__restrict__ lsep,  // [B, Hq, S] log-sum-exp for training bwd
    int B, int S, int Hq, int Hkv, float scale) {
  const int q0 = blockIdx.x * 256;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int qrow = q0 + (threadIdx.x >> 6) * 32 + (threadIdx.x & 31);
  const bool q_valid = qrow < S;

  const auto acc = rb::flash_fwd_rows<DH>(
      qp + ((int64_t)(b * S + (q_valid ? qrow : 0)) * Hq + h) * DH, qrow,
      q_valid, S, q0, DenseKV{kp, vp, b, S, Hkv, h / (Hq / Hkv)}, scale);
  if (q_valid)
    rb::flash_fwd_store<DH>(
        acc, op + ((int64_t)(b * S + qrow) * Hq + h) * DH,
        lsep ? lsep + ((int64_t)b * Hq + h) * S + qrow : nullptr);
}

}  // namespace

static at::Tensor flash_fwd_impl(at::Tensor q, at::Tensor k, at::Tensor v,
                                 double scale, float *lsep) {
  TORCH_CHECK(q.is_cuda() && q.is_contiguous() && k.is_contiguous() &&
                  v.is_contiguous(), "flash_prefill: contiguous GPU tensors");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16, "flash_prefill: bf16 only");
  TORCH_CHECK(q.dim() == 4, "flash_prefill: q must be [B, S, Hq, DH]");
  const int B = (int)q.size(0), S = (int)q.size(1), Hq = (int)q.size(2),
            DH = (int)q.size(3);
  const int Hkv = (int)k.size(2);
  TORCH_CHECK(Hq % Hkv == 0, "flash_prefill: Hq % Hkv");
  auto out = at::empty_like(q);
  auto stream = at::hip::getCurrentHIPStream();
  const dim3 grid((S + 255) / 256, Hq, B);

  rb::flash_dispatch_dh(DH, "flash_prefill", [&](auto dh) {
    constexpr int D = decltype(dh)::value;
    hipLaunchKernelGGL((flash_prefill_kernel<D>), grid, dim3(BLOCK),
                       rb::flash_fwd_smem<D>(), stream,
                       (const uint16_t *)q.data_ptr(),
                       (const uint16_t *)k.data_ptr(),
                       (const uint16_t *)v.data_ptr(), (uint16_t *)out.data_ptr(),
                       lsep, B, S, Hq, Hkv, (float)scale);
  });
  return out;
}

at::Tensor flash_prefill(at::Tensor q, at::Tensor k, at::Tensor v,
                         double scale) {
  return flash_fwd_impl(q, k, v, scale, nullptr);
}

// Training forward: additionally returns the per-row log-sum-exp
// ([B, Hq, S] f32) consumed by fa_bwd (attention_bwd.hip).
std::vector<at::Tensor> flash_fwd_train(at::Tensor q, at::Tensor k,
                                        at::Tensor v, double scale) {
  const int B = (int)q.size(0), S = (int)q.size(1), Hq = (int)q.size(2);
  auto lse = at::empty({B, Hq, S}, q.options().dtype(at::kFloat));
  auto out = flash_fwd_impl(q, k, v, scale, lse.data_ptr<float>());
  return {out, lse};
}

// ---------------------------------------------------------------------------
// Layout probe: one v_mfma_f32_32x32x16_bf16 computing C = A @ B with the
// fragment maps of mfma_frag.h. The GPU test compares it against torch
// matmul — if the assumed lane->element maps are wrong, THIS fails first
// and pinpoints the bug (instead of the whole flash kernel).
// a: [32, 16] bf16 (A[i][k]);  b: [16, 32] bf16 (B[k][j]) -> c: [32, 32] f32
// ---------------------------------------------------------------------------
namespace {
__global__ void mfma_probe_kernel(const uint16_t *__restrict__ a,
                                  const uint16_t *__restrict__ b,
                                  float *__restrict__ c) {
  const int lane = threadIdx.x & 63;
  const int hi = lane >> 5;
  const int i = lane & 31;
  union { unsigned short u[8]; bf16x8v v; } af, bf;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    af.u[e] = a[i * 16 + hi * 8 + e];         // A[i][k], k = hi*8+e
    bf.u[e] = b[(hi * 8 + e) * 32 + i];       // B[k][j], j = lane&31
  }
  f32x16v acc = (f32x16v)(0.0f);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af.v, bf.v, acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * hi;
    c[row * 32 + i] = acc[r];                  // C[row][j = lane&31]
  }
}
}  // namespace

at::Tensor mfma_probe_32x32x16(at::Tensor a, at::Tensor b) {
  TORCH_CHECK(a.is_cuda() && a.scalar_type() == at::kBFloat16);
  TORCH_CHECK(a.sizes() == at::IntArrayRef({32, 16}) &&
              b.sizes() == at::IntArrayRef({16, 32}), "probe shapes");
  auto c = at::zeros({32, 32}, a.options().dtype(at::kFloat));
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, stream,
                     (const uint16_t *)a.contiguous().data_ptr(),
                     (const uint16_t *)b.contiguous().data_ptr(),
                     c.data_ptr<float>());
  return c;
}
