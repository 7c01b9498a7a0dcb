// Batched per-request sampler for CDNA4 (gfx950).
//
// One workgroup per row of the decode batch; every row carries its own
// temperature / top-k / top-p / min-p / penalties / seed. One launch does
// penalties, the row's log-sum-exp, the three filters, the Gumbel-max
// draw, the drawn token's logprob and the top-L logprobs. No sort: every
// threshold comes from a 4 x 8-bit radix select over the order-preserving
// uint32 image of the fp32 value, with a 256-bin histogram in LDS.
//
//   a   = fp32 logits after penalties           (logprobs describe a)
//   z   = a / temperature                       (filters and draw use z)
//   top-k: keep z >= k-th largest z
//   top-p: keep z >= first value at which the mass of {z >= value},
//          renormalised over the top-k survivors, reaches top_p
//   min-p: keep z >= zmax + ln(min_p)
//   draw : argmax over the kept set of z + G(seed, col)
//
// The top-p mass is accumulated as integers (round(exp(z - zmax) * 2^32)
// in uint64, LDS integer atomics): integer adds commute, so a row's
// result is the same bit for bit from run to run and in any batch.
//
// The adjusted logits live in a [B, V] fp32 workspace (L2-resident at
// serving sizes); the row is never held in LDS, so V is unbounded.
// Every pass over the workspace assigns elements to threads the same
// way on the 16 B and on the scalar path, so a row's sums do not depend
// on which path its alignment selects.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"
#include "sampling_rng.h"

namespace {

constexpr int SB_BLOCK = 1024;
constexpr int SB_WAVES = SB_BLOCK / RB_WAVE;
constexpr int SB_MAXL = 20;         // top-L logprobs per row
constexpr int SB_PARAM_WORDS = 10;  // packed per-row parameters (ops/sampling.py)
constexpr int SB_OUT_FIXED = 4;     // token, logprob, kept, thr

typedef unsigned long long u64;

// order-preserving uint32 image of an fp32 value (-0 folded onto +0)
RB_DEV uint32_t ord_key(float v) {
  uint32_t b = __float_as_uint(v);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

RB_DEV float key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// Visit every element of an fp32 row. Thread t owns the 4-element groups
// t, t + BLOCK, ...; `vec` (row base 16 B aligned and V % 4 == 0) only
// chooses how a group is loaded.
template <typename F>
RB_DEV void for_each_f32(const float *row, int V, bool vec, F &&f) {
  const int ngrp = (V + 3) >> 2;
  for (int g = threadIdx.x; g < ngrp; g += SB_BLOCK) {
    const int i0 = g * 4;
    if (vec) {
      const float4 v = *reinterpret_cast<const float4 *>(row + i0);
      f(i0, v.x); f(i0 + 1, v.y); f(i0 + 2, v.z); f(i0 + 3, v.w);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (i0 + k < V) f(i0 + k, row[i0 + k]);
    }
  }
}

// 16 B input loads: 8 bf16 or 4 f32 -> fp32
RB_DEV void load16(const uint16_t *p, float *f) {
  const uint4 r = *reinterpret_cast<const uint4 *>(p);
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
RB_DEV void load16(const float *p, float *f) {
  const float4 r = *reinterpret_cast<const float4 *>(p);
  f[0] = r.x; f[1] = r.y; f[2] = r.z; f[3] = r.w;
}

struct SelState {
  u64 target;   // weight still to cover inside the chosen bin
  u64 bin_w;    // total weight of the chosen bin
  int bin;
};

struct Shared {
  u64 hist[256];
  SelState sel;
  float red_f0[SB_WAVES];
  float red_f1[SB_WAVES];
  int red_i0[SB_WAVES];
  int red_i1[SB_WAVES];
  u64 red_u[SB_WAVES];
  uint32_t cand_key[SB_MAXL];
  int cand_id[SB_MAXL];
  int cand_n;
};

// Largest key K such that the weight of {participating elements with
// key >= K} reaches `target` (1 <= target <= total weight). `kf(idx, v,
// key, w)` says whether an element takes part and gives its key and
// weight. On return sh.sel.target is the weight K itself still had to
// supply and sh.sel.bin_w the weight of the elements whose key is K.
template <typename KF>
RB_DEV uint32_t radix_select(const float *row, int V, bool vec,
                             u64 target, Shared &sh, KF &&kf) {
  uint32_t prefix = 0u, mask = 0u;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = threadIdx.x; i < 256; i += SB_BLOCK) sh.hist[i] = 0ull;
    __syncthreads();
    for_each_f32(row, V, vec, [&](int idx, float v) {
      uint32_t key; u64 w;
      if (kf(idx, v, key, w) && (key & mask) == prefix)
        atomicAdd(&sh.hist[(key >> shift) & 255u], w);
    });
    __syncthreads();
    if (threadIdx.x < RB_WAVE) {
      // lane l walks bins 255-4l .. 252-4l, i.e. the wave walks downward
      const int lane = threadIdx.x;
      u64 h[4], s = 0ull;
#pragma unroll
      for (int k = 0; k < 4; ++k) { h[k] = sh.hist[255 - 4 * lane - k]; s += h[k]; }
      u64 inc = s;
#pragma unroll
      for (int off = 1; off < RB_WAVE; off <<= 1) {
        const u64 o = __shfl_up(inc, off, RB_WAVE);
        if (lane >= off) inc += o;
      }
      const u64 hit = __ballot(inc >= target);
      // target above the total cannot happen for a valid call; then the
      // walk ends in the lowest bin and every element stays selected
      const int first = hit ? (__ffsll((long long)hit) - 1) : (RB_WAVE - 1);
      if (lane == first) {
        u64 c = inc - s;
        int sel = 3;
        bool found = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!found) {
            if (c + h[k] >= target) { sel = k; found = true; }
            else c += h[k];
          }
        }
        sh.sel.bin = 255 - 4 * lane - sel;
        sh.sel.bin_w = h[sel];
        sh.sel.target = found ? target - c : 1ull;
      }
    }
    __syncthreads();
    prefix |= (uint32_t)sh.sel.bin << shift;
    mask |= 255u << shift;
    target = sh.sel.target;
  }
  return prefix;
}

// a -= frequency*count + presence, then the multiplicative penalty; each
// step rounded on its own (no fused multiply-add), as the torch
// expression in Engine._apply_penalties rounds
RB_DEV float penalise(float a, float c, float frequency, float presence,
                      float repetition) {
#pragma clang fp contract(off)
  const float t = frequency * c;
  const float u = t + presence;
  a = a - u;
  if (repetition != 1.0f) a = a > 0.0f ? a / repetition : a * repetition;
  return a;
}

// (max, sum-exp relative to max, argmax with the lowest id on ties)
RB_DEV void lse_combine(float &m, float &s, int &mi, float om, float os, int oi) {
  const float M = fmaxf(m, om);
  const float s1 = (m == -INFINITY) ? 0.0f : s * __expf(m - M);
  const float s2 = (om == -INFINITY) ? 0.0f : os * __expf(om - M);
  if (om > m || (om == m && oi < mi)) mi = oi;
  m = M;
  s = s1 + s2;
}

RB_DEV void argmax_combine(float &v, int &i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

template <typename T>
__global__ __launch_bounds__(SB_BLOCK) void sample_batch_kernel(
    const T *__restrict__ logits, float *__restrict__ ws,
    const int32_t *__restrict__ params, const int32_t *__restrict__ csr,
    int32_t *__restrict__ out, int B, int V, int L, int in_vec, int ws_vec) {
  __shared__ Shared sh;

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;

  const int32_t *pr = params + (int64_t)b * SB_PARAM_WORDS;
  const float temp = __int_as_float(pr[0]);
  const int top_k = pr[1];
  const float top_p = __int_as_float(pr[2]);
  const float ln_min_p = __int_as_float(pr[3]);   // -inf: min-p off
  const float presence = __int_as_float(pr[4]);
  const float frequency = __int_as_float(pr[5]);
  const float repetition = __int_as_float(pr[6]);
  const uint64_t seed = (uint64_t)(uint32_t)pr[7] | ((uint64_t)(uint32_t)pr[8] << 32);

  const T *xr = logits + (int64_t)b * V;
  float *ar = ws + (int64_t)b * V;
  int32_t *orow = out + (int64_t)b * (SB_OUT_FIXED + 2 * L);
  const bool vec = ws_vec != 0;

  // ---- adjusted logits: a = float(x), then the row's sparse penalties ----
  if (in_vec) {
    constexpr int W = 16 / (int)sizeof(T);
    const int nvec = V / W;
    for (int g = tid; g < nvec; g += SB_BLOCK) {
      float f[W];
      load16(xr + (int64_t)g * W, f);
#pragma unroll
      for (int k = 0; k < W; k += 4)
        *reinterpret_cast<float4 *>(ar + (int64_t)g * W + k) =
            make_float4(f[k], f[k + 1], f[k + 2], f[k + 3]);
    }
  } else {
    for (int i = tid; i < V; i += SB_BLOCK) ar[i] = rb::bf16_to_f32_or_id(xr[i]);
  }
  __syncthreads();
  if (csr != nullptr) {
    // ids are unique per row (host-checked to lie in [0, V)): no races
    const int nnz = csr[B];
    const int32_t *ids = csr + (B + 1);
    const int32_t *cnts = ids + nnz;
    const int s = csr[b], e = csr[b + 1];
    for (int j = s + tid; j < e; j += SB_BLOCK) {
      const int id = ids[j];
      if ((unsigned)id < (unsigned)V) {
          const float c = (float)cnts[j];
        ar[id] = penalise(ar[id], c, frequency, presence, repetition);
      }
    }
    __syncthreads();
  }

  // ---- row statistics of a: max, argmax, sum-exp (online softmax) --------
  float m = -INFINITY, se = 0.0f;
  int mi = 0x7fffffff;
  for_each_f32(ar, V, vec, [&](int idx, float v) {
    if (v > m) { se = se * __expf(m - v) + 1.0f; m = v; mi = idx; }
    else if (v != -INFINITY) se += __expf(v - m);
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float om = __shfl_xor(m, off, 64);
    const float os = __shfl_xor(se, off, 64);
    const int oi = __shfl_xor(mi, off, 64);
    lse_combine(m, se, mi, om, os, oi);
  }
  if (lane == 0) { sh.red_f0[wid] = m; sh.red_f1[wid] = se; sh.red_i0[wid] = mi; }
  __syncthreads();
  m = sh.red_f0[0]; se = sh.red_f1[0]; mi = sh.red_i0[0];
  for (int w = 1; w < SB_WAVES; ++w)
    lse_combine(m, se, mi, sh.red_f0[w], sh.red_f1[w], sh.red_i0[w]);
  __syncthreads();
  const float amax = m;
  const int arg = (mi < V) ? mi : 0;
  const float lse = amax + logf(se);

  // ---- filters and draw ----------------------------------------------------
  int token = arg;
  int kept = V;
  float thr = -INFINITY;
  if (temp > 0.0f) {
    const float zmax = __fdiv_rn(amax, temp);
    uint32_t thr_key = 0u;   // below every key: nothing filtered
    bool active = false;
    uint32_t key_k = 0u;
    if (top_k > 0 && top_k < V) {
      key_k = radix_select(ar, V, vec, (u64)top_k, sh,
                           [&](int, float v, uint32_t &key, u64 &w) {
                             key = ord_key(__fdiv_rn(v, temp));
                             w = 1ull;
                             return true;
                           });
      thr_key = key_k;
      active = true;
    }
    if (top_p > 0.0f && top_p < 1.0f) {
      // integer mass of the top-k survivors
      u64 mass = 0ull;
      for_each_f32(ar, V, vec, [&](int, float v) {
        const float z = __fdiv_rn(v, temp);
        if (ord_key(z) >= key_k)
          mass += __float2ull_rn(__expf(z - zmax) * 4294967296.0f);
      });
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) mass += __shfl_xor(mass, off, 64);
      if (lane == 0) sh.red_u[wid] = mass;
      __syncthreads();
      mass = 0ull;
      for (int w = 0; w < SB_WAVES; ++w) mass += sh.red_u[w];
      __syncthreads();
      u64 target = (u64)ceil((double)top_p * (double)mass);
      if (target < 1ull) target = 1ull;
      if (target > mass) target = mass;
      if (mass > 0ull) {
        const uint32_t key_p = radix_select(
            ar, V, vec, target, sh, [&](int, float v, uint32_t &key, u64 &w) {
              const float z = __fdiv_rn(v, temp);
              key = ord_key(z);
              w = __float2ull_rn(__expf(z - zmax) * 4294967296.0f);
              return key >= key_k;
            });
        if (key_p > thr_key) thr_key = key_p;
        active = true;
      }
    }
    if (ln_min_p != -INFINITY) {
      const uint32_t key_m = ord_key(zmax + ln_min_p);
      if (key_m > thr_key) thr_key = key_m;
      active = true;
    }

    // masked Gumbel-max draw; the noise depends on (seed, col) only
    float best = -INFINITY;
    int best_i = 0x7fffffff;
    int cnt = 0;
    for_each_f32(ar, V, vec, [&](int idx, float v) {
      const float z = __fdiv_rn(v, temp);
      if (ord_key(z) >= thr_key) {
        ++cnt;
        const float u = rb::rng_uniform(seed, 0u, (uint32_t)idx);
        const float g = z - rb::neg_gumbel(u);
        if (g > best) { best = g; best_i = idx; }
      }
    });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(best, off, 64);
      const int oi = __shfl_xor(best_i, off, 64);
      argmax_combine(best, best_i, ov, oi);
      cnt += __shfl_xor(cnt, off, 64);
    }
    if (lane == 0) { sh.red_f0[wid] = best; sh.red_i0[wid] = best_i; sh.red_i1[wid] = cnt; }
    __syncthreads();
    best = sh.red_f0[0]; best_i = sh.red_i0[0]; cnt = sh.red_i1[0];
    for (int w = 1; w < SB_WAVES; ++w) {
      argmax_combine(best, best_i, sh.red_f0[w], sh.red_i0[w]);
      cnt += sh.red_i1[w];
    }
    __syncthreads();
    token = (best_i < V) ? best_i : arg;
    kept = cnt;
    thr = active ? key_value(thr_key) : -INFINITY;
  }
  if (tid == 0) {
    orow[0] = token;
    orow[1] = __float_as_int(ar[token] - lse);
    orow[2] = kept;
    orow[3] = __float_as_int(thr);
  }

  // ---- top-L logprobs of a: select by count, ties by lowest id -------------
  if (L > 0) {
    const int Leff = L < V ? L : V;
    uint32_t key_l = 0u;
    int id_cut = 0x7fffffff;
    if (Leff < V) {
      key_l = radix_select(ar, V, vec, (u64)Leff, sh,
                           [&](int, float v, uint32_t &key, u64 &w) {
                             key = ord_key(v);
                             w = 1ull;
                             return true;
                           });
      const u64 need = sh.sel.target;   // how many of the tied ids make it
      const u64 tied = sh.sel.bin_w;
      __syncthreads();
      if (tied > need) {
        // the need-th lowest id among the ties = need-th largest ~id
        const uint32_t key_i = radix_select(
            ar, V, vec, need, sh, [&](int idx, float v, uint32_t &key, u64 &w) {
              key = ~(uint32_t)idx;
              w = 1ull;
              return ord_key(v) == key_l;
            });
        id_cut = (int)~key_i;
      }
    }
    if (tid == 0) sh.cand_n = 0;
    __syncthreads();
    for_each_f32(ar, V, vec, [&](int idx, float v) {
      const uint32_t key = ord_key(v);
      if (key > key_l || (key == key_l && idx <= id_cut)) {
        const int pos = atomicAdd(&sh.cand_n, 1);
        if (pos < SB_MAXL) { sh.cand_key[pos] = key; sh.cand_id[pos] = idx; }
      }
    });
    __syncthreads();
    const int n = sh.cand_n < Leff ? sh.cand_n : Leff;
    if (tid < L) {
      if (tid < n) {
        const uint32_t key = sh.cand_key[tid];
        const int id = sh.cand_id[tid];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
          const uint32_t kj = sh.cand_key[j];
          rank += (kj > key || (kj == key && sh.cand_id[j] < id)) ? 1 : 0;
        }
        orow[SB_OUT_FIXED + rank] = id;
        orow[SB_OUT_FIXED + L + rank] = __float_as_int(key_value(key) - lse);
      } else {
        // V < L: pad
        orow[SB_OUT_FIXED + tid] = -1;
        orow[SB_OUT_FIXED + L + tid] = __float_as_int(-INFINITY);
      }
    }
  }
}

}  // namespace

// logits [B, V] bf16/f32 on the GPU; params_cpu [B, 10] int32 and the
// optional CSR pen_cpu = [offsets(B+1) | ids(nnz) | counts(nnz)] int32 are
// host-built and checked here, on the host copy, before anything is
// uploaded. Returns the packed int32 output [B, 4 + 2L] on the GPU.
at::Tensor sample_batch(at::Tensor logits, at::Tensor params_cpu,
                        c10::optional<at::Tensor> pen_cpu, int64_t num_logprobs) {
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2,
              "sample_batch: contiguous [B, V] GPU logits");
  TORCH_CHECK(logits.scalar_type() == at::kBFloat16 ||
                  logits.scalar_type() == at::kFloat,
              "sample_batch: logits must be bf16 or f32");
  const int64_t B64 = logits.size(0), V64 = logits.size(1);
  TORCH_CHECK(B64 >= 1 && V64 >= 1, "sample_batch: empty logits");
  TORCH_CHECK(V64 < (1ll << 30) && B64 < (1ll << 24), "sample_batch: shape too large");
  TORCH_CHECK(num_logprobs >= 0 && num_logprobs <= SB_MAXL,
              "sample_batch: num_logprobs must be in [0, ", SB_MAXL, "]");
  TORCH_CHECK(params_cpu.device().is_cpu() && params_cpu.is_contiguous() &&
                  params_cpu.scalar_type() == at::kInt && params_cpu.dim() == 2 &&
                  params_cpu.size(0) == B64 && params_cpu.size(1) == SB_PARAM_WORDS,
              "sample_batch: params must be a contiguous CPU int32 [B, ",
              SB_PARAM_WORDS, "] tensor");
  const int B = (int)B64, V = (int)V64, L = (int)num_logprobs;

  at::Tensor pen_dev;
  if (pen_cpu.has_value()) {
    const at::Tensor &p = *pen_cpu;
    TORCH_CHECK(p.device().is_cpu() && p.is_contiguous() &&
                    p.scalar_type() == at::kInt && p.dim() == 1,
                "sample_batch: penalties must be a contiguous CPU int32 vector");
    const int64_t rest = p.numel() - (B64 + 1);
    TORCH_CHECK(rest >= 0 && rest % 2 == 0 && rest / 2 < (1ll << 30),
                "sample_batch: penalty CSR size does not match the batch");
    const int64_t nnz = rest / 2;
    const int32_t *d = p.data_ptr<int32_t>();
    TORCH_CHECK(d[0] == 0 && d[B] == nnz, "sample_batch: bad CSR offsets");
    for (int i = 0; i < B; ++i)
      TORCH_CHECK(d[i] <= d[i + 1], "sample_batch: CSR offsets must not decrease");
    const int32_t *ids = d + B + 1, *cnt = ids + nnz;
    for (int64_t j = 0; j < nnz; ++j) {
      TORCH_CHECK(ids[j] >= 0 && ids[j] < V, "sample_batch: penalty id ", ids[j],
                  " outside [0, ", V, ")");
      TORCH_CHECK(cnt[j] >= 0, "sample_batch: negative penalty count");
    }
    pen_dev = p.to(logits.device(), /*non_blocking=*/true);
  }
  at::Tensor params = params_cpu.to(logits.device(), /*non_blocking=*/true);
  auto ws = at::empty({B64, V64}, logits.options().dtype(at::kFloat));
  auto out = at::empty({B64, SB_OUT_FIXED + 2 * (int64_t)L},
                       logits.options().dtype(at::kInt));

  const bool bf16 = logits.scalar_type() == at::kBFloat16;
  const int W = bf16 ? 8 : 4;
  const int ws_vec = (V % 4 == 0) && ((uintptr_t)ws.data_ptr() % 16 == 0);
  const int in_vec = ws_vec && (V % W == 0) &&
                     ((uintptr_t)logits.data_ptr() % 16 == 0);
  const int32_t *csr = pen_dev.defined() ? pen_dev.data_ptr<int32_t>() : nullptr;
  auto stream = at::hip::getCurrentHIPStream();
  if (bf16) {
    hipLaunchKernelGGL((sample_batch_kernel<uint16_t>), dim3(B), dim3(SB_BLOCK), 0,
                       stream, (const uint16_t *)logits.data_ptr(),
                       ws.data_ptr<float>(), params.data_ptr<int32_t>(), csr,
                       out.data_ptr<int32_t>(), B, V, L, in_vec, ws_vec);
  } else {
    hipLaunchKernelGGL((sample_batch_kernel<float>), dim3(B), dim3(SB_BLOCK), 0,
                       stream, (const float *)logits.data_ptr(),
                       ws.data_ptr<float>(), params.data_ptr<int32_t>(), csr,
                       out.data_ptr<int32_t>(), B, V, L, in_vec, ws_vec);
  }
  return out;
}
