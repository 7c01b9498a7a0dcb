// Multi-query paged decode attention ("verify") for CDNA4 (gfx950): the
// attention of one speculative-decoding step. Sequence b brings q_lens[b]
// (0..T) query rows, the last q_lens[b] positions of its seq_lens[b] cached
// keys; row t is the query at position seq_lens[b] - q_lens[b] + t and sees
// keys [0, that position]. Rows t >= q_lens[b] are padding: they read
// nothing and come back as zeros. Every length is read from device memory,
// so one captured launch serves any mix of lengths.
//
// Geometry: a workgroup serves one (sequence, kv head, row tile, key split).
// The G*T query rows that share a kv head are numbered rr = t*G + g and
// packed into the column dimension of the MFMAs, 16 (RT=1) or 32 (RT=2) to
// a workgroup; more rows than that are tiled over grid.y, never looped over
// the key stream. Each K/V block is read ONCE for all rows of the tile:
//  * a wave owns whole 16-token cache blocks (block blk_lo + wave, step 4),
//    two in flight: raw 16 B fragments sit in a 2-deep register ring and
//    are converted at use;
//  * S[16 tok][16 rows] per row group is one mfma_f32_16x16x32_bf16 chain
//    over DH with K read straight in A-fragment order, as in the MFMA
//    decode kernel (attention_decode.hip); the softmax state (m, l) is per
//    row = per lane, with a per-row key limit instead of one limit;
//  * O^T[d][row] accumulates in mfma_f32_32x32x16_bf16. Transposed-V blocks
//    ([DH][16]) are the A fragment as they lie in memory. Plain blocks
//    ([16][DH]) are loaded with the same 16 B loads and transposed through
//    a per-wave LDS image (2-byte reads), which costs LDS time the
//    transposed layout does not pay;
//  * the block table is staged to LDS once, ids clamped to the pool;
//  * keys at or past seq_len are zeroed in V (0 x NaN would poison PV) and
//    masked in S; keys between a row's limit and seq_len are masked in S;
//  * waves merge through LDS in accumulator lane order, two d-tiles at a
//    time; with nsplit > 1 the workgroup writes fp32 partials (O, m, l)
//    and verify_combine_kernel merges them. A split without keys for a row
//    writes m = -inf and is skipped there.
//
// q, out: [B, T, Hq, DH] bf16. k_cache [blk, Hkv, 16, DH]; v_cache the same
// or [blk, Hkv, DH, 16]. DH in {64, 128}, 1 <= T <= 8, any Hq % Hkv == 0.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int NW = 4;
constexpr int BS = 16;          // tokens per cache block
constexpr int BT_LDS = 512;     // staged block-table entries
constexpr int MAX_T = 8;
constexpr int MAX_NSPLIT = 64;

typedef __attribute__((ext_vector_type(8))) __bf16 vf_bf16x8v;
typedef __attribute__((ext_vector_type(16))) float vf_f32x16v;
typedef __attribute__((ext_vector_type(4))) float vf_f32x4v;

RB_DEV unsigned vf_pack_bf16(float lo, float hi) {
  union { __bf16 b; unsigned short u; } a, b;
  a.b = (__bf16)lo;
  b.b = (__bf16)hi;
  return ((unsigned)b.u << 16) | a.u;
}

RB_DEV vf_bf16x8v vf_frag(const uint32_t *raw) {
  union { unsigned u[4]; vf_bf16x8v v; } c;
  c.u[0] = raw[0]; c.u[1] = raw[1]; c.u[2] = raw[2]; c.u[3] = raw[3];
  return c.v;
}

// partial row: DH floats of O, then m, l, and two pad floats (16 B rows)
__host__ __device__ constexpr int part_stride(int dh) { return dh + 4; }

template <int DH, bool VT, int RT>
__global__ __launch_bounds__(BLOCK) void paged_verify_kernel(
    const uint16_t *__restrict__ q, const uint16_t *__restrict__ k_cache,
    const uint16_t *__restrict__ v_cache,
    const int32_t *__restrict__ block_tables,
    const int32_t *__restrict__ seq_lens, const int32_t *__restrict__ q_lens,
    uint16_t *__restrict__ out, float *__restrict__ partial, int T, int G,
    int hkv, int ntile, int max_blocks, int num_blocks, int nsplit,
    float scale) {
  constexpr int KS32 = DH / 32;           // QK^T contraction steps
  constexpr int DT = DH / 32;             // O^T 32-row d-tiles
  constexpr int R = 16 * RT;              // query rows per workgroup
  constexpr int VP = DH + 8;              // plain-V LDS row pitch (u16)

  const int b = blockIdx.x;
  const int h_kv = (int)blockIdx.y / ntile;
  const int tile = (int)blockIdx.y % ntile;
  const int split = blockIdx.z;
  const int Hq = hkv * G;
  const int hq0 = h_kv * G;
  const int rows = G * T;
  const int rbase = tile * R;

  const int tid = (int)threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int i16 = lane & 15;
  const int h16 = lane >> 4;
  const int h32 = lane >> 5;
  const int c32 = lane & 31;

  // ---- lengths (device memory), clamped to what the tensors can hold ----
  int seq_len = min(max(seq_lens[b], 0), max_blocks * BS);
  const int q_len = min(min(max(q_lens[b], 0), T), seq_len);
  const int ctx = seq_len - q_len;
  if (q_len == 0) seq_len = 0;

  // keys this tile needs: up to its last real row's position
  const int t_lo = rbase / G;
  const int t_hi = min(min((rbase + R - 1) / G, T - 1), q_len - 1);
  const int kmax = (t_hi >= t_lo) ? ctx + t_hi + 1 : 0;
  const int nblk = (kmax + BS - 1) / BS;
  const int chunk = (nblk + nsplit - 1) / nsplit;
  const int blk_lo = split * chunk;
  const int blk_hi = min(nblk, blk_lo + chunk) - 1;   // < blk_lo: no keys

  __shared__ int32_t bt_lds[BT_LDS];
  // cross-wave merge region [NW][32 slots][64 lanes]; the plain-V transpose
  // images ([NW][16][VP] u16) alias its front during the key loop
  __shared__ __attribute__((aligned(16))) float mrg[NW * 32 * 64];
  __shared__ float ml[NW][32][2];
  static_assert(NW * BS * VP * 2 <= NW * 32 * 64 * 4, "V image fits");

  const int32_t *bt = block_tables + (int64_t)b * max_blocks;
  if (blk_hi >= blk_lo) {
    const int nbt = min(blk_hi - blk_lo + 1, BT_LDS);
    for (int i = tid; i < nbt; i += BLOCK)
      bt_lds[i] = min(max(bt[blk_lo + i], 0), num_blocks - 1);
  }
  __syncthreads();

  // ---- per-row state: row group st, row = rbase + st*16 + i16 ----------
  int lim[RT];                      // keys [0, lim) are visible to the row
  vf_bf16x8v qf[RT][KS32];
#pragma unroll
  for (int st = 0; st < RT; ++st) {
    const int rr = rbase + st * 16 + i16;
    const bool rv = rr < rows;
    const int t = rv ? rr / G : 0;
    const int g = rv ? rr % G : 0;
    lim[st] = (rv && t < q_len) ? ctx + t + 1 : 0;
    const uint16_t *qp = q + (((int64_t)b * T + t) * Hq + hq0 + g) * DH;
#pragma unroll
    for (int ks = 0; ks < KS32; ++ks) {
      uint32_t raw[4] = {0u, 0u, 0u, 0u};
      if (rv)
        rb::ld_words<4>(raw, reinterpret_cast<const uint8_t *>(
                                 qp + ks * 32 + h16 * 8));
      qf[st][ks] = vf_frag(raw);
    }
  }

  vf_f32x16v acc_o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc_o[dt] = (vf_f32x16v)(0.0f);
  float m_run[RT], l_run[RT];
#pragma unroll
  for (int st = 0; st < RT; ++st) { m_run[st] = -INFINITY; l_run[st] = 0.0f; }

  uint32_t kfr[2][KS32][4], vfr[2][DT][4];
  uint16_t *vimg = reinterpret_cast<uint16_t *>(mrg) + wid * BS * VP;

  auto fetch = [&](int bi, int slot) {
    const int bi_l = bi - blk_lo;
    const int blk = (bi_l < BT_LDS)
        ? bt_lds[bi_l] : min(max(bt[bi], 0), num_blocks - 1);
    const uint16_t *kb = k_cache + ((int64_t)blk * hkv + h_kv) * BS * DH;
    const uint16_t *vb = v_cache + ((int64_t)blk * hkv + h_kv) * BS * DH;
#pragma unroll
    for (int ks = 0; ks < KS32; ++ks)
      rb::ld_words<4>(kfr[slot][ks], reinterpret_cast<const uint8_t *>(
          kb + i16 * DH + ks * 32 + h16 * 8));
    if constexpr (VT) {
      // [DH][16] block: d row (dt*32 + c32), keys h32*8 .. +8
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        rb::ld_words<4>(vfr[slot][dt], reinterpret_cast<const uint8_t *>(
            vb + (dt * 32 + c32) * BS + h32 * 8));
    } else {
      // [16][DH] block: the wave's DH*2 16 B chunks in memory order
#pragma unroll
      for (int p = 0; p < DT; ++p)
        rb::ld_words<4>(vfr[slot][p], reinterpret_cast<const uint8_t *>(
            vb + (p * 64 + lane) * 8));
    }
  };

  auto step = [&](int bi, int cur) {
    if (bi + NW <= blk_hi) fetch(bi + NW, cur ^ 1);
    const int tok0 = bi * BS;

    // ---- S[16 tok][16 rows] per row group, mask, online softmax ---------
    unsigned w01[RT], w23[RT];
    float alpha[RT];
#pragma unroll
    for (int st = 0; st < RT; ++st) {
      vf_f32x4v s4 = (vf_f32x4v)(0.0f);
#pragma unroll
      for (int ks = 0; ks < KS32; ++ks)
        s4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            vf_frag(kfr[cur][ks]), qf[st][ks], s4, 0, 0, 0);
      float p4[4];
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int tk = tok0 + h16 * 4 + r;
        p4[r] = (tk < lim[st]) ? s4[r] * scale : -INFINITY;
        mx = fmaxf(mx, p4[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m_run[st], mx);
      const float ms = (mn == -INFINITY) ? 0.0f : mn;   // no key yet: p = 0
      alpha[st] = (m_run[st] == -INFINITY) ? ((mn == -INFINITY) ? 1.0f : 0.0f)
                                           : __expf(m_run[st] - ms);
      float psum = 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p4[r] = (p4[r] == -INFINITY) ? 0.0f : __expf(p4[r] - ms);
        psum += p4[r];
      }
      psum += __shfl_xor(psum, 16, 64);
      psum += __shfl_xor(psum, 32, 64);
      l_run[st] = l_run[st] * alpha[st] + psum;
      m_run[st] = mn;
      w01[st] = vf_pack_bf16(p4[0], p4[1]);
      w23[st] = vf_pack_bf16(p4[2], p4[3]);
    }

    // ---- rescale O^T: column c32 is row (c32>>4)*16 + (c32&15) ----------
    float alpha_o = alpha[0];
    if constexpr (RT == 2) alpha_o = (c32 >> 4) ? alpha[1] : alpha[0];
    if (alpha_o != 1.0f) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_o[dt][r] *= alpha_o;
    }

    // ---- P[tok][row] -> B fragment of PV (k = tok, col = row) -----------
    // lane (row&15) + 16*qd of group (row>>4) holds tokens 4*qd .. +4; the
    // target lane needs tokens h32*8 .. +8 of row c32.
    const int s1 = (c32 & 15) + 32 * h32;
    const int s2 = s1 + 16;
    unsigned pw[4];
    pw[0] = __shfl(w01[0], s1, 64);
    pw[1] = __shfl(w23[0], s1, 64);
    pw[2] = __shfl(w01[0], s2, 64);
    pw[3] = __shfl(w23[0], s2, 64);
    if constexpr (RT == 2) {
      const unsigned x0 = __shfl(w01[1], s1, 64);
      const unsigned x1 = __shfl(w23[1], s1, 64);
      const unsigned x2 = __shfl(w01[1], s2, 64);
      const unsigned x3 = __shfl(w23[1], s2, 64);
      if (c32 >> 4) { pw[0] = x0; pw[1] = x1; pw[2] = x2; pw[3] = x3; }
    }
    const vf_bf16x8v pf = vf_frag(pw);

    // ---- V^T fragments: keys >= seq_len are zeroed, never multiplied ----
    const bool tail = tok0 + BS > seq_len;     // wave-uniform
    if constexpr (VT) {
      if (tail) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int t0 = tok0 + h32 * 8 + 2 * w;
          const unsigned mask = (t0 < seq_len ? 0xFFFFu : 0u) |
                                (t0 + 1 < seq_len ? 0xFFFF0000u : 0u);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) vfr[cur][dt][w] &= mask;
        }
      }
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        acc_o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            vf_frag(vfr[cur][dt]), pf, acc_o[dt], 0, 0, 0);
    } else {
      constexpr int CPR = DH / 8;              // 16 B chunks per token row
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int p = 0; p < DT; ++p) {
        const int c = p * 64 + lane;
        const int tk = c / CPR;
        const int d0 = (c % CPR) * 8;
        typedef __attribute__((ext_vector_type(4))) unsigned int u32x4i;
        u32x4i w = {vfr[cur][p][0], vfr[cur][p][1], vfr[cur][p][2],
                    vfr[cur][p][3]};
        if (tail && tok0 + tk >= seq_len) w = (u32x4i)(0u);
        *reinterpret_cast<u32x4i *>(vimg + tk * VP + d0) = w;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        unsigned vw[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const uint16_t *src = vimg + (h32 * 8 + 2 * w) * VP + dt * 32 + c32;
          vw[w] = (unsigned)src[0] | ((unsigned)src[VP] << 16);
        }
        acc_o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            vf_frag(vw), pf, acc_o[dt], 0, 0, 0);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  };

  const int bi0 = blk_lo + wid;
  if (bi0 <= blk_hi) fetch(bi0, 0);
  for (int bi = bi0; bi <= blk_hi; bi += 2 * NW) {
    step(bi, 0);
    if (bi + NW <= blk_hi) step(bi + NW, 1);
  }

  // ---- cross-wave merge -------------------------------------------------
  __syncthreads();                       // V images (aliasing mrg) are done
  if (lane < 16) {
#pragma unroll
    for (int st = 0; st < RT; ++st) {
      ml[wid][st * 16 + lane][0] = m_run[st];
      ml[wid][st * 16 + lane][1] = l_run[st];
    }
  } else if (RT == 1 && lane < 32) {     // unused columns merge to nothing
    ml[wid][lane][0] = -INFINITY;
    ml[wid][lane][1] = 0.0f;
  }

  // this lane's output row: column c32 of the accumulators
  const int rr = rbase + c32;
  const bool row_ok = rr < rows && c32 < R;
  const int ot = row_ok ? rr / G : 0;
  const int og = row_ok ? rr % G : 0;
  const int64_t orow = ((int64_t)b * T + ot) * Hq + hq0 + og;

  float aw[NW], mm = -INFINITY, ll = 0.0f;
  constexpr int PASSES = DT / 2;
#pragma unroll
  for (int ps = 0; ps < PASSES; ++ps) {
    if (ps > 0) __syncthreads();         // the previous pass was read
#pragma unroll
    for (int dl = 0; dl < 2; ++dl)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        mrg[(wid * 32 + dl * 16 + r) * 64 + lane] = acc_o[ps * 2 + dl][r];
    __syncthreads();
    if (ps == 0) {
#pragma unroll
      for (int w = 0; w < NW; ++w) mm = fmaxf(mm, ml[w][c32][0]);
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const float mw = ml[w][c32][0];
        aw[w] = (mw == -INFINITY) ? 0.0f : __expf(mw - mm);
        ll += ml[w][c32][1] * aw[w];
      }
    }
    // wave w merges slots w*8 .. +8: d-tile w>>1, registers (w&1)*8 .. +8
    const int dl = wid >> 1;
#pragma unroll
    for (int gq = 0; gq < 2; ++gq) {
      const int rg = (wid & 1) * 2 + gq;         // register group r>>2
      float o4[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int slot = dl * 16 + rg * 4 + e;
        float acc = 0.0f;
#pragma unroll
        for (int w = 0; w < NW; ++w)
          acc += (aw[w] != 0.0f) ? mrg[(w * 32 + slot) * 64 + lane] * aw[w]
                                 : 0.0f;
        o4[e] = acc;
      }
      const int d = (ps * 2 + dl) * 32 + 8 * rg + 4 * h32;
      if (row_ok) {
        if (partial != nullptr) {
          float *pp = partial +
              (orow * nsplit + split) * part_stride(DH) + d;
          *reinterpret_cast<float4 *>(pp) =
              make_float4(o4[0], o4[1], o4[2], o4[3]);
        } else {
          const float inv_l = (ll > 0.0f) ? 1.0f / ll : 0.0f;
          uint2 pk;
          pk.x = (unsigned)rb::f32_to_bf16(o4[0] * inv_l) |
                 ((unsigned)rb::f32_to_bf16(o4[1] * inv_l) << 16);
          pk.y = (unsigned)rb::f32_to_bf16(o4[2] * inv_l) |
                 ((unsigned)rb::f32_to_bf16(o4[3] * inv_l) << 16);
          *reinterpret_cast<uint2 *>(out + orow * DH + d) = pk;
        }
      }
    }
    if (ps == 0 && wid == 0 && h32 == 0 && row_ok && partial != nullptr) {
      float *pp = partial + (orow * nsplit + split) * part_stride(DH);
      pp[DH] = mm;
      pp[DH + 1] = ll;
    }
  }
}

// Merge the nsplit partials of one (b, t, hq) row. A partial with
// m == -inf had no key for the row and is skipped; a row without any key
// (padding) is stored as zeros.
__global__ void verify_combine_kernel(const float *__restrict__ partial,
                                      uint16_t *__restrict__ out, int nsplit,
                                      int dh) {
  const int64_t row = blockIdx.x;
  const int ps = part_stride(dh);
  const float *p = partial + row * (int64_t)nsplit * ps;
  float mm = -INFINITY;
  for (int s = 0; s < nsplit; ++s) mm = fmaxf(mm, p[s * ps + dh]);
  float ll = 0.f;
  for (int s = 0; s < nsplit; ++s)
    if (p[s * ps + dh] != -INFINITY)
      ll += p[s * ps + dh + 1] * __expf(p[s * ps + dh] - mm);
  const float inv_l = (ll > 0.f) ? 1.0f / ll : 0.f;
  for (int d = threadIdx.x; d < dh; d += blockDim.x) {
    float o = 0.f;
    for (int s = 0; s < nsplit; ++s) {
      const float ms = p[s * ps + dh];
      if (ms != -INFINITY) o += p[s * ps + d] * __expf(ms - mm);
    }
    out[row * dh + d] = rb::f32_to_bf16(o * inv_l);
  }
}

template <int DH, bool VT, int RT>
void launch_verify(const at::Tensor &q, const at::Tensor &k_cache,
                   const at::Tensor &v_cache, const at::Tensor &block_tables,
                   const at::Tensor &seq_lens, const at::Tensor &q_lens,
                   at::Tensor &out, int nsplit, float scale,
                   hipStream_t stream) {
  const int B = (int)q.size(0), T = (int)q.size(1), Hq = (int)q.size(2);
  const int hkv = (int)k_cache.size(1);
  const int G = Hq / hkv;
  const int ntile = (G * T + 16 * RT - 1) / (16 * RT);
  float *part = nullptr;
  at::Tensor partial;
  if (nsplit > 1) {
    partial = at::empty({(int64_t)B * T * Hq, nsplit, part_stride(DH)},
                        q.options().dtype(at::kFloat));
    part = partial.data_ptr<float>();
  }
  hipLaunchKernelGGL((paged_verify_kernel<DH, VT, RT>),
                     dim3(B, hkv * ntile, nsplit), dim3(BLOCK), 0, stream,
                     (const uint16_t *)q.data_ptr(),
                     (const uint16_t *)k_cache.data_ptr(),
                     (const uint16_t *)v_cache.data_ptr(),
                     block_tables.data_ptr<int32_t>(),
                     seq_lens.data_ptr<int32_t>(), q_lens.data_ptr<int32_t>(),
                     (uint16_t *)out.data_ptr(), part, T, G, hkv, ntile,
                     (int)block_tables.size(1), (int)k_cache.size(0), nsplit,
                     scale);
  if (nsplit > 1)
    hipLaunchKernelGGL(verify_combine_kernel, dim3(B * T * Hq), dim3(64), 0,
                       stream, part, (uint16_t *)out.data_ptr(), nsplit, DH);
}

}  // namespace

// Host checks cover shapes, dtypes, contiguity, table height and T; lengths
// stay on the device (the kernel clamps them to the table), so the call
// never waits and can be captured.
at::Tensor paged_verify(at::Tensor q, at::Tensor k_cache, at::Tensor v_cache,
                        at::Tensor block_tables, at::Tensor seq_lens,
                        at::Tensor q_lens, int64_t nsplit, double scale) {
  const char *op = "paged_verify";
  TORCH_CHECK(k_cache.scalar_type() != at::kByte &&
                  v_cache.scalar_type() != at::kByte,
              op, ": fp8 KV caches are not supported");
  TORCH_CHECK(q.is_cuda() && k_cache.is_cuda() && v_cache.is_cuda() &&
                  block_tables.is_cuda() && seq_lens.is_cuda() &&
                  q_lens.is_cuda(),
              op, ": GPU tensors");
  TORCH_CHECK(k_cache.device() == q.device() &&
                  v_cache.device() == q.device() &&
                  block_tables.device() == q.device() &&
                  seq_lens.device() == q.device() &&
                  q_lens.device() == q.device(),
              op, ": all tensors on q's device");
  TORCH_CHECK(q.is_contiguous() && k_cache.is_contiguous() &&
                  v_cache.is_contiguous() && block_tables.is_contiguous() &&
                  seq_lens.is_contiguous() && q_lens.is_contiguous(),
              op, ": contiguous tensors");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16 &&
                  k_cache.scalar_type() == at::kBFloat16 &&
                  v_cache.scalar_type() == at::kBFloat16,
              op, ": bf16 only");
  TORCH_CHECK(q.dim() == 4, op, ": q must be [B, T, Hq, DH]");
  TORCH_CHECK(k_cache.dim() == 4 && v_cache.dim() == 4,
              op, ": caches must be 4-d");
  TORCH_CHECK(block_tables.scalar_type() == at::kInt &&
                  block_tables.dim() == 2,
              op, ": block_tables must be int32 [B, maxb]");
  TORCH_CHECK(seq_lens.scalar_type() == at::kInt && seq_lens.dim() == 1,
              op, ": seq_lens must be int32 [B]");
  TORCH_CHECK(q_lens.scalar_type() == at::kInt && q_lens.dim() == 1,
              op, ": q_lens must be int32 [B]");
  const int64_t B = q.size(0), T = q.size(1), Hq = q.size(2), DH = q.size(3);
  const int64_t Hkv = k_cache.size(1);
  TORCH_CHECK(B >= 1 && B < (int64_t(1) << 20), op, ": B out of range");
  TORCH_CHECK(T >= 1 && T <= MAX_T, op, ": T must be 1..", MAX_T, ", got ", T);
  TORCH_CHECK(DH == 64 || DH == 128, op, ": Dh must be 64 or 128, got ", DH);
  TORCH_CHECK(block_tables.size(0) >= B, op, ": block_tables has ",
              block_tables.size(0), " rows for ", B, " sequences");
  TORCH_CHECK(block_tables.size(1) >= 1 &&
                  block_tables.size(1) < (int64_t(1) << 26),
              op, ": block_tables width out of range");
  TORCH_CHECK(seq_lens.numel() >= B && q_lens.numel() >= B,
              op, ": seq_lens and q_lens need B entries");
  TORCH_CHECK(k_cache.size(0) >= 1 && k_cache.size(2) == BS &&
                  k_cache.size(3) == DH,
              op, ": k_cache must be [blk, Hkv, 16, DH]");
  TORCH_CHECK(Hkv >= 1 && Hq % Hkv == 0, op, ": Hq % Hkv");
  const bool vt = v_cache.size(2) == DH && v_cache.size(3) == BS;
  TORCH_CHECK(v_cache.size(0) == k_cache.size(0) && v_cache.size(1) == Hkv &&
                  (vt || (v_cache.size(2) == BS && v_cache.size(3) == DH)),
              op, ": v_cache must be [blk, Hkv, 16, DH] or [blk, Hkv, DH, 16]");
  TORCH_CHECK(nsplit >= 1 && nsplit <= MAX_NSPLIT, op, ": nsplit must be 1..",
              MAX_NSPLIT);
  const int64_t rows = (Hq / Hkv) * T;
  const int rt = rows > 16 ? 2 : 1;
  TORCH_CHECK(Hkv * ((rows + 16 * rt - 1) / (16 * rt)) <= 65535,
              op, ": too many heads");
  auto out = at::empty_like(q);
  auto stream = at::hip::getCurrentHIPStream();

#define RB_VERIFY(DHV)                                                        \
  do {                                                                        \
    if (vt) {                                                                 \
      if (rt == 2)                                                            \
        launch_verify<DHV, true, 2>(q, k_cache, v_cache, block_tables,        \
                                    seq_lens, q_lens, out, (int)nsplit,       \
                                    (float)scale, stream);                    \
      else                                                                    \
        launch_verify<DHV, true, 1>(q, k_cache, v_cache, block_tables,        \
                                    seq_lens, q_lens, out, (int)nsplit,       \
                                    (float)scale, stream);                    \
    } else {                                                                  \
      if (rt == 2)                                                            \
        launch_verify<DHV, false, 2>(q, k_cache, v_cache, block_tables,       \
                                     seq_lens, q_lens, out, (int)nsplit,      \
                                     (float)scale, stream);                   \
      else                                                                    \
        launch_verify<DHV, false, 1>(q, k_cache, v_cache, block_tables,       \
                                     seq_lens, q_lens, out, (int)nsplit,      \
                                     (float)scale, stream);                   \
    }                                                                         \
  } while (0)
  if (DH == 128) RB_VERIFY(128); else RB_VERIFY(64);
#undef RB_VERIFY
  return out;
}
