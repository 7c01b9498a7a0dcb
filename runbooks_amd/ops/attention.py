"""Attention ops.

* ``causal_attention``: batch-uniform causal GQA attention used by the
  trainer forward/backward. Built from explicit GEMMs (hipBLASLt/rocBLAS
  via torch.matmul — plain library GEMMs) + fused softmax, chunked over
  query blocks to bound the S^2 score memory. No Triton, no SDPA dispatch.
  A hand-written MFMA flash-attention prefill kernel supersedes this on
  the serving path (see csrc/attention_prefill.hip).

* ``paged_decode``: single-token decode against the paged KV cache —
  gfx950 HIP kernel on GPU (csrc/attention_decode.hip), fp32 reference on
  CPU (also the numerics oracle for the GPU test).

* ``paged_prefill``: one chunk of one sequence's prompt attending over the
  paged KV cache (cached prefix + the chunk itself) — gfx950 MFMA kernel
  on GPU (csrc/attention_prefill_paged.hip), fp32 reference on CPU.

* ``paged_prefill_batch``: the same for several sequences' chunks packed
  into one token dimension, one launch; lengths come from a host-built
  ``paged_prefill_plan``.
"""
from __future__ import annotations

import math

import torch

from . import _backend


class _FlashAttnTrain(torch.autograd.Function):
    """Differentiable causal GQA attention on the gfx950 MFMA kernels.

    Forward: flash_fwd_train (attention_prefill.hip, saves LSE).
    Backward: fa_bwd (attention_bwd.hip, FA2-style recompute); GQA dk/dv
    come back per-q-head and are group-summed to the kv heads here.
    """

    @staticmethod
    def forward(ctx, q, k, v, scale):
        qc, kc, vc = q.contiguous(), k.contiguous(), v.contiguous()
        out, lse = _backend.ext().flash_fwd_train(qc, kc, vc, float(scale))
        ctx.save_for_backward(qc, kc, vc, out, lse)
        ctx.scale = float(scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        dq, dk, dv = _backend.ext().fa_bwd(dout.contiguous(), q, k, v, out,
                                           lse, ctx.scale)
        hq, hkv = q.shape[2], k.shape[2]
        if hkv != hq:  # sum the q-head group (GQA/MQA)
            g = hq // hkv
            b, s = dk.shape[0], dk.shape[1]
            dk = dk.view(b, s, hkv, g, -1).sum(dim=3)
            dv = dv.view(b, s, hkv, g, -1).sum(dim=3)
        return dq, dk, dv, None


def causal_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                     scale: float | None = None, q_block: int = 256) -> torch.Tensor:
    """q [B, S, Hq, Dh]; k, v [B, S, Hkv, Dh] -> [B, S, Hq, Dh].

    Differentiable. GPU bf16 (Dh 64/128) runs the MFMA flash kernels;
    otherwise the chunked fp32 reference below (also the numerics oracle
    for the GPU test). Dh=256 has an MFMA INFERENCE prefill
    (flash_prefill) but trains on the reference (fa_bwd has no 256
    tile yet).
    """
    if _backend.use_hip(q) and q.shape[-1] in (64, 128) \
            and q.dtype == torch.bfloat16:
        if scale is None:
            scale = 1.0 / math.sqrt(q.shape[-1])
        return _FlashAttnTrain.apply(q, k, v, scale)
    return causal_attention_ref(q, k, v, scale=scale, q_block=q_block)


def causal_attention_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                         scale: float | None = None,
                         q_block: int = 256) -> torch.Tensor:
    """Chunked eager reference (fp32 softmax), differentiable."""
    B, S, Hq, Dh = q.shape
    Hkv = k.shape[2]
    if scale is None:
        scale = 1.0 / math.sqrt(Dh)
    g = Hq // Hkv
    if g > 1:
        k = k.repeat_interleave(g, dim=2)
        v = v.repeat_interleave(g, dim=2)
    qt = q.transpose(1, 2)  # [B, H, S, D]
    kt = k.transpose(1, 2)
    vt = v.transpose(1, 2)

    outs = []
    for s0 in range(0, S, q_block):
        s1 = min(S, s0 + q_block)
        qb = qt[:, :, s0:s1]                              # [B,H,bs,D]
        scores = torch.matmul(qb, kt[:, :, :s1].transpose(-1, -2)).float() * scale
        mask = torch.ones(s1 - s0, s1, dtype=torch.bool, device=q.device)
        mask = torch.triu(mask, diagonal=s0 + 1)
        scores = scores.masked_fill(mask, float("-inf"))
        p = torch.softmax(scores, dim=-1).to(vt.dtype)
        outs.append(torch.matmul(p, vt[:, :, :s1]))
    return torch.cat(outs, dim=2).transpose(1, 2).contiguous()


def flash_prefill(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                  scale: float | None = None) -> torch.Tensor:
    """Causal GQA attention, inference-only (no autograd).

    q [B, S, Hq, Dh] bf16 on GPU -> gfx950 MFMA flash kernel
    (csrc/attention_prefill.hip); CPU falls back to the chunked reference.
    """
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if _backend.use_hip(q) and q.shape[-1] in (64, 128, 256) \
            and q.dtype == torch.bfloat16:
        return _backend.ext().flash_prefill(
            q.contiguous(), k.contiguous(), v.contiguous(), float(scale))
    return causal_attention_ref(q, k, v, scale=scale)


def paged_decode_ref(q, k_cache, v_cache, block_tables, seq_lens, scale,
                     seq_starts=None):
    """fp32 reference decode: q [B, Hq, Dh]. fp8 caches (uint8 rows of
    Dh bytes + f32 scale) are dequantized up front. seq_starts (strict
    sliding window) bounds attention to virtual positions
    [start, seq_len)."""
    if k_cache.dtype == torch.uint8:
        from .kvcache import fp8_dequant_cache_ref
        k_cache = fp8_dequant_cache_ref(k_cache)
        v_cache = fp8_dequant_cache_ref(v_cache)
    B, Hq, Dh = q.shape
    _, Hkv, BS, _ = k_cache.shape
    g = Hq // Hkv
    vt = (v_cache.shape[2] == Dh and v_cache.shape[3] == BS
          and Dh != BS)  # transposed-V layout (alloc_kv_cache v_transposed)
    out = torch.empty_like(q)
    for b in range(B):
        n = int(seq_lens[b])
        st = int(seq_starts[b]) if seq_starts is not None else 0
        blocks = block_tables[b, : (n + BS - 1) // BS].long()
        k = k_cache[blocks].transpose(1, 2).reshape(-1, Hkv, Dh)[st:n].float()
        if vt:
            v = v_cache[blocks].permute(0, 3, 1, 2).reshape(
                -1, Hkv, Dh)[st:n].float()
        else:
            v = v_cache[blocks].transpose(1, 2).reshape(
                -1, Hkv, Dh)[st:n].float()
        for h in range(Hq):
            hk = h // g
            s = (k[:, hk] @ q[b, h].float()) * scale
            p = torch.softmax(s, dim=0)
            out[b, h] = (p @ v[:, hk]).to(q.dtype)
    return out


def paged_prefill_ref(q, k_cache, v_cache, block_table, ctx_len, scale=None):
    """fp32 reference for paged_prefill: gather keys [0, ctx_len + T) from
    the cache (plain or transposed-V blocks; fp8 caches are dequantized up
    front), then masked softmax — row r sees keys <= ctx_len + r.
    q [T, Hq, Dh] -> [T, Hq, Dh] in q's dtype."""
    if k_cache.dtype == torch.uint8:
        from .kvcache import fp8_dequant_cache_ref
        k_cache = fp8_dequant_cache_ref(k_cache)
        v_cache = fp8_dequant_cache_ref(v_cache)
    T, Hq, Dh = q.shape
    _, Hkv, BS, _ = k_cache.shape
    if scale is None:
        scale = 1.0 / math.sqrt(Dh)
    ctx_len = int(ctx_len)
    n = ctx_len + T
    vt = (v_cache.shape[2] == Dh and v_cache.shape[3] == BS and Dh != BS)
    blocks = block_table[: (n + BS - 1) // BS].long().to(k_cache.device)
    k = k_cache[blocks].transpose(1, 2).reshape(-1, Hkv, Dh)[:n].float()
    if vt:
        v = v_cache[blocks].permute(0, 3, 1, 2).reshape(-1, Hkv, Dh)[:n].float()
    else:
        v = v_cache[blocks].transpose(1, 2).reshape(-1, Hkv, Dh)[:n].float()
    g = Hq // Hkv
    if g > 1:
        k = k.repeat_interleave(g, dim=1)
        v = v.repeat_interleave(g, dim=1)
    # [Hq, T, n] scores; key j is masked for row r when j > ctx_len + r
    s = torch.einsum("thd,nhd->htn", q.float(), k) * scale
    rows = torch.arange(T, device=q.device)[:, None] + ctx_len
    keys = torch.arange(n, device=q.device)[None, :]
    s = s.masked_fill(keys > rows, float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.einsum("htn,nhd->thd", p, v).to(q.dtype)


def paged_prefill(q, k_cache, v_cache, block_table, ctx_len,
                  scale: float | None = None):
    """Causal attention of one prompt chunk over the paged cache.

    q [T, Hq, Dh]: one sequence, row r at absolute position ctx_len + r.
    The chunk's own k/v must already be appended, so keys [0, ctx_len + T)
    are all read through ``block_table`` (int32 [>= ceil((ctx_len+T)/16)]).
    GPU: bf16 caches in either alloc_kv_cache layout run the gfx950 MFMA
    kernel; fp8 caches raise. CPU: fp32 reference.
    """
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if _backend.use_hip(q):
        if k_cache.dtype == torch.uint8:
            raise NotImplementedError(
                "paged_prefill: fp8 KV caches are not supported")
        return _backend.ext().flash_prefill_paged(
            q.contiguous(), k_cache, v_cache,
            block_table.to(torch.int32).contiguous(), int(ctx_len),
            float(scale))
    return paged_prefill_ref(q, k_cache, v_cache, block_table, ctx_len, scale)


class PagedPrefillPlan:
    """Host-side description of one packed ("varlen") paged prefill:
    sequence b owns packed rows [cu_q[b], cu_q[b+1]) and has ctx_lens[b]
    keys cached before them. ``cpu`` is the int32 tensor
    [cu_q (B+1) | ctx_lens (B) | tile_seq (ntiles) | tile_row0 (ntiles)]
    — one 256-row kernel tile per entry, never spanning two sequences —
    and ``dev`` its copy on the device (None for a CPU plan). Build it with
    ``paged_prefill_plan``; it is immutable and shared by every layer of a
    forward."""

    __slots__ = ("q_lens", "ctx_lens", "cu_q", "num_seqs", "total",
                 "ntiles", "cpu", "dev")

    def __init__(self, q_lens, ctx_lens, device):
        q_lens = [int(t) for t in q_lens]
        ctx_lens = [int(c) for c in ctx_lens]
        if not q_lens or len(q_lens) != len(ctx_lens):
            raise ValueError("paged_prefill_plan: q_lens and ctx_lens must "
                             "be equally long and not empty")
        for t, c in zip(q_lens, ctx_lens):
            if t < 1 or c < 0 or c + t >= 1 << 30:
                raise ValueError(
                    f"paged_prefill_plan: need T >= 1, ctx >= 0 and "
                    f"ctx + T < 2^30, got T={t}, ctx={c}")
        cu = [0]
        for t in q_lens:
            cu.append(cu[-1] + t)
        if cu[-1] >= 1 << 30:
            raise ValueError("paged_prefill_plan: too many packed rows")
        tile_seq, tile_row0 = [], []
        for b, t in enumerate(q_lens):
            for r0 in range(0, t, 256):
                tile_seq.append(b)
                tile_row0.append(r0)
        self.q_lens = tuple(q_lens)
        self.ctx_lens = tuple(ctx_lens)
        self.cu_q = tuple(cu)
        self.num_seqs = len(q_lens)
        self.total = cu[-1]
        self.ntiles = len(tile_seq)
        self.cpu = torch.tensor(cu + ctx_lens + tile_seq + tile_row0,
                                dtype=torch.int32)
        dev = torch.device(device)
        # the forward's one host-to-device copy of the lengths
        self.dev = self.cpu.to(dev) if dev.type != "cpu" else None

    def last_rows(self) -> torch.Tensor:
        """Packed index of each sequence's last row, int64 [B], on the
        plan's device (derived from the copy already there)."""
        t = self.dev if self.dev is not None else self.cpu
        return t[1:self.num_seqs + 1].long() - 1

    def max_blocks(self, block_size: int = 16) -> int:
        """Block-table width the longest sequence needs."""
        return max((c + t + block_size - 1) // block_size
                   for t, c in zip(self.q_lens, self.ctx_lens))


def paged_prefill_plan(q_lens, ctx_lens, device) -> PagedPrefillPlan:
    """Plan a packed paged prefill from host ints: q_lens[b] rows of
    sequence b follow its ctx_lens[b] cached keys. Built once per model
    forward (one small host-to-device copy) and passed to every layer's
    ``paged_prefill_batch``."""
    return PagedPrefillPlan(q_lens, ctx_lens, device)


def _check_batch_shapes(q, block_tables, plan):
    if q.dim() != 3 or q.shape[0] != plan.total:
        raise ValueError(
            f"paged_prefill_batch: q has {tuple(q.shape)} rows/shape, the "
            f"plan packs {plan.total} rows")
    if block_tables.dim() != 2 or block_tables.shape[0] != plan.num_seqs:
        raise ValueError(
            f"paged_prefill_batch: block_tables {tuple(block_tables.shape)} "
            f"for a plan of {plan.num_seqs} sequences")
    if block_tables.shape[1] < plan.max_blocks():
        raise ValueError(
            f"paged_prefill_batch: block_tables has {block_tables.shape[1]} "
            f"columns, the longest sequence needs {plan.max_blocks()}")


def paged_prefill_batch_ref(q, k_cache, v_cache, block_tables, plan,
                            scale=None):
    """fp32 reference for paged_prefill_batch: paged_prefill_ref on each
    sequence's rows, table row and context length."""
    _check_batch_shapes(q, block_tables, plan)
    out = torch.empty_like(q)
    for b in range(plan.num_seqs):
        lo, hi = plan.cu_q[b], plan.cu_q[b + 1]
        out[lo:hi] = paged_prefill_ref(q[lo:hi], k_cache, v_cache,
                                       block_tables[b], plan.ctx_lens[b],
                                       scale)
    return out


def paged_prefill_batch(q, k_cache, v_cache, block_tables, plan,
                        scale: float | None = None):
    """Causal attention of several sequences' prompt chunks, packed back to
    back in q [Ttot, Hq, Dh], over the paged cache in one launch.

    ``plan`` (paged_prefill_plan) holds each sequence's row count and
    cached context; ``block_tables`` int32 [B, >= longest sequence's
    blocks], row b valid below ceil((ctx_b + T_b)/16) — entries past that
    are never read. Every chunk's own k/v must already be appended. GPU:
    the gfx950 MFMA kernel, each sequence bit-identical to ``paged_prefill``
    on it alone; all lengths are checked on the host, nothing waits for the
    device. fp8 caches raise. CPU: fp32 reference.
    """
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if _backend.use_hip(q):
        if k_cache.dtype == torch.uint8:
            raise NotImplementedError(
                "paged_prefill_batch: fp8 KV caches are not supported")
        if plan.dev is None or plan.dev.device != q.device:
            raise ValueError("paged_prefill_batch: the plan was built for "
                             "another device than q's")
        _check_batch_shapes(q, block_tables, plan)
        if block_tables.dtype != torch.int32:
            block_tables = block_tables.to(torch.int32)
        return _backend.ext().flash_prefill_paged_batch(
            q.contiguous(), k_cache, v_cache, block_tables.contiguous(),
            plan.dev, plan.cpu, plan.num_seqs, float(scale))
    return paged_prefill_batch_ref(q, k_cache, v_cache, block_tables, plan,
                                   scale)


VERIFY_MAX_T = 8


def _check_verify_shapes(q, k_cache, block_tables, seq_lens, q_lens):
    """Host-side checks of paged_verify: shapes and dtypes only, never a
    length (those stay on the device)."""
    if q.dim() != 4:
        raise ValueError(f"paged_verify: q must be [B, T, Hq, Dh], got "
                         f"{tuple(q.shape)}")
    B, T, Hq, Dh = q.shape
    if not 1 <= T <= VERIFY_MAX_T:
        raise ValueError(f"paged_verify: T must be 1..{VERIFY_MAX_T}, got {T}")
    if Hq % k_cache.shape[1]:
        raise ValueError("paged_verify: Hq % Hkv")
    if block_tables.dim() != 2 or block_tables.shape[0] < B:
        raise ValueError(
            f"paged_verify: block_tables {tuple(block_tables.shape)} has "
            f"fewer rows than the {B} sequences")
    for name, t in (("block_tables", block_tables), ("seq_lens", seq_lens),
                    ("q_lens", q_lens)):
        if t.dtype != torch.int32:
            raise TypeError(f"paged_verify: {name} must be int32, got "
                            f"{t.dtype}")
    if seq_lens.dim() != 1 or q_lens.dim() != 1 or \
            seq_lens.shape[0] < B or q_lens.shape[0] < B:
        raise ValueError("paged_verify: seq_lens and q_lens must be [B]")


def paged_verify_ref(q, k_cache, v_cache, block_tables, seq_lens, q_lens,
                     scale=None):
    """fp32 reference for paged_verify (and its CPU path):
    paged_prefill_ref on each sequence's real rows with
    ctx = seq_lens[b] - q_lens[b]; zeros in the padding rows. A sequence
    with q_lens[b] == 0 reads nothing, not even its table row."""
    if k_cache.dtype == torch.uint8:
        raise NotImplementedError(
            "paged_verify: fp8 KV caches are not supported")
    _check_verify_shapes(q, k_cache, block_tables, seq_lens, q_lens)
    out = torch.zeros_like(q)
    for b in range(q.shape[0]):
        n, s = int(q_lens[b]), int(seq_lens[b])
        if n <= 0:
            continue
        out[b, :n] = paged_prefill_ref(q[b, :n], k_cache, v_cache,
                                       block_tables[b], s - n, scale)
    return out


def verify_auto_nsplit(B: int, hkv: int, rows: int, max_blocks: int) -> int:
    """Key split for paged_verify from host-known sizes only: aim at ~512
    workgroups (the MFMA decode kernel's knee), at least 8 cache blocks
    (128 keys) per split of the widest possible sequence, at most 16."""
    tiles = (rows + 31) // 32 if rows > 16 else 1
    base = max(1, B * hkv * tiles)
    return max(1, min(16, 512 // base, (max_blocks + 7) // 8))


def paged_verify(q, k_cache, v_cache, block_tables, seq_lens, q_lens,
                 scale: float | None = None, nsplit: int | None = None):
    """Multi-query decode attention over the paged cache: the attention of
    a speculative verify step.

    q [B, T, Hq, Dh] bf16, 1 <= T <= 8. Sequence b has ``seq_lens[b]`` keys
    in the cache (its new ones included; they are appended before the call)
    and ``q_lens[b]`` (0..T) real query rows: row t < q_lens[b] is the query
    at position seq_lens[b] - q_lens[b] + t and attends to keys up to that
    position. Rows t >= q_lens[b] are padding: they read nothing and are
    returned as zeros; with q_lens[b] == 0 nothing of table row b is read.
    block_tables, seq_lens and q_lens are int32 device tensors and are only
    read on the device, so the launch can sit in a captured graph; ``nsplit``
    (flash-decoding key split) is fixed per launch and defaults to a value
    picked from B, Hkv and the table width. GPU: the gfx950 kernel
    (csrc/attention_verify.hip), bf16 caches in either alloc_kv_cache
    layout, Dh 64/128; fp8 caches and Dh 256 raise. CPU: fp32 reference.
    """
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if _backend.use_hip(q):
        if k_cache.dtype == torch.uint8:
            raise NotImplementedError(
                "paged_verify: fp8 KV caches are not supported")
        if q.shape[-1] not in (64, 128):
            raise NotImplementedError(
                f"paged_verify: head_dim must be 64 or 128 on the GPU, got "
                f"{q.shape[-1]}")
        _check_verify_shapes(q, k_cache, block_tables, seq_lens, q_lens)
        if nsplit is None:
            hkv = k_cache.shape[1]
            nsplit = verify_auto_nsplit(
                q.shape[0], hkv, (q.shape[2] // hkv) * q.shape[1],
                block_tables.shape[1])
        return _backend.ext().paged_verify(
            q.contiguous(), k_cache, v_cache, block_tables, seq_lens, q_lens,
            int(nsplit), float(scale))
    return paged_verify_ref(q, k_cache, v_cache, block_tables, seq_lens,
                            q_lens, scale)


def _is_vt(k_cache, v_cache) -> bool:
    """Transposed-V cache layout (alloc_kv_cache v_transposed) == the
    MFMA decode path; the shape is the routing signal. fp8 vt blocks
    are [dh+4, bs] bytes (scale tail)."""
    if v_cache.dim() != 4:
        return False
    bs = k_cache.shape[2]
    if k_cache.dtype == torch.uint8:
        dh = k_cache.shape[3] - 16
        return v_cache.shape[2] == dh + 4 and v_cache.shape[3] == bs
    return (v_cache.shape[2] == k_cache.shape[3]
            and v_cache.shape[3] == bs and k_cache.shape[3] != bs)


def _auto_nsplit(B, hkv, seq_lens, mfma=False):
    """Work-split (measured sweeps: profiles/decode_attn_pipeline.md).
    The MFMA path is block-granular and latency-light: ~512 WGs is the
    knee. The scalar kernels want ~1024 (4 WGs/CU). Chunks should still
    cover >= ~64 tokens each."""
    base = max(1, B * hkv)
    target = 512 if mfma else 1024
    if base >= target:
        return 1
    max_len = int(seq_lens.max())
    return max(1, min(16, target // base, (max_len + 63) // 64))


def paged_decode(q, k_cache, v_cache, block_tables, seq_lens,
                 scale: float | None = None, nsplit: int | None = None,
                 seq_starts=None):
    """Decode attention over the paged cache. q [B, Hq, Dh] bf16.
    seq_starts (int32 [B], optional): strict-window start positions."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if _backend.use_hip(q):
        if nsplit is None:
            nsplit = _auto_nsplit(q.shape[0], k_cache.shape[1], seq_lens,
                                  mfma=_is_vt(k_cache, v_cache))
        return _backend.ext().paged_decode(
            q.contiguous(), k_cache, v_cache, block_tables, seq_lens,
            int(nsplit), float(scale), seq_starts=seq_starts,
        )
    return paged_decode_ref(q, k_cache, v_cache, block_tables, seq_lens,
                            scale, seq_starts=seq_starts)


def paged_decode_with_operand(q, k_cache, v_cache, block_tables, seq_lens,
                              scale: float | None = None,
                              nsplit: int | None = None, seq_starts=None):
    """paged_decode that ALSO returns the decode-GEMM operand layout of
    the attention output (the o_proj input swizzle fused into the
    epilogue) when the kernel emits it; (out, swz_or_None)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if _backend.use_hip(q):
        if nsplit is None:
            nsplit = _auto_nsplit(q.shape[0], k_cache.shape[1], seq_lens,
                                  mfma=_is_vt(k_cache, v_cache))
        res = _backend.ext().paged_decode_swz(
            q.contiguous(), k_cache, v_cache, block_tables, seq_lens,
            int(nsplit), float(scale), seq_starts=seq_starts)
        return res[0], (res[1] if len(res) > 1 else None)
    return paged_decode_ref(q, k_cache, v_cache, block_tables, seq_lens,
                            scale, seq_starts=seq_starts), None
