"""hipGraph-captured decode step.

The decode inner loop is launch-bound: ~8 small kernels x num_layers per
step plus five host->device tensor builds. This wraps the whole
model.decode(...) call in a hipGraph (torch.cuda.CUDAGraph is hipGraph on
ROCm) per batch-size bucket: static device input buffers are filled from
pinned staging with async copies, then one graph replay launches the
whole step (graph-replay floor ~10-16 us vs ~3.5 us/launch eager,
MI355X_MICROARCH.md price list).

Batch sizes are bucketed to powers of two; short batches pad with a
dummy sequence that reads/writes a reserved KV block, so replay shapes
stay fixed while requests come and go.
"""
from __future__ import annotations

import torch


def fixed_nsplit(batch: int, hkv: int, mfma: bool = False) -> int:
    """Work-split for the paged-decode kernel, chosen per bucket at capture
    time (the eager heuristic in ops/attention.py reads seq_lens.max() —
    a host sync, impossible inside a graph). base = batch*hkv workgroups
    per split; split until ~4x256 CUs are covered — the head-split GQA
    kernels run 4-5 waves/SIMD, so ~4 WGs/CU (1024 WGs) fills the
    machine (measured sweep: llama2-70b B=32 len-2048 1.75 vs 0.67
    TB/s, falcon MQA 0.72 vs 0.23, B=8 0.99-1.24 vs 0.16 —
    profiles/decode_attn_pipeline.md)."""
    base = max(1, batch * hkv)
    # MFMA path (transposed-V caches): per-wave work is block-granular
    # and latency-light — ~512 WGs is the knee (measured: llama2-70b
    # B=32 len-2048 best at nsplit 2, B=8 at 4-8); the scalar kernels
    # want ~1024.
    target = 512 if mfma else 1024
    if base >= target:
        return 1
    return min(16, max(1, target // base))


class GraphedDecoder:
    def __init__(self, model, caches, max_batch: int, max_blocks: int,
                 dummy_block: int, device):
        self.model = model
        self.caches = caches
        self.device = device
        self.max_blocks = max_blocks
        self.dummy_block = dummy_block
        self.buckets = []
        b = 1
        while b < max_batch:
            self.buckets.append(b)
            b *= 2
        self.buckets.append(max_batch)

        B = max_batch
        dev = device
        self.tokens = torch.zeros(B, dtype=torch.long, device=dev)
        self.positions = torch.zeros(B, dtype=torch.int32, device=dev)
        self.slots = torch.full((B,), dummy_block * _bs(), dtype=torch.int32,
                                device=dev)
        self.block_tables = torch.full((B, max_blocks), dummy_block,
                                       dtype=torch.int32, device=dev)
        self.seq_lens = torch.ones(B, dtype=torch.int32, device=dev)
        self.seq_starts = torch.zeros(B, dtype=torch.int32, device=dev)
        pin = dict(dtype=torch.int64,
                   pin_memory=torch.cuda.is_available())
        self.h_staging = torch.zeros(B * 5 + B * max_blocks, **pin)
        self._np = self.h_staging.numpy()
        self.graphs = {}     # bucket -> (CUDAGraph, logits_out)
        self._pool = None
        self.lora_pool = None   # serve/lora.py AdapterPool (enable_lora)
        self.verify_T = None    # rows per sequence of the verify family

    def enable_lora(self, pool) -> None:
        """Second graph family, keyed (bucket, "lora"), for batches in
        which a row has an adapter: the same decode captured with
        ``lora=`` over one more static buffer, ``adapter_idx`` (-1 = no
        adapter, padding rows included), filled from its own pinned
        staging tensor. The adapter-free family and ``h_staging`` are
        untouched."""
        B = self.tokens.shape[0]
        self.lora_pool = pool
        self.adapter_idx = torch.full((B,), -1, dtype=torch.int32,
                                      device=self.device)
        self.h_adapter = torch.full((B,), -1, dtype=torch.int32,
                                    pin_memory=torch.cuda.is_available())
        self._np_adapter = self.h_adapter.numpy()

    def enable_verify(self, T: int, vocab_size: int | None = None) -> None:
        """Third graph family, keyed (bucket, "verify"): the speculative
        verify forward (Transformer.verify) at a fixed T rows per sequence
        and a fixed key split. Static buffers of its own hold tokens,
        positions and slots [B, T], seq_lens and q_lens [B]; the block
        tables are the decode family's buffer. Filled from a pinned staging
        tensor of its own; the other families are untouched."""
        B = self.tokens.shape[0]
        dev = self.device
        self.verify_T = int(T)
        # staged token ids are checked against it (the model's, unless given)
        self.vocab_size = int(vocab_size if vocab_size is not None
                              else self.model.cfg.vocab_size)
        self.v_tokens = torch.zeros(B, T, dtype=torch.long, device=dev)
        self.v_positions = torch.zeros(B, T, dtype=torch.int32, device=dev)
        self.v_slots = torch.full((B, T), self.dummy_block * _bs(),
                                  dtype=torch.int32, device=dev)
        self.v_seq_lens = torch.zeros(B, dtype=torch.int32, device=dev)
        self.v_q_lens = torch.zeros(B, dtype=torch.int32, device=dev)
        self.h_verify = torch.zeros(
            B * (3 * T + 2) + B * self.max_blocks, dtype=torch.int64,
            pin_memory=torch.cuda.is_available())
        self._np_verify = self.h_verify.numpy()

    def _verify_nsplit(self, b: int) -> int:
        from ..ops.attention import verify_auto_nsplit
        attn = self.model.blocks[0].attn
        return verify_auto_nsplit(b, attn.hkv,
                                  (attn.hq // attn.hkv) * self.verify_T,
                                  self.max_blocks)

    def _capture_verify(self, b: int):
        args = (self.v_tokens[:b], self.v_positions[:b], self.caches,
                self.v_slots[:b], self.block_tables[:b],
                self.v_seq_lens[:b], self.v_q_lens[:b])
        kw = dict(nsplit=self._verify_nsplit(b))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self.model.verify(*args, **kw)
        torch.cuda.current_stream().wait_stream(s)

        g = torch.cuda.CUDAGraph()
        if self._pool is None:
            with torch.cuda.graph(g):
                out = self.model.verify(*args, **kw)
            self._pool = g.pool()
        else:
            with torch.cuda.graph(g, pool=self._pool):
                out = self.model.verify(*args, **kw)
        self.graphs[(b, "verify")] = (g, out)

    def verify(self, token_rows, pos_rows, slot_rows, block_rows, seq_lens):
        """Replay the verify family. Host lists: sequence i brings
        len(token_rows[i]) (1..T) real rows with their positions and slots,
        its block list and its key count. Returns logits [n * T, V] (a view
        into the static output), row i * T + j for row j of sequence i."""
        n = len(token_rows)
        b = next(x for x in self.buckets if x >= n)
        self._stage_verify(b, token_rows, pos_rows, slot_rows, block_rows,
                           seq_lens)
        if (b, "verify") not in self.graphs:
            self._capture_verify(b)
        g, out = self.graphs[(b, "verify")]
        T, mb, h = self.verify_T, self.max_blocks, self.h_verify
        bT = b * T
        self.v_tokens[:b].copy_(h[0:bT].view(b, T), non_blocking=True)
        self.v_positions[:b].copy_(h[bT:2 * bT].view(b, T),
                                   non_blocking=True)
        self.v_slots[:b].copy_(h[2 * bT:3 * bT].view(b, T),
                               non_blocking=True)
        o = 3 * bT
        self.v_seq_lens[:b].copy_(h[o:o + b], non_blocking=True)
        self.v_q_lens[:b].copy_(h[o + b:o + 2 * b], non_blocking=True)
        self.block_tables[:b].copy_(
            h[o + 2 * b:o + 2 * b + b * mb].view(b, mb), non_blocking=True)
        g.replay()
        return out[:n * T]

    def _stage_verify(self, b, token_rows, pos_rows, slot_rows, block_rows,
                      seq_lens) -> None:
        """Range-check the step's lengths, token ids, slots and block ids on
        the host (the kernels only index with them) and fill the pinned staging
        buffer for bucket b. Padding rows of a sequence repeat its last
        position, carry token 0 and write to the dummy block; sequences
        beyond n have q_len 0 and are not read at all. CPU-testable."""
        n = len(token_rows)
        T, mb, bs = self.verify_T, self.max_blocks, _bs()
        nblk = self.caches[0][0].shape[0]
        hn = self._np_verify
        bT = b * T
        tok = hn[0:bT].reshape(b, T)
        pos = hn[bT:2 * bT].reshape(b, T)
        slt = hn[2 * bT:3 * bT].reshape(b, T)
        o = 3 * bT
        sl = hn[o:o + b]
        ql = hn[o + b:o + 2 * b]
        btn = hn[o + 2 * b:o + 2 * b + b * mb].reshape(b, mb)
        for i in range(n):
            q = len(token_rows[i])
            s = int(seq_lens[i])
            row = block_rows[i]
            if not (1 <= q <= T and len(pos_rows[i]) == q
                    and len(slot_rows[i]) == q):
                raise ValueError(f"verify row {i}: {q} query rows, the graph "
                                 f"holds 1..{T}")
            if not (q <= s <= len(row) * bs and len(row) <= mb):
                raise ValueError(f"verify row {i}: seq_len {s} with {q} rows "
                                 f"and {len(row)} blocks (table width {mb})")
            V = self.vocab_size
            if any(not 0 <= x < V for x in token_rows[i]):
                raise ValueError(f"verify row {i}: token id outside the "
                                 f"vocabulary of {V}")
            if any(not 0 <= x < nblk for x in row) or \
                    any(not 0 <= x < nblk * bs for x in slot_rows[i]):
                raise ValueError(f"verify row {i}: block id or slot out of "
                                 f"the pool of {nblk} blocks")
        tok.fill(0)
        pos.fill(0)
        slt.fill(self.dummy_block * bs)
        sl.fill(0)
        ql.fill(0)
        btn.fill(self.dummy_block)
        for i in range(n):
            q = len(token_rows[i])
            tok[i, :q] = token_rows[i]
            pos[i, :q] = pos_rows[i]
            pos[i, q:] = pos_rows[i][-1]
            slt[i, :q] = slot_rows[i]
            sl[i] = seq_lens[i]
            ql[i] = q
            btn[i, :len(block_rows[i])] = block_rows[i]

    # -- capture -----------------------------------------------------------
    def _capture(self, b: int, lora: bool = False):
        hkv = self.model.local_kv_heads()
        from ..ops.attention import _is_vt
        nsplit = fixed_nsplit(b, hkv,
                              mfma=_is_vt(*self.caches[0][:2]))
        args = (self.tokens[:b], self.positions[:b], self.caches,
                self.slots[:b], self.block_tables[:b], self.seq_lens[:b])
        kw = dict(nsplit=nsplit, seq_starts=self.seq_starts[:b])
        if lora:
            from .lora import LoraBatch
            kw["lora"] = LoraBatch(self.lora_pool, idx=self.adapter_idx[:b])
        # warmup outside the graph (allocator + autotune settle)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self.model.decode(*args, **kw)
        torch.cuda.current_stream().wait_stream(s)

        g = torch.cuda.CUDAGraph()
        if self._pool is None:
            with torch.cuda.graph(g):
                out = self.model.decode(*args, **kw)
            self._pool = g.pool()
        else:
            with torch.cuda.graph(g, pool=self._pool):
                out = self.model.decode(*args, **kw)
        self.graphs[(b, "lora") if lora else b] = (g, out)

    # -- replay ------------------------------------------------------------
    def decode(self, tokens, positions, slots, block_rows, seq_lens,
               seq_starts=None, adapter_slots=None):
        """All args host lists; block_rows is a list of per-seq block lists.
        Returns logits [len(tokens), V] (a view into the static output).
        ``adapter_slots`` (one adapter slot per row, -1 = none; needs
        enable_lora) replays the "lora" graph family."""
        n = len(tokens)
        b = next(x for x in self.buckets if x >= n)
        key = b if adapter_slots is None else (b, "lora")
        if adapter_slots is not None:
            self._stage_adapters(b, adapter_slots)
        if key not in self.graphs:
            self._capture(b, lora=adapter_slots is not None)
        g, out = self.graphs[key]
        bt = self._stage(b, tokens, positions, slots, block_rows, seq_lens,
                         seq_starts or [0] * n)

        h = self.h_staging
        self.tokens[:b].copy_(h[0:b], non_blocking=True)
        self.positions[:b].copy_(h[b:2 * b], non_blocking=True)
        self.slots[:b].copy_(h[2 * b:3 * b], non_blocking=True)
        self.seq_lens[:b].copy_(h[3 * b:4 * b], non_blocking=True)
        self.seq_starts[:b].copy_(h[4 * b:5 * b], non_blocking=True)
        self.block_tables[:b].copy_(bt, non_blocking=True)
        if adapter_slots is not None:
            self.adapter_idx[:b].copy_(self.h_adapter[:b], non_blocking=True)
        g.replay()
        return out[:n]

    def _stage_adapters(self, b, adapter_slots) -> None:
        """Range-check the rows' adapter slots on the host (the kernels
        only index with them) and stage them; padding rows get -1."""
        if self.lora_pool is None:
            raise RuntimeError("adapter_slots given before enable_lora()")
        n = len(adapter_slots)
        top = self.lora_pool.max_loras
        for i, s in enumerate(adapter_slots):
            if not -1 <= s < top:
                raise ValueError(f"adapter slot {s} of row {i} is out of "
                                 f"range (-1..{top - 1})")
        self._np_adapter[:n] = adapter_slots
        self._np_adapter[n:b] = -1

    def _stage(self, b, tokens, positions, slots, block_rows, seq_lens,
               seq_starts):
        """Fill the pinned staging buffer for bucket size b (numpy view:
        C-speed fills instead of one small torch.tensor per row). Unit-
        tested on CPU (the rest of this class needs a GPU)."""
        n = len(tokens)
        mb = self.max_blocks
        hn = self._np
        hn[0:n] = tokens
        hn[b:b + n] = positions
        hn[2 * b:2 * b + n] = slots
        hn[3 * b:3 * b + n] = seq_lens
        hn[4 * b:4 * b + n] = seq_starts
        btn = hn[5 * b:5 * b + b * mb].reshape(b, mb)
        btn.fill(self.dummy_block)
        for i, row in enumerate(block_rows):
            btn[i, :len(row)] = row
        # pad rows beyond n: dummy sequence at position 0, length 1
        if n < b:
            hn[n:b] = 0
            hn[b + n:2 * b] = 0
            hn[2 * b + n:3 * b] = self.dummy_block * _bs()
            hn[3 * b + n:4 * b] = 1
            hn[4 * b + n:5 * b] = 0
        return self.h_staging[5 * b:5 * b + b * mb].view(b, mb)


def _bs() -> int:
    from .. import ops
    return ops.BLOCK_SIZE
