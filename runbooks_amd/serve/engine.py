"""Serving engine: paged KV cache + continuous batching.

Native replacement for the reference's external basaran server image
(SURVEY.md §2b "server image"): greedy/temperature decode over a paged
KV cache, sized for the MI355X's 288 GB HBM3E (the cache pool is
allocated from measured free memory, not a guess), TP across up to 8
GPUs over xGMI.

Scheduling: one prefill (whole prompt in one pass) is admitted per step
when capacity allows, then all running sequences decode as one batch —
decode batches hit the gfx950 paged-decode kernel
(ops/csrc/attention_decode.hip).

Two opt-in knobs prefill FROM the paged cache instead
(ops/csrc/attention_prefill_paged.hip): ``prefill_from_cache`` runs only
the uncached tail of a prompt on a prefix-cache hit, and
``prefill_chunk`` feeds a long prompt through the model at most that
many tokens per step, so running sequences keep decoding in between.
A third, ``prefill_batch`` = N > 1, admits up to N waiting requests per
step and runs their (uncached) prompt tokens packed into ONE model
forward (``Transformer.prefill_paged_batch``, the varlen kernel in the
same file) instead of one forward each: a burst of short tails behind a
shared system prompt streams the weights once. A request that would hit
on a prefix another member of the same batch is about to publish waits
one step and hits; a prompt longer than ``prefill_chunk`` still takes the
chunked path alone.

Sliding-window attention (mistral, cfg.sliding_window): enforced here as
pure KV bookkeeping — RoPE is applied at absolute positions when keys
are written, so attention over any suffix of the cache is exact, and the
kernel needs no window parameter. Whole front blocks that fall entirely
outside the window are freed (bounded cache memory per sequence) and
the block table / seq_len presented to the kernel cover only the
retained suffix. Granularity is BLOCK_SIZE: a query attends to between
W and W+BLOCK_SIZE-1 trailing tokens; prompts longer than W prefill
with full causal attention (exact for prompts <= W, which covers the
supported max prompt for mistral-7b).
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import torch

from .. import ops
from ..models import Transformer, build_model
from ..parallel import comm
from ..utils.trace import get_tracer


class BlockAllocator:
    """Free-list allocator with reference counts: prefix-cached blocks
    are shared across requests (and held by the cache itself); a block
    returns to the free list when its last reference is released."""

    def __init__(self, num_blocks: int):
        self.free = list(range(num_blocks - 1, -1, -1))
        self.num_blocks = num_blocks
        self.refs = [0] * num_blocks

    def alloc(self, n: int) -> list[int]:
        if n > len(self.free):
            raise RuntimeError("KV cache exhausted")
        out = [self.free.pop() for _ in range(n)]
        for b in out:
            self.refs[b] = 1
        return out

    def share(self, block: int) -> None:
        assert self.refs[block] > 0, "sharing a free block"
        self.refs[block] += 1

    def release(self, blocks: list[int]):
        for b in blocks:
            self.refs[b] -= 1
            assert self.refs[b] >= 0, "double release"
            if self.refs[b] == 0:
                self.free.append(b)


@dataclass
class Request:
    request_id: int
    prompt_ids: list[int]
    max_new_tokens: int = 64
    temperature: float = 0.0
    top_p: float = 1.0
    logprobs: int | None = None     # record top-k logprobs per token
    seed: int | None = None         # per-request sampling seed override
    presence_penalty: float = 0.0   # subtract once per seen token
    frequency_penalty: float = 0.0  # subtract per occurrence
    repetition_penalty: float = 1.0  # HF-style multiplicative penalty
    stop_ids: tuple[int, ...] = ()
    top_k: int = 0                  # keep the k most likely tokens (0 = off)
    min_p: float = 0.0              # keep p >= min_p * p_max (0 = off)
    # state
    output_ids: list[int] = field(default_factory=list)
    # per output token, when logprobs is set: {"logprob": f, "top": [(id, f)]}
    logprob_data: list = field(default_factory=list)
    blocks: list[int] = field(default_factory=list)
    # tokens whose KV blocks were freed by the sliding window (always a
    # multiple of BLOCK_SIZE; blocks[] maps retained positions only)
    dropped: int = 0
    # prompt tokens whose KV is in the cache (prefix hit + chunks done so
    # far) while the request is prefilling
    computed: int = 0
    finished: bool = False
    created: float = field(default_factory=time.time)
    # name of the LoRA adapter this request is served with (None = base)
    adapter: str | None = None

    @property
    def seq_len(self) -> int:
        return len(self.prompt_ids) + len(self.output_ids)


class Engine:
    def __init__(self, model: Transformer | str, device=None,
                 dtype=torch.bfloat16, kv_blocks: int | None = None,
                 max_batch: int = 64, mem_fraction: float = 0.85, seed: int = 0,
                 load_in_8bit: bool = False, prefix_cache: bool | None = None,
                 kv_fp8: bool | None = None, load_in_4bit: bool = False,
                 prefill_from_cache: bool | None = None,
                 prefill_chunk: int | None = None,
                 prefill_batch: int | None = None,
                 w4_resident: bool | None = None,
                 batch_sampler: bool | None = None,
                 max_loras: int | None = None,
                 lora_rank: int | None = None,
                 speculative: int | None = None,
                 spec_ngram: int | None = None,
                 drafter=None):
        self.device = device if device is not None else (
            f"cuda:{comm.local_rank()}" if torch.cuda.is_available() else "cpu")
        if isinstance(model, str):
            model = build_model(model, dtype=dtype, seed=seed,
                                device=self.device)
        self.model = model.to(self.device).eval()
        if load_in_4bit and load_in_8bit:
            print("engine: MODEL_LOAD_IN_4BIT and MODEL_LOAD_IN_8BIT both "
                  "set; serving 4-bit", flush=True)
            load_in_8bit = False
        # Int4-resident serving (RB_W4_RESIDENT=1 or w4_resident=True, with
        # load_in_4bit): the bf16 masters of the int4-quantized weights
        # are freed right after quantization, BEFORE the KV pool is sized
        # below, so the freed bytes become KV blocks; prefill then runs
        # the int4 GEMM (ops/csrc/gemm_w4.hip) on the weights decode
        # streams.
        import os as _os1
        if w4_resident is None:
            w4_resident = _os1.environ.get("RB_W4_RESIDENT", "0") == "1"
        if w4_resident and not (torch.cuda.is_available() and load_in_4bit
                                and model.tp == 1):
            print("engine: w4_resident ignored "
                  + ("without a GPU" if not torch.cuda.is_available()
                     else "at TP>1" if model.tp > 1
                     else "without load_in_4bit")
                  + " (the bf16 master weights stay)", flush=True)
            w4_resident = False
        self.w4_resident = bool(w4_resident)
        if torch.cuda.is_available():
            # TP>1 included: each rank fuses ITS OWN qkv / gate-up weight
            # shards and registers decode-GEMM layouts for them — the
            # collective order (o/down all-reduce per layer) is untouched,
            # so the worker-follow protocol stays aligned.
            from ..models.transformer import fuse_for_inference
            fuse_for_inference(self.model,
                               load_in_8bit=load_in_8bit and model.tp == 1,
                               load_in_4bit=load_in_4bit and model.tp == 1,
                               w4_resident=self.w4_resident)
        if load_in_4bit and model.tp > 1:
            print("engine: MODEL_LOAD_IN_4BIT ignored at TP>1 "
                  "(int4 decode path is single-GPU, like the fp8 one)",
                  flush=True)
        if load_in_8bit and model.tp > 1:
            print("engine: MODEL_LOAD_IN_8BIT ignored at TP>1 "
                  "(fp8 decode path is single-GPU; 288 GB/GPU rarely "
                  "needs 8-bit at TP>1)", flush=True)
        # LoRA adapter serving (off by default): RB_MAX_LORAS=N /
        # max_loras=N > 0 preallocates N adapter slots of rank
        # RB_LORA_RANK / lora_rank (serve/lora.py) before the KV pool is
        # sized; requests then pick an adapter by name and a decode batch
        # may mix them. With 0 nothing is allocated and every path below
        # is the adapter-free one.
        self.max_loras = int(max_loras if max_loras is not None
                             else _os1.environ.get("RB_MAX_LORAS", "0") or 0)
        self.lora_rank = int(lora_rank if lora_rank is not None
                             else _os1.environ.get("RB_LORA_RANK", "16")
                             or 16)
        self.lora_pool = None
        if self.max_loras < 0:
            raise ValueError(f"max_loras must be >= 0, got {self.max_loras}")
        if self.max_loras > 0:
            if comm.world_size() > 1 or model.tp > 1:
                raise NotImplementedError(
                    "max_loras > 0: adapter serving is single-GPU (TP=1)")
            from .lora import AdapterPool
            if not torch.cuda.is_available():
                # the CPU reference path serves adapters through the same
                # fused qkv / gate-up sites
                from ..models.transformer import fuse_for_inference
                if getattr(self.model.blocks[0].attn, "_qkv_w", None) is None:
                    fuse_for_inference(self.model)
            self.lora_pool = AdapterPool(self.model, self.max_loras,
                                         self.lora_rank)
        self.cfg = model.cfg
        if torch.cuda.is_available() and model.cfg.head_dim not in (64, 128,
                                                                    256):
            raise NotImplementedError(
                f"paged decode supports head_dim 64/128/256 on gfx950; "
                f"{model.cfg.name} has {model.cfg.head_dim}")
        self.bs = ops.BLOCK_SIZE
        self.max_batch = max_batch
        # Admission budget per step: the default 1 matches the classic
        # one-prefill-then-decode cadence (decode latency bounded); the
        # HTTP server raises it for bursty arrival patterns where
        # admission throughput dominates (scripts/bench_http.py).
        self.max_prefills_per_step = 1
        self.seed = seed
        # fp8-e4m3 KV cache (RB_KV_FP8=1 or kv_fp8=True): halves the
        # decode-attention read stream and doubles KV capacity — the
        # long-context lever for the 288 GB/GPU KV story (BASELINE #5).
        import os as _os0
        self.kv_fp8 = (kv_fp8 if kv_fp8 is not None
                       else _os0.environ.get("RB_KV_FP8", "0") == "1")
        if self.kv_fp8 and self.lora_pool is not None:
            raise NotImplementedError(
                "max_loras > 0 with an fp8 KV cache (RB_KV_FP8) is not "
                "supported: adapter batches are validated on the bf16 "
                "cache only; serve adapters with kv_fp8 off")
        if kv_blocks is None:
            kv_blocks = self._auto_kv_blocks(mem_fraction)
        if comm.is_dist() and comm.world_size() > 1 and model.tp > 1:
            # Every rank must agree on the pool size: rank 0's scheduler
            # hands out slot indices that worker ranks index their OWN
            # caches with — a rank with less free memory would otherwise
            # read/write out of bounds. Take the fleet minimum.
            t = torch.tensor([kv_blocks], dtype=torch.int64,
                             device=self.device if
                             torch.cuda.is_available() else "cpu")
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MIN)
            kv_blocks = int(t.item())
        # last block is reserved as the dummy block hipGraph-padded decode
        # rows read/write (serve/graph.py)
        self.allocator = BlockAllocator(kv_blocks - 1)
        self.caches = self.model.alloc_caches(kv_blocks, self.device,
                                              fp8=self.kv_fp8)
        self.dummy_block = kv_blocks - 1
        self.waiting: list[Request] = []
        self.running: list[Request] = []
        # the one request whose prompt is part-way through a chunked
        # prefill: holds its blocks, is in neither waiting nor running
        self.prefilling: Request | None = None
        self._next_id = 0
        # sliding window bounds per-seq blocks at W//bs + 2 (retained
        # suffix <= W + bs tokens incl. the one being appended); prompts
        # prefill in full but front blocks are dropped before the first
        # decode, so this is the true block-table width for decode.
        seq_cap = self.cfg.max_seq_len
        if self.cfg.sliding_window:
            seq_cap = min(seq_cap, self.cfg.sliding_window + 2 * self.bs)
        # +1: _admit allocates ceil(S/bs)+1 blocks (prompt + headroom for
        # the first decoded token), so a near-max-length prompt can hold
        # ceil(seq_cap/bs)+1 blocks — the graph staging table must be at
        # least that wide or btn[i, :len(row)] raises mid-flight.
        self.max_blocks_per_seq = min(
            kv_blocks, (seq_cap + self.bs - 1) // self.bs + 1)
        self._graphed = None
        # hipGraphs drive the single-GPU decode; the TP>1 path runs eager
        # so the worker-follow protocol (serve/tp_worker.py) sees every
        # collective.
        self.tp = comm.world_size()
        self.use_graphs = torch.cuda.is_available() and self.tp == 1
        # Prefix caching (RB_PREFIX_CACHE=0 or prefix_cache=False turns it
        # off): full 16-token prompt-prefix chunks are shared across
        # requests by refcount, which bounds cache memory for
        # common-system-prompt serving. By default a hit only skips the KV
        # writes for those chunks and the prefill still computes the full
        # prompt; with prefill_from_cache the hit chunks are not computed
        # at all — the rest of the prompt attends over them in the cache.
        import os as _os
        # default-on since the GPU validation pass (r2: shared-prompt
        # decode parity vs an uncached engine); RB_PREFIX_CACHE=0 disables
        self.prefix_cache_enabled = (
            prefix_cache if prefix_cache is not None
            else _os.environ.get("RB_PREFIX_CACHE", "1") == "1")
        from collections import OrderedDict
        self._pc: "OrderedDict[tuple, int]" = OrderedDict()
        # Prefill from the paged cache (both off by default):
        # RB_PREFILL_FROM_CACHE=1 / prefill_from_cache=True skips the
        # cached prefix of a prompt; RB_PREFILL_CHUNK=N / prefill_chunk=N
        # (a multiple of the block size, 0 = off) bounds the prompt tokens
        # run per step.
        self.prefill_from_cache = (
            prefill_from_cache if prefill_from_cache is not None
            else _os.environ.get("RB_PREFILL_FROM_CACHE", "0") == "1")
        self.prefill_chunk = int(
            prefill_chunk if prefill_chunk is not None
            else _os.environ.get("RB_PREFILL_CHUNK", "0") or 0)
        if self.prefill_chunk < 0 or self.prefill_chunk % self.bs:
            raise ValueError(
                f"prefill_chunk must be a multiple of {self.bs}, got "
                f"{self.prefill_chunk}")
        if (self.prefill_from_cache or self.prefill_chunk) and \
                (self.tp > 1 or self.kv_fp8):
            print("engine: prefill_from_cache / prefill_chunk ignored "
                  + ("at TP>1" if self.tp > 1 else "with an fp8 KV cache")
                  + " (paged prefill is single-GPU bf16; whole-prompt "
                  "prefill is used)", flush=True)
            self.prefill_from_cache = False
            self.prefill_chunk = 0
        # Batched prefill (off by default): RB_PREFILL_BATCH=N /
        # prefill_batch=N > 1 packs up to N admissions of a step into one
        # model forward; prefill_chunk, when set, is also that forward's
        # token budget. 0 or 1 = one forward per request.
        self.prefill_batch = int(
            prefill_batch if prefill_batch is not None
            else _os.environ.get("RB_PREFILL_BATCH", "0") or 0)
        if self.prefill_batch < 0:
            raise ValueError(
                f"prefill_batch must be >= 0, got {self.prefill_batch}")
        if self.prefill_batch > 1 and (self.tp > 1 or self.kv_fp8):
            print("engine: prefill_batch ignored "
                  + ("at TP>1" if self.tp > 1 else "with an fp8 KV cache")
                  + " (paged prefill is single-GPU bf16; one prefill per "
                  "request is used)", flush=True)
            self.prefill_batch = 0
        # Batched sampler (off by default): RB_BATCH_SAMPLER=1 /
        # batch_sampler=True samples every batch, whatever mix of
        # per-request parameters it holds, with one ops.sample_batch call
        # and one download (ops/csrc/sample_batch.hip). A batch in which a
        # request sets top_k or min_p takes that path whatever the knob
        # says: the older path has no such filters.
        self.batch_sampler = (
            batch_sampler if batch_sampler is not None
            else _os.environ.get("RB_BATCH_SAMPLER", "0") == "1")
        # request_id -> {token id: count} over prompt + output, kept up to
        # date one token at a time for the batched sampler's penalty CSR
        self._tok_counts: dict[int, dict] = {}
        self.stats = {"steps": 0, "prefills": 0, "decode_tokens": 0,
                      "preemptions": 0, "prefix_hits": 0,
                      "prefix_hit_blocks": 0, "window_dropped_blocks": 0,
                      "prefill_tokens": 0, "prefix_skipped_tokens": 0,
                      "prefill_chunks": 0, "prefill_batches": 0,
                      "prefill_batched_requests": 0,
                      "sampler_batched_steps": 0}
        if self.lora_pool is not None:
            self.stats["lora_decode_steps"] = 0
            self.stats["lora_rows"] = 0
        # Speculative decoding (off by default): RB_SPECULATIVE=K /
        # speculative=K in 1..7 drafts up to K tokens per running sequence
        # per step from the request's own text (serve/spec.py NgramDrafter
        # over RB_SPEC_NGRAM / spec_ngram tokens, or ``drafter``) and
        # verifies them in one forward (Transformer.verify,
        # ops/csrc/attention_verify.hip). Every row is sampled with the
        # batched sampler at the seed its position would get without
        # speculation, so the text is that of Engine(batch_sampler=True);
        # the knob therefore also turns the batched sampler on. With 0
        # nothing is allocated and every path is the one above.
        K = int(speculative if speculative is not None
                else _os.environ.get("RB_SPECULATIVE", "0") or 0)
        N = int(spec_ngram if spec_ngram is not None
                else _os.environ.get("RB_SPEC_NGRAM", "3") or 3)
        if not 0 <= K <= ops.attention.VERIFY_MAX_T - 1:
            raise ValueError(f"speculative must be 0.."
                             f"{ops.attention.VERIFY_MAX_T - 1}, got {K}")
        if K > 0:
            why = ("at TP>1" if self.tp > 1 or model.tp > 1
                   else "with an fp8 KV cache" if self.kv_fp8
                   else "for a sliding-window model"
                   if self.cfg.sliding_window
                   else "at head_dim 256" if self.cfg.head_dim not in (64, 128)
                   else None)
            if why is not None:
                print(f"engine: speculative ignored {why} (the verify "
                      "kernel is single-GPU bf16, head_dim 64/128, full "
                      "attention; one token per step is used)", flush=True)
                K = 0
        self.speculative = K
        self.drafter = None
        if K > 0:
            if drafter is None:
                from .spec import NgramDrafter
                drafter = NgramDrafter(N)
            self.drafter = drafter
            self.batch_sampler = True
            self.stats.update(spec_steps=0, spec_drafted=0, spec_accepted=0)

    def _auto_kv_blocks(self, mem_fraction: float) -> int:
        elem = (self.cfg.head_dim + 16) if self.kv_fp8 \
            else self.cfg.head_dim * 2
        bytes_per_block = (2 * self.cfg.num_layers * self.model.local_kv_heads()
                           * self.bs * elem)
        if torch.cuda.is_available():
            free, _total = torch.cuda.mem_get_info(self.device)
            budget = int(free * mem_fraction) - (2 << 30)  # activations headroom
        else:
            budget = 64 << 20
        return max(16, budget // bytes_per_block)

    # -- request API ------------------------------------------------------------
    def submit(self, prompt_ids: list[int], max_new_tokens: int = 64,
               temperature: float = 0.0, top_p: float = 1.0,
               logprobs: int | None = None, seed: int | None = None,
               presence_penalty: float = 0.0,
               frequency_penalty: float = 0.0,
               repetition_penalty: float = 1.0,
               stop_token_ids: tuple[int, ...] = (),
               top_k: int = 0, min_p: float = 0.0,
               adapter: str | None = None) -> Request:
        if adapter is not None and (self.lora_pool is None
                                    or adapter not in self.lora_pool):
            raise KeyError(f"no adapter named {adapter!r} is loaded")
        req = Request(self._next_id, list(prompt_ids), max_new_tokens,
                      temperature, top_p, logprobs, seed,
                      presence_penalty, frequency_penalty,
                      repetition_penalty, tuple(stop_token_ids),
                      int(top_k or 0), float(min_p or 0.0))
        req.adapter = adapter
        self._next_id += 1
        self.waiting.append(req)
        return req

    # -- adapters ---------------------------------------------------------------
    def _need_pool(self):
        if self.lora_pool is None:
            raise RuntimeError("this engine serves no adapters: construct it "
                               "with max_loras > 0 (RB_MAX_LORAS)")
        return self.lora_pool

    def load_adapter(self, name: str, path) -> None:
        """Read a LoRA adapter (trainer checkpoint or HF PEFT directory)
        into a free slot. Copies on the current stream between steps:
        call it from the thread that steps the engine (EngineLoop queues
        it)."""
        self._need_pool().load(name, path)

    def load_adapter_state(self, name: str, state: dict, alpha: float,
                           r: int | None = None) -> None:
        """load_adapter for tensors already in memory (serve/lora.py
        read_adapter); the same threading rule holds."""
        self._need_pool().load_state(name, state, alpha, r)

    def unload_adapter(self, name: str) -> None:
        pool = self._need_pool()
        pool.slot_of(name)          # KeyError for an unknown name
        live = list(self.waiting) + list(self.running)
        if self.prefilling is not None:
            live.append(self.prefilling)
        users = [r.request_id for r in live if r.adapter == name]
        if users:
            raise RuntimeError(f"adapter {name!r} is in use by request(s) "
                               f"{users}; unload it once they finish")
        if self.prefix_cache_enabled:
            # a later adapter of the same name must not hit on this one's
            # K/V
            for key in [k for k in self._pc
                        if k and isinstance(k[0], str) and k[0] == name]:
                self.allocator.release([self._pc.pop(key)])
        pool.unload(name)

    def adapters(self) -> list[str]:
        return [] if self.lora_pool is None else self.lora_pool.loaded()

    def _lora_for(self, reqs: list[Request]):
        """LoraBatch for these rows / sequences, None when none of them
        has an adapter (the adapter-free call is then made unchanged)."""
        if self.lora_pool is None or all(r.adapter is None for r in reqs):
            return None
        from .lora import LoraBatch
        return LoraBatch(self.lora_pool, self._lora_slots(reqs))

    def _lora_slots(self, reqs: list[Request]) -> list[int]:
        pool = self.lora_pool
        return [-1 if r.adapter is None else pool.slot_of(r.adapter)
                for r in reqs]

    def _pc_key(self, req: Request, n_tokens: int) -> tuple:
        """Prefix-cache key of the request's first n_tokens prompt tokens.
        K/V depend on the adapter, so its name leads the key: two adapters
        never share a block, requests of one adapter still do."""
        key = tuple(req.prompt_ids[:n_tokens])
        return key if req.adapter is None else (req.adapter,) + key

    @staticmethod
    def _apply_penalties(row, r: Request):
        """OpenAI presence/frequency penalties over the text so far
        (prompt + generated). Torch ops on the logits row, outside the
        decode hipGraph — zero cost for requests that don't ask."""
        if not (r.presence_penalty or r.frequency_penalty or
                r.repetition_penalty != 1.0):
            return row
        from collections import Counter
        cnt = Counter(r.prompt_ids)
        cnt.update(r.output_ids)
        ids = torch.tensor(list(cnt.keys()), dtype=torch.long,
                           device=row.device)
        c = torch.tensor([float(v) for v in cnt.values()],
                         device=row.device)
        row = row.clone().float()
        row[ids] -= r.frequency_penalty * c + r.presence_penalty
        if r.repetition_penalty != 1.0:
            seen = row[ids]
            row[ids] = torch.where(seen > 0, seen / r.repetition_penalty,
                                   seen * r.repetition_penalty)
        return row

    @staticmethod
    def _record_logprobs(req: Request, logits_row, tok_id: int) -> None:
        """Top-k logprob bookkeeping for one sampled token (host sync;
        only runs for requests that asked — sampling already lives
        outside the hipGraph, so the graphed decode path is untouched)."""
        lp = torch.log_softmax(logits_row.float(), dim=-1)
        entry = {"logprob": float(lp[tok_id])}
        k = req.logprobs or 0
        if k > 0:
            v, idx = lp.topk(min(k, lp.numel()))
            entry["top"] = list(zip(idx.tolist(), v.tolist()))
        req.logprob_data.append(entry)

    def _admit(self) -> Request | None:
        if not self.waiting or len(self.running) >= self.max_batch:
            return None
        if self.prefilling is not None:   # one chunked prefill at a time
            return None
        req = self.waiting[0]
        S = len(req.prompt_ids)
        hits: list[tuple[tuple, int]] = []
        if self.prefix_cache_enabled:
            for k in range(1, S // self.bs + 1):
                key = self._pc_key(req, k * self.bs)
                b = self._pc.get(key)
                if b is None:
                    break
                hits.append((key, b))
        need = (S + self.bs - 1) // self.bs + 1 - len(hits)
        if need > len(self.allocator.free) and self.prefix_cache_enabled:
            self._evict_prefix(need - len(self.allocator.free),
                               protect={b for _, b in hits})
        if need > len(self.allocator.free):
            return None
        self.waiting.pop(0)
        if hits:
            self.stats["prefix_hits"] += 1
            self.stats["prefix_hit_blocks"] += len(hits)
        for key, b in hits:
            self.allocator.share(b)
            self._pc.move_to_end(key)
        req.blocks = [b for _, b in hits] + self.allocator.alloc(need)
        req._shared_chunks = len(hits)
        return req

    def _evict_prefix(self, n_blocks: int, protect: set = frozenset()):
        """Drop LRU prefix-cache entries until ~n_blocks come free (an
        entry only frees its block if no live request still shares it)."""
        for key in list(self._pc):
            if n_blocks <= 0:
                return
            b = self._pc[key]
            if b in protect:
                continue
            if self.prefill_from_cache and self.allocator.refs[b] > 1:
                # still shared by a live request: dropping the entry frees
                # nothing now, and would cost that request's re-prefill
                # its cached history if it is preempted next
                continue
            del self._pc[key]
            before = len(self.allocator.free)
            self.allocator.release([b])
            n_blocks -= len(self.allocator.free) - before

    def _pc_insert(self, req: Request) -> None:
        """After a successful prefill, publish the request's full prompt
        chunks (cache holds its own reference per block)."""
        S = len(req.prompt_ids)
        for k in range(1, S // self.bs + 1):
            key = self._pc_key(req, k * self.bs)
            if key not in self._pc:
                b = req.blocks[k - 1]
                self._pc[key] = b
                self.allocator.share(b)
            self._pc.move_to_end(key)

    def flush_prefix_cache(self) -> None:
        for b in self._pc.values():
            self.allocator.release([b])
        self._pc.clear()

    # -- model invocations ------------------------------------------------------
    def _prefill(self, req: Request) -> int:
        S = len(req.prompt_ids)
        tokens = torch.tensor([req.prompt_ids], dtype=torch.long, device=self.device)
        positions = torch.arange(S, dtype=torch.int32, device=self.device)
        # prefix-cache hits: those chunks' KV already sit in the shared
        # blocks, so their writes are redirected to the dummy block
        # (trash); everything else lands in the request's own blocks.
        shared_tokens = getattr(req, "_shared_chunks", 0) * self.bs
        slots = torch.tensor(
            [(self.dummy_block * self.bs + i % self.bs) if i < shared_tokens
             else req.blocks[i // self.bs] * self.bs + i % self.bs
             for i in range(S)],
            dtype=torch.int32, device=self.device)
        if self.tp > 1:
            from .tp_worker import broadcast_prefill
            broadcast_prefill(tokens, positions, slots)
        lora = self._lora_for([req])
        if lora is None:
            logits = self.model.prefill(tokens, positions, self.caches,
                                        slots)
        else:
            logits = self.model.prefill(tokens, positions, self.caches,
                                        slots, lora=lora)
        return self._sample_first(req, logits)

    def _sample_first(self, req: Request, logits) -> int:
        """Sample the first output token from last-position prefill logits."""
        if self._use_batch_sampler([req]):
            return self._sample_batched(logits[:1], [req])[0]
        S = len(req.prompt_ids)
        # a per-request seed makes sampling reproducible across runs and
        # independent of the request_id the scheduler happened to assign
        base = (req.seed * 2654435761 if req.seed is not None
                else self.seed + req.request_id * 65537)
        logits0 = self._apply_penalties(logits[0], req)
        tok = ops.sample_tokens(logits0.unsqueeze(0), req.temperature,
                                top_p=req.top_p, seed=base + S)
        t = int(tok[0])
        if req.logprobs is not None:
            self._record_logprobs(req, logits0, t)
        return t

    def _prefill_paged(self, req: Request) -> int | None:
        """Run prompt tokens [computed, end) through the model against the
        paged cache: positions below ``computed`` (prefix-cache hit, earlier
        chunks) are read through the request's block table, not recomputed.
        Returns the first output token after the last chunk, else None."""
        S = len(req.prompt_ids)
        start = req.computed
        end = min(S, start + self.prefill_chunk) if self.prefill_chunk else S
        tokens = torch.tensor([req.prompt_ids[start:end]], dtype=torch.long,
                              device=self.device)
        positions = torch.arange(start, end, dtype=torch.int32,
                                 device=self.device)
        # as in _prefill: writes into shared prefix blocks go to the dummy
        # block (only the S-1 token of a fully cached prompt lands there)
        shared_tokens = getattr(req, "_shared_chunks", 0) * self.bs
        slots = torch.tensor(
            [(self.dummy_block * self.bs + i % self.bs) if i < shared_tokens
             else req.blocks[i // self.bs] * self.bs + i % self.bs
             for i in range(start, end)],
            dtype=torch.int32, device=self.device)
        nb = (end + self.bs - 1) // self.bs
        bt = torch.tensor(req.blocks[:nb], dtype=torch.int32,
                          device=self.device)
        lora = self._lora_for([req])
        if lora is None:
            logits = self.model.prefill_paged(tokens, positions, self.caches,
                                              slots, bt, start)
        else:
            logits = self.model.prefill_paged(tokens, positions, self.caches,
                                              slots, bt, start, lora=lora)
        self.stats["prefill_tokens"] += end - start
        if getattr(req, "_chunked", False):
            self.stats["prefill_chunks"] += 1
        req.computed = end
        if end < S:
            return None
        return self._sample_first(req, logits)

    def _prefill_step(self, req: Request) -> int | None:
        """One step of a request's prefill: the whole prompt in one pass
        by default; with the paged-prefill knobs, the uncached part, at
        most prefill_chunk tokens at a time (None = more chunks to go)."""
        if req is not self.prefilling:   # fresh from _admit
            S = len(req.prompt_ids)
            ctx = 0
            if self.prefill_from_cache:
                # at least one token is computed: its logits pick the
                # first output token
                ctx = min(getattr(req, "_shared_chunks", 0) * self.bs, S - 1)
            req._chunked = bool(self.prefill_chunk
                                and S - ctx > self.prefill_chunk)
            if ctx == 0 and not req._chunked:
                tok = self._prefill(req)
                self.stats["prefill_tokens"] += S
                req.computed = S
                return tok
            req.computed = ctx
            self.stats["prefix_skipped_tokens"] += ctx
        return self._prefill_paged(req)

    def _prefill_ctx(self, req: Request) -> int:
        """Prompt tokens of a freshly admitted request that are read from
        the cache instead of computed (at least one token is computed)."""
        if not self.prefill_from_cache:
            return 0
        return min(getattr(req, "_shared_chunks", 0) * self.bs,
                   len(req.prompt_ids) - 1)

    def _admit_batch(self) -> list[Request]:
        """prefill_batch mode: admit up to prefill_batch waiting requests,
        FIFO, through _admit. Stops at the first that does not fit (pool,
        max_batch, the prefill_chunk token budget) or that would hit on a
        prefix a member of this batch is about to publish — it stays in
        ``waiting`` and hits next step. A prompt whose own remainder
        exceeds prefill_chunk is returned alone (chunked path) when first,
        and ends the batch otherwise."""
        batch: list[Request] = []
        publish: set[tuple] = set()
        total = 0
        while self.waiting and len(batch) < self.prefill_batch and \
                len(self.running) + len(batch) < self.max_batch:
            cand = self.waiting[0]
            S = len(cand.prompt_ids)
            hits = 0
            if self.prefix_cache_enabled:
                while (hits + 1) * self.bs <= S and \
                        self._pc_key(cand, (hits + 1) * self.bs) \
                        in self._pc:
                    hits += 1
                if (hits + 1) * self.bs <= S and \
                        self._pc_key(cand, (hits + 1) * self.bs) \
                        in publish:
                    break
            rem = S - (min(hits * self.bs, S - 1)
                       if self.prefill_from_cache else 0)
            # prefill_chunk is the packed forward's token budget
            alone = bool(self.prefill_chunk) and rem > self.prefill_chunk
            if batch and (alone or (self.prefill_chunk and
                                    total + rem > self.prefill_chunk)):
                break
            req = self._admit()
            if req is None:
                break
            batch.append(req)
            if alone:
                break           # chunk by chunk, through _prefill_step
            total += rem
            if self.prefix_cache_enabled:
                for k in range(hits + 1, S // self.bs + 1):
                    publish.add(self._pc_key(req, k * self.bs))
        return batch

    def _prefill_batch(self, reqs: list[Request]) -> list[int]:
        """One packed forward over the uncached prompt tokens of several
        freshly admitted requests; returns each one's first output token."""
        dev = self.device
        toks: list[int] = []
        pos: list[int] = []
        slots: list[int] = []
        q_lens: list[int] = []
        ctx_lens: list[int] = []
        for r in reqs:
            S = len(r.prompt_ids)
            ctx = self._prefill_ctx(r)
            # as in _prefill: writes into shared prefix blocks go to the
            # dummy block
            shared_tokens = getattr(r, "_shared_chunks", 0) * self.bs
            toks.extend(r.prompt_ids[ctx:])
            pos.extend(range(ctx, S))
            slots.extend(
                (self.dummy_block * self.bs + i % self.bs)
                if i < shared_tokens
                else r.blocks[i // self.bs] * self.bs + i % self.bs
                for i in range(ctx, S))
            q_lens.append(S - ctx)
            ctx_lens.append(ctx)
        plan = ops.paged_prefill_plan(q_lens, ctx_lens, dev)
        # rows are padded with the dummy block: never read, always valid
        bt = torch.full((len(reqs), plan.max_blocks(self.bs)),
                        self.dummy_block, dtype=torch.int32)
        for i, r in enumerate(reqs):
            nb = (len(r.prompt_ids) + self.bs - 1) // self.bs
            bt[i, :nb] = torch.tensor(r.blocks[:nb], dtype=torch.int32)
        lora = self._lora_for(reqs)
        logits = self.model.prefill_paged_batch(
            torch.tensor(toks, dtype=torch.long, device=dev),
            torch.tensor(pos, dtype=torch.int32, device=dev), self.caches,
            torch.tensor(slots, dtype=torch.int32, device=dev),
            bt.to(dev), plan, **({} if lora is None else {"lora": lora}))
        first = [self._sample_first(r, logits[i:i + 1])
                 for i, r in enumerate(reqs)]
        for r, t, c in zip(reqs, q_lens, ctx_lens):
            r._chunked = False
            r.computed = len(r.prompt_ids)
            self.stats["prefill_tokens"] += t
            self.stats["prefix_skipped_tokens"] += c
        self.stats["prefill_batches"] += 1
        self.stats["prefill_batched_requests"] += len(reqs)
        return first

    def _graph_decoder(self):
        """The engine's GraphedDecoder, built on first use."""
        if self._graphed is None:
            from .graph import GraphedDecoder
            self._graphed = GraphedDecoder(
                self.model, self.caches, self.max_batch,
                self.max_blocks_per_seq, self.dummy_block, self.device)
        return self._graphed

    def _decode_batch(self, reqs: list[Request]) -> list[int]:
        B = len(reqs)
        dev = self.device
        last = [r.prompt_ids[-1] if not r.output_ids else r.output_ids[-1]
                for r in reqs]
        # RoPE position of the token being generated = absolute seq_len - 1
        # (keys were roped at absolute positions too, so windowed suffixes
        # stay exact). Its kv slot / the attended seq_len use the VIRTUAL
        # position within the retained blocks: absolute minus dropped.
        pos = [r.seq_len - 1 for r in reqs]
        vpos = [r.seq_len - 1 - r.dropped for r in reqs]
        slots = []
        for r, v in zip(reqs, vpos):
            blk = r.blocks[v // self.bs]
            slots.append(blk * self.bs + v % self.bs)
        # strict sliding window: attend to exactly the last W virtual
        # positions (block dropping keeps memory bounded; seq_starts
        # removes the residual 0..15-token block slack)
        W = self.cfg.sliding_window
        starts = [max(0, v + 1 - W) if W else 0 for v in vpos]

        if self.lora_pool is not None and \
                any(r.adapter is not None for r in reqs):
            return self._sample_batch(
                self._decode_lora(reqs, last, pos, slots, vpos, starts),
                reqs)
        if self.use_graphs and B <= self.max_batch:
            logits = self._graph_decoder().decode(last, pos, slots,
                                          [r.blocks for r in reqs],
                                          [v + 1 for v in vpos], starts)
        else:
            maxb = max(len(r.blocks) for r in reqs)
            bt = torch.zeros(B, maxb, dtype=torch.int32)
            for i, r in enumerate(reqs):
                bt[i, :len(r.blocks)] = torch.tensor(r.blocks,
                                                     dtype=torch.int32)
            tokens = torch.tensor(last, dtype=torch.long, device=dev)
            positions = torch.tensor(pos, dtype=torch.int32, device=dev)
            slot_t = torch.tensor(slots, dtype=torch.int32, device=dev)
            seq_lens = torch.tensor([v + 1 for v in vpos], dtype=torch.int32,
                                    device=dev)
            start_t = torch.tensor(starts, dtype=torch.int32, device=dev)
            bt = bt.to(dev)
            if self.tp > 1:
                from .tp_worker import broadcast_decode
                broadcast_decode(tokens, positions, slot_t, bt, seq_lens,
                                 start_t)
            logits = self.model.decode(tokens, positions, self.caches, slot_t,
                                       bt, seq_lens, seq_starts=start_t)
        return self._sample_batch(logits, reqs)

    def _decode_lora(self, reqs, last, pos, slots, vpos, starts):
        """The decode step of a batch in which at least one row has an
        adapter: the same call with ``lora=``, through the graph family
        keyed (bucket, "lora") under graphs."""
        B = len(reqs)
        dev = self.device
        lslots = self._lora_slots(reqs)
        self.stats["lora_decode_steps"] += 1
        self.stats["lora_rows"] += sum(1 for s in lslots if s >= 0)
        if self.use_graphs and B <= self.max_batch:
            gd = self._graph_decoder()
            if gd.lora_pool is None:
                gd.enable_lora(self.lora_pool)
            return gd.decode(last, pos, slots,
                                        [r.blocks for r in reqs],
                                        [v + 1 for v in vpos], starts,
                                        adapter_slots=lslots)
        from .lora import LoraBatch
        maxb = max(len(r.blocks) for r in reqs)
        bt = torch.zeros(B, maxb, dtype=torch.int32)
        for i, r in enumerate(reqs):
            bt[i, :len(r.blocks)] = torch.tensor(r.blocks, dtype=torch.int32)
        return self.model.decode(
            torch.tensor(last, dtype=torch.long, device=dev),
            torch.tensor(pos, dtype=torch.int32, device=dev), self.caches,
            torch.tensor(slots, dtype=torch.int32, device=dev), bt.to(dev),
            torch.tensor([v + 1 for v in vpos], dtype=torch.int32,
                         device=dev),
            seq_starts=torch.tensor(starts, dtype=torch.int32, device=dev),
            lora=LoraBatch(self.lora_pool, lslots))

    def _spec_decode(self, reqs: list[Request]) -> list[list[int]] | None:
        """One speculative step over the running batch: draft, verify in
        one forward, sample every row, accept the agreeing prefix. Returns
        each request's emitted tokens (one or more), or None when the step
        has to take the normal path: no row has a draft, or a row has an
        adapter."""
        if any(r.adapter is not None for r in reqs):
            return None
        K, bs = self.speculative, self.bs
        free = len(self.allocator.free)
        drafts: list[list[int]] = []
        for r in reqs:
            L = r.seq_len
            n = min(K, r.max_new_tokens - len(r.output_ids) - 1,
                    self.cfg.max_seq_len - 1 - L)
            if (r.presence_penalty or r.frequency_penalty
                    or r.repetition_penalty != 1.0
                    or r.logprobs is not None):
                n = 0
            d = [int(t) for t in self.drafter.propose(r, n)][:n] \
                if n > 0 else []
            # a drafter is user code: an id outside the vocabulary would
            # index the embedding out of bounds, so the draft ends there
            V = self.cfg.vocab_size
            for j, t in enumerate(d):
                if not 0 <= t < V:
                    d = d[:j]
                    break
            # blocks for positions L-1 .. L-1+len(d) must be free NOW:
            # a draft never evicts or preempts
            while d and (L - 1 + len(d)) // bs + 1 - len(r.blocks) > free:
                d.pop()
            if d:
                need = (L - 1 + len(d)) // bs + 1 - len(r.blocks)
                if need > 0:
                    r.blocks.extend(self.allocator.alloc(need))
                    free -= need
            drafts.append(d)
        if not any(drafts):
            return None
        dev = self.device
        tok_rows, pos_rows, slot_rows = [], [], []
        for r, d in zip(reqs, drafts):
            L = r.seq_len
            last = r.output_ids[-1] if r.output_ids else r.prompt_ids[-1]
            tok_rows.append([last] + d)
            pos_rows.append(list(range(L - 1, L + len(d))))
            slot_rows.append([r.blocks[p // bs] * bs + p % bs
                              for p in pos_rows[-1]])
        seq_lens = [r.seq_len + len(d) for r, d in zip(reqs, drafts)]
        B = len(reqs)
        if self.use_graphs and B <= self.max_batch:
            gd = self._graph_decoder()
            if gd.verify_T is None:
                gd.enable_verify(K + 1)
            T = K + 1
            logits = gd.verify(tok_rows, pos_rows, slot_rows,
                                          [r.blocks for r in reqs], seq_lens)
        else:
            T = 1 + max(len(d) for d in drafts)
            maxb = max(len(r.blocks) for r in reqs)
            bt = torch.full((B, maxb), self.dummy_block, dtype=torch.int32)
            for i, r in enumerate(reqs):
                bt[i, :len(r.blocks)] = torch.tensor(r.blocks,
                                                     dtype=torch.int32)
            pad_slot = self.dummy_block * bs
            tokens = [t + [0] * (T - len(t)) for t in tok_rows]
            poss = [p + [p[-1]] * (T - len(p)) for p in pos_rows]
            slots = [s + [pad_slot] * (T - len(s)) for s in slot_rows]
            logits = self.model.verify(
                torch.tensor(tokens, dtype=torch.long, device=dev),
                torch.tensor(poss, dtype=torch.int32, device=dev),
                self.caches,
                torch.tensor(slots, dtype=torch.int32, device=dev),
                bt.to(dev),
                torch.tensor(seq_lens, dtype=torch.int32, device=dev),
                torch.tensor([len(t) for t in tok_rows], dtype=torch.int32,
                             device=dev))
        # every real row is sampled at the seed its position would get in a
        # step of its own
        idx, owners, seed_pos = [], [], []
        for i, (r, d) in enumerate(zip(reqs, drafts)):
            for j in range(len(d) + 1):
                idx.append(i * T + j)
                owners.append(r)
                seed_pos.append(r.seq_len + j)
        if len(idx) != logits.shape[0]:
            logits = logits.index_select(
                0, torch.tensor(idx, dtype=torch.long, device=dev))
        sampled = self._sample_batched(logits, owners, seed_pos)
        out: list[list[int]] = []
        k = 0
        self.stats["spec_steps"] += 1
        for r, d in zip(reqs, drafts):
            s = sampled[k:k + len(d) + 1]
            k += len(d) + 1
            a = 0
            while a < len(d) and s[a] == d[a]:
                a += 1
            # the drafts were trimmed to max_new_tokens above, so the run
            # fits; a stop id inside it ends it there
            emit = s[:a + 1]
            for j, t in enumerate(emit):
                if r.stop_ids and t in r.stop_ids:
                    emit = emit[:j + 1]
                    break
            self.stats["spec_drafted"] += len(d)
            self.stats["spec_accepted"] += len(emit) - 1
            out.append(emit)
        return out

    def _use_batch_sampler(self, reqs: list[Request]) -> bool:
        return self.batch_sampler or any(r.top_k > 0 or r.min_p > 0.0
                                         for r in reqs)

    def _token_counts(self, r: Request) -> dict:
        """{token id: count} over the request's prompt + output. Counted
        once, then one token per step; recounted when the sequence is not
        the counted one plus new output (preemption folds the output into
        the prompt)."""
        ent = self._tok_counts.get(r.request_id)
        n_p, n_o = len(r.prompt_ids), len(r.output_ids)
        if ent is None or ent["prompt"] != n_p or ent["out"] > n_o:
            cnt: dict[int, int] = {}
            for t in r.prompt_ids:
                cnt[t] = cnt.get(t, 0) + 1
            ent = {"prompt": n_p, "out": 0, "cnt": cnt}
            self._tok_counts[r.request_id] = ent
        cnt = ent["cnt"]
        for t in r.output_ids[ent["out"]:]:
            cnt[t] = cnt.get(t, 0) + 1
        ent["out"] = n_o
        return cnt

    def _sample_batched(self, logits, reqs: list[Request],
                        seed_pos: list[int] | None = None) -> list[int]:
        """One ops.sample_batch call and one download for the whole
        batch, each row with its own parameters and seed. ``seed_pos``
        (speculative verify: a request may own several rows) gives each
        row's sequence length for the seed instead of ``r.seq_len``."""
        rows, counts = [], []
        for i, r in enumerate(reqs):
            base = (r.seed * 2654435761 if r.seed is not None
                    else self.seed + r.request_id * 65537)
            rows.append({"temperature": r.temperature, "top_k": r.top_k,
                         "top_p": r.top_p, "min_p": r.min_p,
                         "presence": r.presence_penalty,
                         "frequency": r.frequency_penalty,
                         "repetition": r.repetition_penalty,
                         "seed": base + (r.seq_len if seed_pos is None
                                         else seed_pos[i])})
            pen = (r.presence_penalty or r.frequency_penalty
                   or r.repetition_penalty != 1.0)
            counts.append(self._token_counts(r) if pen else None)
        want = [r.logprobs for r in reqs if r.logprobs is not None]
        V = logits.shape[-1]
        L = min(max(want, default=0), ops.sampling.MAX_LOGPROBS, V)
        params, penalties = ops.pack_sample_batch(rows, counts)
        res = ops.sample_batch(logits.reshape(-1, V).contiguous(), params,
                               penalties, num_logprobs=L).host()
        out = res.tokens.tolist()
        self.stats["sampler_batched_steps"] += 1
        if want:
            lps = res.logprobs.tolist()
            ids, tops = res.top_ids.tolist(), res.top_logprobs.tolist()
            for i, r in enumerate(reqs):
                if r.logprobs is None:
                    continue
                entry = {"logprob": lps[i]}
                k = min(r.logprobs or 0, L)
                if k > 0:
                    entry["top"] = list(zip(ids[i][:k], tops[i][:k]))
                r.logprob_data.append(entry)
        return out

    def _sample_batch(self, logits, reqs: list[Request]) -> list[int]:
        if self._use_batch_sampler(reqs):
            return self._sample_batched(logits, reqs)
        seed = self.seed + 1_000_003 * reqs[0].seq_len
        params = {(r.temperature, r.top_p) for r in reqs}
        plain = all(r.seed is None and not r.presence_penalty and
                    not r.frequency_penalty and
                    r.repetition_penalty == 1.0 for r in reqs)
        if len(params) == 1 and plain:
            t, p = params.pop()
            toks = ops.sample_tokens(logits, t, top_p=p, seed=seed)
            out = toks.tolist()     # one device-to-host copy, not one per row
        else:
            # heterogeneous sampling params / custom seeds: row-by-row
            out = []
            for i, r in enumerate(reqs):
                rs = (r.seed * 2654435761 + r.seq_len
                      if r.seed is not None else seed + r.request_id)
                row = self._apply_penalties(logits[i], r)
                tok = ops.sample_tokens(row.unsqueeze(0), r.temperature,
                                        top_p=r.top_p, seed=rs)
                out.append(int(tok[0]))
        for i, r in enumerate(reqs):
            if r.logprobs is not None:
                self._record_logprobs(r, logits[i], out[i])
        return out

    def _apply_window(self) -> None:
        """Free whole front KV blocks that fall entirely outside the
        sliding window of the next query (absolute position seq_len - 1).
        Dropping whole blocks keeps the within-block slot offsets of the
        retained tokens unchanged, so no cache data moves."""
        w = self.cfg.sliding_window
        if not w:
            return
        for r in self.running:
            while r.dropped + self.bs <= r.seq_len - w and len(r.blocks) > 1:
                self.allocator.release([r.blocks.pop(0)])
                r.dropped += self.bs
                self.stats["window_dropped_blocks"] += 1

    def _preempt(self, r: Request) -> None:
        """Release a running request's cache and requeue it: its generated
        tokens become part of the prompt for the re-prefill."""
        self.allocator.release(r.blocks)
        r.blocks = []
        r.dropped = 0
        r.prompt_ids = r.prompt_ids + r.output_ids
        r.max_new_tokens -= len(r.output_ids)
        r.output_ids = []
        self.stats["preemptions"] += 1
        if hasattr(r, "_watch_sent"):
            r._watch_sent = 0  # post-preempt tokens are all new to watchers
        self.running.remove(r)
        self.waiting.insert(0, r)

    def _preempt_newest(self, exclude: Request) -> bool:
        for r in reversed(self.running):
            if r is not exclude:
                self._preempt(r)
                return True
        return False

    def cancel(self, request_id: int) -> bool:
        """Stop a request: waiting -> dropped now; part-way through a
        chunked prefill -> dropped now, blocks released; running ->
        finishes at the next scheduler sweep."""
        for r in self.waiting:
            if r.request_id == request_id:
                self.waiting.remove(r)
                r.finished = True
                self._forget(r)
                return True
        r = self.prefilling
        if r is not None and r.request_id == request_id:
            self.prefilling = None
            self.allocator.release(r.blocks)
            r.blocks = []
            r.finished = True
            self._forget(r)
            return True
        for r in self.running:
            if r.request_id == request_id:
                r.max_new_tokens = max(1, len(r.output_ids))
                return True
        return False

    # -- scheduler step ----------------------------------------------------------
    def step(self) -> list[Request]:
        """One engine iteration. Returns requests finished this step."""
        self.stats["steps"] += 1
        finished = []
        # sweep first: requests already satisfied (cancel() capped their
        # max_new_tokens between steps) must not decode one extra token
        self._sweep_finished(finished)
        # a prefill in flight takes its next chunk before anything new is
        # admitted
        tr = get_tracer()
        # prefill_batch mode: one prefill forward per step — the next chunk
        # of a prefill in flight, else a packed one for two or more
        # admissions, else the single-request path below for one
        batched = self.prefill_batch > 1
        batch: list[Request] = []
        if batched and self.prefilling is None:
            batch = self._admit_batch()
            req = batch[0] if len(batch) == 1 else None
        else:
            req = self.prefilling if self.prefilling is not None \
                else self._admit()
        if len(batch) > 1:
            try:
                if tr:
                    with tr.span(
                            "prefill_batch", requests=len(batch),
                            tokens=sum(len(r.prompt_ids) for r in batch)):
                        firsts = self._prefill_batch(batch)
                else:
                    firsts = self._prefill_batch(batch)
            except Exception:
                # as for a single prefill: no member may leak its blocks
                for r in batch:
                    self.allocator.release(r.blocks)
                    r.blocks = []
                    r.finished = True
                raise
            for r, first in zip(batch, firsts):
                self.stats["prefills"] += 1
                if self.prefix_cache_enabled:
                    self._pc_insert(r)
                r.output_ids.append(first)
                self.running.append(r)
            self._sweep_finished(finished)
        if req is None and not batch and not self.running and self.waiting:
            head = self.waiting[0]
            need = (len(head.prompt_ids) + self.bs - 1) // self.bs + 1
            if self.prefix_cache_enabled:
                for k in range(1, len(head.prompt_ids) // self.bs + 1):
                    if self._pc_key(head, k * self.bs) in self._pc:
                        need -= 1
                    else:
                        break
            if need > self.allocator.num_blocks:
                r = self.waiting.pop(0)
                r.finished = True
                raise RuntimeError(
                    f"prompt of {len(r.prompt_ids)} tokens cannot fit the KV "
                    f"cache ({self.allocator.num_blocks} blocks)")
        n_admitted = 0
        while req is not None:
            try:
                if tr:
                    with tr.span("prefill", tokens=len(req.prompt_ids),
                                 request=req.request_id):
                        first = self._prefill_step(req)
                else:
                    first = self._prefill_step(req)
            except Exception:
                # _admit already popped req from waiting and allocated its
                # blocks; releasing here (shared prefix blocks are
                # refcounted, release decrements) keeps a failing request
                # from leaking KV pool forever.
                self.prefilling = None
                self.allocator.release(req.blocks)
                req.blocks = []
                req.finished = True
                raise
            if first is None:
                # more chunks to go: keep the blocks, decode the running
                # sequences, continue next step
                self.prefilling = req
                break
            self.prefilling = None
            self.stats["prefills"] += 1
            if self.prefix_cache_enabled:
                self._pc_insert(req)
            req.output_ids.append(first)
            self.running.append(req)
            # the prefill token may already satisfy the request
            self._sweep_finished(finished)
            n_admitted += 1
            req = (self._admit() if not batched and
                   n_admitted < self.max_prefills_per_step else None)
        # decode every step — admissions must not starve running
        # sequences (a freshly prefilled request decodes its second
        # token in the same step it was admitted)
        if self.running:
            self._apply_window()
            # ensure every running seq has a block for the next position;
            # when the pool is exhausted, preempt the newest sequence
            # (its blocks are freed and it requeues for a fresh prefill)
            # instead of failing the whole batch.
            for r in list(self.running):
                if r not in self.running:
                    continue
                while r.seq_len - r.dropped >= len(r.blocks) * self.bs:
                    if not self.allocator.free and self.prefix_cache_enabled:
                        # idle cached prefix blocks are reclaimable memory:
                        # evict before resorting to preemption
                        self._evict_prefix(1)
                    if self.allocator.free:
                        r.blocks.extend(self.allocator.alloc(1))
                    elif not self._preempt_newest(exclude=r):
                        # nothing left to preempt: preempt r itself
                        self._preempt(r)
                        break
            if self.running:
                spec = None
                if self.speculative:
                    if tr:
                        with tr.span("spec_decode", batch=len(self.running)):
                            spec = self._spec_decode(self.running)
                    else:
                        spec = self._spec_decode(self.running)
                if spec is not None:
                    # several tokens per request from one forward
                    for r, ts in zip(self.running, spec):
                        r.output_ids.extend(ts)
                        self.stats["decode_tokens"] += len(ts)
                else:
                    if tr:
                        with tr.span("decode", batch=len(self.running)):
                            toks = self._decode_batch(self.running)
                    else:
                        toks = self._decode_batch(self.running)
                    self.stats["decode_tokens"] += len(toks)
                    for r, t in zip(self.running, toks):
                        r.output_ids.append(t)
        self._sweep_finished(finished)
        return finished

    def _forget(self, r: Request) -> None:
        """Drop the per-request state kept outside the request (penalty
        token counts, the drafter's index) when it leaves the engine."""
        self._tok_counts.pop(r.request_id, None)
        if self.drafter is not None and hasattr(self.drafter, "forget"):
            self.drafter.forget(r.request_id)

    def _sweep_finished(self, finished: list[Request]) -> None:
        for r in list(self.running):
            if (len(r.output_ids) >= r.max_new_tokens
                    or (r.stop_ids and r.output_ids[-1] in r.stop_ids)
                    or r.seq_len >= self.cfg.max_seq_len):
                r.finished = True
                self.allocator.release(r.blocks)
                r.blocks = []
                self.running.remove(r)
                self._forget(r)
                finished.append(r)

    def has_work(self) -> bool:
        return bool(self.waiting or self.running
                    or self.prefilling is not None)

    # -- convenience --------------------------------------------------------------
    def generate(self, prompt_ids: list[int], max_new_tokens: int = 64,
                 temperature: float = 0.0) -> list[int]:
        req = self.submit(prompt_ids, max_new_tokens, temperature)
        while not req.finished:
            self.step()
        return req.output_ids
