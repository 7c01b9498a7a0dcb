"""Adapter pool: many LoRA fine-tunes served over one base model.

``AdapterPool`` preallocates, per transformer block and GEMM site, the
slot stacks the batched per-row kernels read (ops/lora_serve.py):

  site     input        segments (S)     output columns
  qkv      norm1(x)     q, k, v   (3)    fused qkv
  o        attention    o_proj    (1)    hidden
  gateup   norm2(x)     gate, up  (2)    fused gate-up
  down     act(gate)*up down_proj (1)    hidden

The stacks are zero-filled and their addresses never change, so captured
decode graphs stay valid while adapters come and go; ``load`` only copies
into a free slot (on the current stream — call it from the thread that
steps the engine, between steps), ``unload`` frees the slot's name. A
free slot holds stale weights nobody indexes.

``LoraBatch`` is what the model entry points take as ``lora=``: the pool
plus which slot each row (decode) or sequence (prefill) uses, -1 for none.
"""
from __future__ import annotations

import json
import re
from pathlib import Path

import torch

from .. import ops

ATTN_TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj")
MLP_TARGETS = ("gate_proj", "up_proj", "down_proj")
TARGETS = ATTN_TARGETS + MLP_TARGETS
# site -> its segments, in output-column order
SITES = {"qkv": ("q_proj", "k_proj", "v_proj"), "o": ("o_proj",),
         "gateup": ("gate_proj", "up_proj"), "down": ("down_proj",)}
_SITE_OF = {t: (site, s) for site, ts in SITES.items()
            for s, t in enumerate(ts)}
TRAINER_DEFAULT_ALPHA = 32     # train/trainer.py's fixed lora_alpha

_KEY = re.compile(r"^blocks\.(\d+)\.(attn|mlp)\.(\w+)\.lora_(a|b)$")


def unsupported_reason(model) -> str | None:
    """Why this model cannot serve adapters, or None when it can."""
    if getattr(model, "tp", 1) != 1:
        return "adapter serving is single-GPU (TP=1)"
    if model.cfg.parallel_residual or model.cfg.single_norm:
        return (f"{model.cfg.name}: adapter serving covers sequential-"
                f"residual models (llama, mistral, gemma families)")
    for blk in model.blocks:
        if getattr(blk.attn, "_qkv_w", None) is None or \
                getattr(blk.mlp, "_gateup_w", None) is None:
            return (f"{model.cfg.name}: adapter serving needs the fused qkv "
                    f"and gate-up serving path (llama, mistral, gemma "
                    f"families after fuse_for_inference)")
        if blk.attn.o_proj.bias is not None or \
                blk.mlp.down_proj.bias is not None:
            return f"{model.cfg.name}: o_proj / down_proj carry a bias"
        # ops.lora_shrink needs K % 8 == 0, ops.lora_expand_ N % 8 == 0
        dims = {"hidden_size": blk.attn._qkv_w.shape[1],
                "fused qkv width": blk.attn._qkv_w.shape[0],
                "attention width": blk.attn.o_proj.weight.shape[1],
                "intermediate_size": blk.mlp._gateup_w.shape[0] // 2}
        for what, d in dims.items():
            if d % 8:
                return (f"{model.cfg.name}: {what} = {d} is not a multiple "
                        f"of 8, which the per-row LoRA kernels need")
    return None


class Site:
    """One GEMM site's stacks (all slots)."""
    __slots__ = ("a", "b", "seg_ends", "segments", "K", "N")

    def __init__(self, n_slots, R, K, seg_ends, dtype, device):
        self.segments = len(seg_ends)
        self.seg_ends = tuple(seg_ends)
        self.K, self.N = K, seg_ends[-1]
        self.a = torch.zeros(n_slots, self.segments * R, K, dtype=dtype,
                             device=device)
        self.b = torch.zeros(n_slots, self.N, R, dtype=dtype, device=device)


class AdapterPool:
    def __init__(self, model, max_loras: int, rank: int = 16):
        why = unsupported_reason(model)
        if why is not None:
            raise NotImplementedError(why)
        if max_loras < 1:
            raise ValueError(f"max_loras must be >= 1, got {max_loras}")
        if rank % 16 or not 16 <= rank <= ops.lora_serve.MAX_RANK:
            raise ValueError(f"lora_rank must be a multiple of 16 and at "
                             f"most {ops.lora_serve.MAX_RANK}, got {rank}")
        self.model = model
        self.max_loras = int(max_loras)
        self.rank = int(rank)
        blk0 = model.blocks[0]
        # K/N come from the fused tensors themselves: int4-resident
        # placeholders keep their shapes
        dev = blk0.attn.o_proj.weight.device
        if dev.type == "meta":
            dev = model.embed.weight.device
        self.device = dev
        self.dtype = model.dtype
        self.sites: list[dict[str, Site]] = []
        for blk in model.blocks:
            attn, mlp = blk.attn, blk.mlp
            qo, kvo = attn.hq * attn.dh, attn.hkv * attn.dh
            hid = attn._qkv_w.shape[1]
            inter = mlp._gateup_w.shape[0] // 2
            mk = lambda K, ends: Site(self.max_loras, self.rank, K,  # noqa: E731
                                      ends, self.dtype, dev)
            self.sites.append({
                "qkv": mk(hid, (qo, qo + kvo, qo + 2 * kvo)),
                "o": mk(qo, (attn.o_proj.weight.shape[0],)),
                "gateup": mk(hid, (inter, 2 * inter)),
                "down": mk(inter, (mlp.down_proj.weight.shape[0],))})
        self.scales = torch.zeros(self.max_loras, dtype=torch.float32,
                                  device=dev)
        self.scale_host = [0.0] * self.max_loras
        self.names: list[str | None] = [None] * self.max_loras

    # -- bookkeeping -------------------------------------------------------
    def slot_of(self, name: str) -> int:
        try:
            return self.names.index(name)
        except ValueError:
            raise KeyError(f"no adapter named {name!r} is loaded") from None

    def loaded(self) -> list[str]:
        return [n for n in self.names if n is not None]

    def __contains__(self, name) -> bool:
        return name is not None and name in self.names

    def unload(self, name: str) -> None:
        self.names[self.slot_of(name)] = None

    # -- loading -----------------------------------------------------------
    def _need_free_slot(self, name: str) -> None:
        if None not in self.names:
            raise RuntimeError(
                f"adapter {name!r}: all {self.max_loras} adapter slots are in "
                f"use ({', '.join(self.loaded())}); unload one or raise "
                f"max_loras")

    def load(self, name: str, path) -> int:
        """Read an adapter (trainer checkpoint or HF PEFT directory) into
        a free slot; returns the slot."""
        if not name or not isinstance(name, str):
            raise ValueError("adapter name must be a non-empty string")
        if name in self.names:
            raise ValueError(f"adapter {name!r} is already loaded")
        self._need_free_slot(name)
        state, alpha, r_cfg = read_adapter(path, self.model.cfg)
        return self.load_state(name, state, alpha, r_cfg)

    def load_state(self, name: str, state: dict, alpha: float,
                   r: int | None = None) -> int:
        """``state``: native keys ``blocks.i.attn.q_proj.lora_a`` [r, in]
        / ``...lora_b`` [out, r]. Everything is validated before the
        first byte is copied, so a refused adapter leaves the pool as it
        was."""
        if name in self.names:
            raise ValueError(f"adapter {name!r} is already loaded")
        self._need_free_slot(name)
        slot = self.names.index(None)
        R = self.rank
        plan = []          # (dst view, src)
        seen_r = set()
        pairs: dict[tuple, dict] = {}
        for key, w in state.items():
            m = _KEY.match(key)
            if m is None:
                raise ValueError(f"adapter {name!r}: {key} is not a LoRA "
                                 f"tensor of a block's linear layer")
            i, _grp, tgt, kind = int(m[1]), m[2], m[3], m[4]
            if tgt not in TARGETS or \
                    (_grp == "attn") != (tgt in ATTN_TARGETS):
                raise ValueError(
                    f"adapter {name!r}: target {key.rsplit('.', 1)[0]} is "
                    f"not served (only {', '.join(TARGETS)} are)")
            if i >= len(self.sites):
                raise ValueError(f"adapter {name!r}: {key} names block {i}, "
                                 f"the base has {len(self.sites)}")
            pairs.setdefault((i, tgt), {})[kind] = (key, w)
        for (i, tgt), ab in sorted(pairs.items()):
            if set(ab) != {"a", "b"}:
                have = next(iter(ab.values()))[0]
                raise ValueError(f"adapter {name!r}: {have} has no matching "
                                 f"lora_{'b' if 'a' in ab else 'a'}")
            (ka, a), (kb, b) = ab["a"], ab["b"]
            site_name, s = _SITE_OF[tgt]
            site = self.sites[i][site_name]
            lo = site.seg_ends[s - 1] if s else 0
            hi = site.seg_ends[s]
            ra = a.shape[0] if a.dim() == 2 else -1
            if a.dim() != 2 or b.dim() != 2 or b.shape[1] != ra:
                raise ValueError(
                    f"adapter {name!r}: {ka} {tuple(a.shape)} and {kb} "
                    f"{tuple(b.shape)} are not an [r, in] / [out, r] pair")
            if ra > R:
                raise ValueError(
                    f"adapter {name!r}: {ka} has rank {ra}, the pool was "
                    f"built for rank <= {R} (lora_rank)")
            if a.shape[1] != site.K or b.shape[0] != hi - lo:
                raise ValueError(
                    f"adapter {name!r}: {ka} {tuple(a.shape)} / {kb} "
                    f"{tuple(b.shape)} do not match the base's {tgt} "
                    f"[{hi - lo}, {site.K}]")
            seen_r.add(ra)
            plan.append((site.a[slot, s * R:s * R + ra], a))
            plan.append((site.b[slot, lo:hi, :ra], b))
        if not plan:
            raise ValueError(f"adapter {name!r}: no LoRA tensors found")
        if r is None:
            if len(seen_r) != 1:
                raise ValueError(f"adapter {name!r}: mixed ranks "
                                 f"{sorted(seen_r)} and no lora_r given")
            r = seen_r.pop()
        # a rank below the pool's is zero-padded (exact): clear the slot
        # first, which also drops whatever a previous tenant left
        for sites in self.sites:
            for site in sites.values():
                site.a[slot].zero_()
                site.b[slot].zero_()
        for dst, src in plan:
            dst.copy_(src.to(device=self.device, dtype=self.dtype))
        scale = float(alpha) / float(r)
        self.scales[slot] = scale
        self.scale_host[slot] = scale
        self.names[slot] = name
        return slot


def _latest_ckpt(path: Path) -> Path | None:
    ckpts = [p for p in path.glob("checkpoint-*")
             if p.name.split("-")[-1].isdigit()]
    return max(ckpts, key=lambda p: int(p.name.split("-")[-1])) \
        if ckpts else None


def read_adapter(path, cfg):
    """-> (state with native keys, lora_alpha, lora_r or None)."""
    from safetensors.torch import load_file
    path = Path(path)
    if (path / "adapter_model.safetensors").exists():
        # HF PEFT layout
        meta = json.loads((path / "adapter_config.json").read_text())
        from ..models.load import convert_hf_state_dict
        raw = load_file(str(path / "adapter_model.safetensors"))
        hf = {}
        for k, w in raw.items():
            k = k.removeprefix("base_model.model.")
            hf[k] = w
        state = {}
        for k, w in convert_hf_state_dict(hf, cfg).items():
            if k == "lm_head.weight":       # derived by the converter
                continue
            m = re.match(r"^(.*)\.lora_([AB])(?:\.\w+)?\.weight$", k)
            if m is None:
                raise ValueError(f"{path}: {k} is not a lora_A / lora_B "
                                 f"weight")
            state[f"{m[1]}.lora_{m[2].lower()}"] = w
        return state, float(meta["lora_alpha"]), int(meta["r"])
    if not (path / "model.safetensors").exists():
        ck = _latest_ckpt(path)
        if ck is None:
            raise FileNotFoundError(
                f"{path}: neither a PEFT adapter (adapter_model.safetensors)"
                f" nor a trainer checkpoint (model.safetensors or "
                f"checkpoint-*/)")
        path = ck
    state = {k: w for k, w in
             load_file(str(path / "model.safetensors")).items()
             if "lora_a" in k or "lora_b" in k}
    alpha, r = float(TRAINER_DEFAULT_ALPHA), None
    side = path / "adapter.json"
    if side.exists():
        d = json.loads(side.read_text())
        alpha = float(d.get("lora_alpha", alpha))
        r = int(d["lora_r"]) if d.get("lora_r") else None
    return state, alpha, r


class LoraBatch:
    """``lora=`` argument of Transformer.decode / prefill*.

    ``slots``: host ints, one per decode row or per prefill sequence (-1 =
    none), range-checked here once. ``idx``: the same as a device int32
    tensor for the decode kernels, built on first use (a prefill never
    needs it); the graphed decode passes its static buffer and no
    ``slots`` (it validated the values when it staged them)."""

    def __init__(self, pool: AdapterPool, slots=None, idx=None):
        self.pool = pool
        self.slots = None if slots is None else [int(s) for s in slots]
        if self.slots is not None:
            for s in self.slots:
                if not -1 <= s < pool.max_loras:
                    raise ValueError(f"adapter slot {s} out of range "
                                     f"(-1..{pool.max_loras - 1})")
        if idx is None and self.slots is None:
            raise ValueError("LoraBatch needs slots or idx")
        self._idx = idx

    @property
    def idx(self):
        if self._idx is None:
            self._idx = torch.tensor(self.slots, dtype=torch.int32,
                                     device=self.pool.device)
        return self._idx

    def at(self, layer: int, spans=None) -> "LoraLayer":
        return LoraLayer(self, self.pool.sites[layer], spans)

    def seq_spans(self, bounds) -> list[tuple[int, int, int]]:
        """(row0, row1, slot) of every sequence that has an adapter;
        ``bounds``: the sequences' row boundaries (len = sequences + 1)."""
        if self.slots is None or len(self.slots) != len(bounds) - 1:
            raise ValueError("prefill needs one host slot per sequence")
        return [(bounds[i], bounds[i + 1], s)
                for i, s in enumerate(self.slots) if s >= 0]


class LoraLayer:
    """One block's view of a LoraBatch: ``patch_(y, x, site)`` adds the
    rows' low-rank deltas to the base GEMM's output in place."""

    def __init__(self, batch: LoraBatch, sites: dict, spans):
        self.batch = batch
        self.sites = sites
        self.spans = spans          # None: decode (one row per slot)

    def patch_(self, y, x, site_name: str):
        site = self.sites[site_name]
        b = self.batch
        if self.spans is None:
            x2 = x.reshape(-1, x.shape[-1])
            y2 = y.view(-1, y.shape[-1])
            if not x2.is_contiguous():
                x2 = x2.contiguous()
            idx = b.idx         # values validated by LoraBatch / staging
            t = ops.lora_shrink(x2, site.a, idx, segments=site.segments)
            ops.lora_expand_(y2, t, site.b, b.pool.scales, idx,
                             site.seg_ends)
            return y
        # prefill: rows are whole sequences — plain GEMMs per sequence
        from ..train.lora import _delta_add_
        R = b.pool.rank
        for r0, r1, slot in self.spans:
            xs, ys = x[r0:r1], y[r0:r1]
            scale = b.pool.scale_host[slot]
            t = torch.nn.functional.linear(xs, site.a[slot])
            if site.segments == 1:
                _delta_add_(ys, t, site.b[slot], scale)
                continue
            lo = 0
            for s, hi in enumerate(site.seg_ends):
                ys[:, lo:hi].addmm_(t[:, s * R:(s + 1) * R],
                                    site.b[slot, lo:hi].t(), alpha=scale)
                lo = hi
        return y
