"""server image main.

Parity: substratusai/model-server-basaran (reference
examples/llama2-7b/server.yaml, container-contract.md:50-56) — loads
/content/model, serves an OpenAI-style completions API on :8080 with
"/" readiness. Honors the contract env knobs:

- MODEL_LOAD_IN_8BIT / MODEL_LOAD_IN_4BIT ("1" or "true"): weight-only
  quantized decode (reference examples/llama2-7b/server.yaml:9,
  llama2-70b/server.yaml:9). 8-bit stores fp8-e4m3 + per-channel scales,
  4-bit stores group-64 int4 + bf16 scales; both keep the bf16 masters
  for prefill. 4-bit wins when both are set; both apply at TP=1 on a GPU
  and are otherwise ignored (bf16 serving).
- PARAM_W4_RESIDENT / W4_RESIDENT ("1" or "true", with MODEL_LOAD_IN_4BIT):
  drop the bf16 masters of the 4-bit weights; prefill runs the int4 GEMM
  and the freed memory becomes KV cache.
- PARAM_BATCH_SAMPLER / BATCH_SAMPLER ("1" or "true"): sample each decode
  batch with the batched per-request sampler (one launch, one download);
  unset leaves the engine's RB_BATCH_SAMPLER default.
- PARAM_SPECULATIVE / SPECULATIVE (K in 1..7): speculative decoding with
  up to K n-gram drafts per sequence per step, verified in one forward;
  PARAM_SPEC_NGRAM / SPEC_NGRAM (default 3) is the longest suffix matched.
  Unset leaves the engine's RB_SPECULATIVE / RB_SPEC_NGRAM defaults (off).
- PARAM_LORA_ADAPTERS / LORA_ADAPTERS: LoRA adapters served over the one
  base model, ``name=path,name=path`` (trainer adapter checkpoints or HF
  PEFT directories); a bare directory loads each of its subdirectories
  under its own name. A request picks one with its ``model`` field.
  PARAM_MAX_LORAS / MAX_LORAS (default: the number listed) and
  PARAM_LORA_RANK / LORA_RANK (default 16) size the adapter pool. TP=1.
- TP: tensor parallelism degree (defaults to visible GPU count); ranks
  are spawned via torch.distributed.run over RCCL/xGMI.
"""
from __future__ import annotations

import json
import os
import sys
from pathlib import Path


def _maybe_relaunch_tp() -> bool:
    import torch
    n = int(os.environ.get("TP", "0")) or (
        torch.cuda.device_count() if torch.cuda.is_available() else 1)
    if n <= 1 or os.environ.get("RANK") is not None:
        return False
    os.execvp(sys.executable, [
        sys.executable, "-m", "torch.distributed.run",
        "--standalone", "--local-addr", "127.0.0.1",
        f"--nproc-per-node={n}",
        "-m", "runbooks_amd.workloads.server_main"])
    return True


def parse_lora_adapters(spec: str) -> list[tuple[str, Path]]:
    """``name=path,name=path`` -> [(name, path)]; an entry without ``=``
    is a directory whose subdirectories are adapters named after
    themselves."""
    out: list[tuple[str, Path]] = []
    for item in (i.strip() for i in spec.split(",")):
        if not item:
            continue
        if "=" in item:
            name, path = item.split("=", 1)
            out.append((name.strip(), Path(path.strip())))
            continue
        root = Path(item)
        if not root.is_dir():
            raise ValueError(f"LORA_ADAPTERS: {item} is neither name=path "
                             f"nor a directory of adapters")
        out.extend((p.name, p) for p in sorted(root.iterdir())
                   if p.is_dir() and not p.name.startswith("."))
    names = [n for n, _ in out]
    dup = {n for n in names if names.count(n) > 1}
    if dup or "" in names:
        raise ValueError(f"LORA_ADAPTERS: empty or repeated adapter names "
                         f"{sorted(dup)}")
    return out


def _env(name: str) -> str:
    return os.environ.get(f"PARAM_{name}", os.environ.get(name, ""))


def main():
    if _maybe_relaunch_tp():
        return 0
    import torch

    from ..models import build_model, get_config, list_configs
    from ..models.load import config_from_hf_json, load_pretrained
    from ..parallel import comm
    from ..serve import Engine
    from ..serve.http import serve_forever
    from ..serve.tokenizer import load_tokenizer

    comm.init_from_env()
    model_dir = Path(os.environ.get("MODEL_DIR", "/content/model"))
    # A fine-tuned Model's artifacts hold trainer checkpoints
    # (checkpoint-N/model.safetensors + meta.json) rather than top-level
    # files: serve the latest checkpoint (the Server CRD points at the
    # Model's artifacts — reference server_controller.go model mount).
    if not list(model_dir.glob("*.safetensors")):
        ckpts = sorted(model_dir.glob("checkpoint-*"),
                       key=lambda p: int(p.name.split("-")[-1]))
        if ckpts:
            model_dir = ckpts[-1]
            print(f"server: serving latest checkpoint {model_dir}")
    arch = os.environ.get("PARAM_MODEL") or "llama2-7b"
    marker = model_dir / "config.json"
    cfg = None
    if marker.exists():
        meta = json.loads(marker.read_text())
        name = meta.get("runbooks_amd_config")
        if name and name in list_configs():
            cfg = get_config(name)
        elif "runbooks_amd_fields" in meta:
            from ..models import ModelConfig
            from ..models.config import register
            cfg = register(ModelConfig(**meta["runbooks_amd_fields"]))
        elif "model_type" in meta or "architectures" in meta:
            cfg = config_from_hf_json(marker)
    if cfg is None:
        cfg = get_config(arch)

    dtype = torch.bfloat16 if torch.cuda.is_available() else torch.float32
    model = build_model(cfg, dtype=dtype)
    if model_dir.exists() and list(model_dir.glob("*.safetensors")):
        load_pretrained(model, model_dir, rank=comm.rank(),
                        tp=comm.world_size(), strict=False)
        print(f"server: loaded weights from {model_dir}")

    in_8bit = os.environ.get("MODEL_LOAD_IN_8BIT", "").lower() in ("1", "true")
    # PARAM_KV_FP8 / KV_FP8: e4m3 KV cache (2x capacity, long-context)
    kv_fp8 = os.environ.get("PARAM_KV_FP8",
                            os.environ.get("KV_FP8", "")).lower() in \
        ("1", "true")
    in_4bit = os.environ.get("MODEL_LOAD_IN_4BIT", "").lower() in ("1", "true")
    # PARAM_PREFILL_FROM_CACHE / PREFILL_FROM_CACHE: a prefix-cache hit
    # skips the cached part of the prompt instead of recomputing it
    from_cache = os.environ.get(
        "PARAM_PREFILL_FROM_CACHE",
        os.environ.get("PREFILL_FROM_CACHE", "")).lower() in ("1", "true")
    # PARAM_PREFILL_CHUNK / PREFILL_CHUNK: prompt tokens run per engine
    # step (a multiple of 16; 0 or unset = whole prompt in one pass)
    chunk = int(os.environ.get("PARAM_PREFILL_CHUNK",
                               os.environ.get("PREFILL_CHUNK", "")) or 0)
    # PARAM_PREFILL_BATCH / PREFILL_BATCH: admissions packed into one
    # prefill forward per engine step (0, 1 or unset = one forward each)
    pbatch = int(os.environ.get("PARAM_PREFILL_BATCH",
                                os.environ.get("PREFILL_BATCH", "")) or 0)
    # PARAM_W4_RESIDENT / W4_RESIDENT: serve a 4-bit model from its int4
    # weights alone (no bf16 masters)
    resident = os.environ.get(
        "PARAM_W4_RESIDENT",
        os.environ.get("W4_RESIDENT", "")).lower() in ("1", "true")
    # PARAM_BATCH_SAMPLER / BATCH_SAMPLER: sample every decode batch with
    # the one-launch per-request sampler (unset leaves RB_BATCH_SAMPLER)
    bsampler = os.environ.get(
        "PARAM_BATCH_SAMPLER",
        os.environ.get("BATCH_SAMPLER", "")).lower() in ("1", "true")
    # PARAM_SPECULATIVE / SPECULATIVE: n-gram drafts verified per step
    # (unset leaves RB_SPECULATIVE); PARAM_SPEC_NGRAM / SPEC_NGRAM: the
    # longest suffix the drafter matches
    spec_k = int(_env("SPECULATIVE") or 0)
    spec_n = int(_env("SPEC_NGRAM") or 0)
    loras = parse_lora_adapters(_env("LORA_ADAPTERS"))
    max_loras = int(_env("MAX_LORAS") or len(loras))
    engine = Engine(model, load_in_8bit=in_8bit, load_in_4bit=in_4bit,
                    kv_fp8=kv_fp8, w4_resident=resident or None,
                    # unset leaves the engine's own RB_* env defaults
                    prefill_from_cache=from_cache or None,
                    prefill_chunk=chunk or None,
                    prefill_batch=pbatch or None,
                    batch_sampler=bsampler or None,
                    speculative=spec_k or None,
                    spec_ngram=spec_n or None,
                    # unset / none listed leaves RB_MAX_LORAS, RB_LORA_RANK
                    max_loras=max_loras or None,
                    lora_rank=int(_env("LORA_RANK") or 0) or None)
    for name, path in loras:
        engine.load_adapter(name, path)
        print(f"server: adapter {name!r} loaded from {path}")
    tok = load_tokenizer(model_dir if model_dir.exists() else None)
    if comm.rank() == 0:
        serve_forever(engine, tok, port=int(os.environ.get("PORT", "8080")),
                      model_name=cfg.name)
    else:
        # TP worker ranks follow rank 0's collectives inside the model;
        # they loop in the engine's worker protocol.
        from ..serve.tp_worker import worker_loop
        worker_loop(engine)
    return 0


if __name__ == "__main__":
    sys.exit(main())
