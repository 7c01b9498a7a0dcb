#!/usr/bin/env python3
"""Generate docs/api.md from the CRD dataclasses (the reference renders
the same document with crd-ref-docs, reference Makefile:204-214).

Run: python scripts/gen_api_docs.py  (rewrites docs/api.md in place).
"""
import dataclasses
import inspect
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from runbooks_amd.api import types as T


def type_name(t) -> str:
    s = str(t).replace("typing.", "")
    s = s.replace("runbooks_amd.api.types.", "")
    s = s.replace("<class '", "").replace("'>", "")
    return s


def doc_for(cls) -> str:
    out = [f"### {cls.__name__}\n"]
    doc = inspect.getdoc(cls)
    if doc:
        out.append(doc.split("\n\n")[0] + "\n")
    out.append("| field | type | default |")
    out.append("|---|---|---|")
    for f in dataclasses.fields(cls):
        if f.name.startswith("_"):
            continue
        default = ""
        if f.default is not dataclasses.MISSING:
            default = repr(f.default)
        elif f.default_factory is not dataclasses.MISSING:  # type: ignore
            default = f.default_factory.__name__ + "()"
        out.append(f"| `{f.name}` | `{type_name(f.type)}` | {default} |")
    out.append("")
    return "\n".join(out)


# The Server's HTTP surface is not a CRD type; its request fields are
# documented by hand here so regenerating keeps them.
HTTP_API = """\
## Server HTTP API (`POST /v1/completions`, `POST /v1/chat/completions`)

OpenAI-style request bodies (`runbooks_amd/serve/http.py`). Sampling
fields, all optional and per request:

| field | type | default | meaning |
|---|---|---|---|
| `temperature` | `float` | 0.0 | `<= 0` is greedy decoding |
| `top_p` | `float` | 1.0 | nucleus: keep the most likely tokens whose mass reaches `top_p` |
| `top_k` | `int` | 0 | keep the `top_k` most likely tokens (ties at the k-th value are kept); 0 = off |
| `min_p` | `float` | 0.0 | keep tokens with probability `>= min_p * p_max`; 0 = off |
| `seed` | `int` | None | reproducible sampling, independent of the batch |
| `presence_penalty` | `float` | 0.0 | subtracted once from every token seen so far |
| `frequency_penalty` | `float` | 0.0 | subtracted per occurrence |
| `repetition_penalty` | `float` | 1.0 | seen logits divided (if positive) or multiplied by it |
| `logprobs` | `int` | None | completions only: top-k logprobs per generated token |

A request that sets `top_k` or `min_p` is sampled by the batched
per-request sampler (`ops.sample_batch`, `sample_batch.hip` in
`docs/kernels.md`) together with the rest of its decode batch: penalties,
then temperature, then top-k, top-p (within the top-k survivors) and
min-p as value thresholds, then the draw. `RB_BATCH_SAMPLER=1`
(`PARAM_BATCH_SAMPLER` on the server image) sends every batch that way;
by default batches without `top_k` / `min_p` keep the older path, which
applies `top_p` before the temperature.

### Speculative decoding

`Engine(..., speculative=K, spec_ngram=3, drafter=None)` (env
`RB_SPECULATIVE`, `RB_SPEC_NGRAM`; `PARAM_SPECULATIVE` / `PARAM_SPEC_NGRAM`
on the server image) lets one engine step emit several tokens per request:
each running request brings up to `K` (1..7) draft tokens, one forward
(`Transformer.verify`, `attention_verify.hip` in `docs/kernels.md`) scores
the request's last token and its drafts, every row is sampled by
`ops.sample_batch` with the seed its position would get in a step of its
own, and drafts are kept while they equal the sample. Given equal logits
the completion is token for token that of `batch_sampler=True` without
speculation, greedy or seeded; no request field changes. Streaming
delivers every token of a step, in order. A `drafter` is any object with
`propose(request, k) -> list[int]` (at most `k` tokens; an optional
`forget(request_id)` is called when the request leaves); the default
`NgramDrafter(spec_ngram)` proposes what followed the most recent earlier
occurrence of the request's last `spec_ngram` (down to 1) tokens in its own
prompt and output. Requests with a penalty or `logprobs` are served without
drafts, a batch with an adapter row takes the normal step. `K = 0`
(default) allocates nothing and changes no path; the knob is ignored with
one printed line at TP>1, with an fp8 KV cache, for sliding-window models
and at head_dim 256. `engine.stats` adds `spec_steps`, `spec_drafted` and
`spec_accepted`.

### LoRA adapters: the `model` field

One server can serve many LoRA fine-tunes of its base model
(`runbooks_amd/serve/lora.py`). `model` picks one per request:

| `model` | served |
|---|---|
| missing, `""` or the base model's name | the base model |
| the name of a loaded adapter | base + that adapter |
| anything else | 404, `{"error": {"message": "model '<id>' not found"}}` |

The response's `model` echoes what was served. `GET /v1/models` lists the
base and every loaded adapter, adapters with `"parent": <base>`.

Engine knobs (`Engine(..., max_loras=0, lora_rank=16)`; env `RB_MAX_LORAS`,
`RB_LORA_RANK`; `PARAM_LORA_ADAPTERS` / `PARAM_MAX_LORAS` /
`PARAM_LORA_RANK` on the server image, `docs/container-contract.md`):
`max_loras` adapter slots of rank `lora_rank` (a multiple of 16, at most
64) are preallocated per block and GEMM site; with the default 0 nothing
is allocated and no code path changes. `engine.load_adapter(name, path)`
reads a trainer adapter checkpoint (`checkpoint-N/`, or a directory of
them: the latest; `lora_alpha` from its `adapter.json`, else 32) or an HF
PEFT directory (`adapter_model.safetensors` + `adapter_config.json`) on
q/k/v/o/gate/up/down projections; a smaller rank is zero-padded, a larger
one, a shape that does not match the base or any other target is refused
by name. `engine.unload_adapter(name)` is refused while a request uses the
adapter; `engine.adapters()` lists the names; `submit(..., adapter=name)`
raises `KeyError` for an unknown one. Both calls copy into memory the
decode step reads: make them from the thread that steps the engine
(`EngineLoop.load_adapter` / `unload_adapter` queue them there).

A decode batch may mix adapters and adapter-free rows; a batch with at
least one adapter row runs each GEMM site as the plain base GEMM plus
`ops.lora_shrink` / `ops.lora_expand_` (`lora_serve.hip` in
`docs/kernels.md`), under its own hipGraph family. Prefix-cache blocks
are keyed on (adapter, tokens). Supported: TP=1; llama, mistral and gemma
family models (fused qkv and gate-up); any base weight format (bf16,
8-bit, 4-bit with or without `w4_resident`). Anything else raises
`NotImplementedError` when the engine is built, and so does `max_loras >
0` together with an fp8 KV cache: the engine refuses that combination at
construction.
"""


def main():
    kinds = ["Model", "Dataset", "Server", "Notebook"]
    shared = ["Build", "BuildGit", "BuildUpload", "UploadStatus",
              "ObjectRef", "Resources", "GPUResources", "ArtifactsStatus",
              "Condition"]
    parts = [
        "# API reference (`substratus.ai/v1`)\n",
        "Generated by `scripts/gen_api_docs.py` from "
        "`runbooks_amd/api/types.py` — the field-compatible dataclass "
        "mirror of the reference CRDs (reference renders the equivalent "
        "with crd-ref-docs). Regenerate after editing the types.\n",
        "## Kinds\n",
    ]
    for name in kinds:
        parts.append(doc_for(getattr(T, name)))
    parts.append("## Shared types\n")
    for name in shared:
        cls = getattr(T, name, None)
        if cls is not None and dataclasses.is_dataclass(cls):
            parts.append(doc_for(cls))
    parts.append(HTTP_API)
    out = "\n".join(parts)
    dst = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "docs", "api.md")
    with open(dst, "w") as f:
        f.write(out)
    print(f"wrote {dst} ({len(out)} bytes)")


if __name__ == "__main__":
    main()
