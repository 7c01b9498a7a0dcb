"""Decode-step cost of serving LoRA adapters over one base model:
llama2-7b shapes (random weights), all seven targets, rank 16, batch 32,
context 128, everything under a hipGraph (serve/graph.py).

  step   graphed decode step: adapter-free family; "lora" family with 32
         rows on one adapter / spread over 8 adapters / all rows -1; and
         the adapter-free bucket-4 step (8 merged models = 8 of those)
  sites  lora_shrink and lora_expand_ at the four GEMM sites against the
         PyTorch formulation (a_stack[idx] gather + torch.bmm)

Times are device events around back-to-back replays / launches, rounds of
the variants interleaved in one process; median and min over the rounds.

    python benchmarks/lora_decode.py [OUT.json]
    rocprofv3 --kernel-trace --stats -- \\
        python benchmarks/lora_decode.py --sites-only
"""
import json
import statistics
import sys

import torch

sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1]))
from runbooks_amd import ops  # noqa: E402
from runbooks_amd.models import build_model  # noqa: E402
from runbooks_amd.models.transformer import fuse_for_inference  # noqa: E402
from runbooks_amd.serve.graph import GraphedDecoder  # noqa: E402
from runbooks_amd.serve.lora import AdapterPool  # noqa: E402

DEV = "cuda:0"
B, CTX, R, SLOTS = 32, 128, 16, 8
sites_only = "--sites-only" in sys.argv
_pos = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = _pos[0] if _pos else "lora_decode.json"


def timed(fn, n):
    """us per call: n back-to-back calls between two device events."""
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def rounds(variants, n, reps=7):
    for fn in variants.values():            # warm every shape
        timed(fn, 5)
    got = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            got[k].append(timed(fn, n))
    return {k: {"median_us": round(statistics.median(v), 2),
                "min_us": round(min(v), 2)} for k, v in got.items()}


def bench_sites():
    g = torch.Generator().manual_seed(0)
    res = {}
    idx8 = torch.tensor([m % SLOTS for m in range(B)], dtype=torch.int32,
                        device=DEV)
    sc = torch.full((SLOTS,), 2.0, device=DEV)
    for name, K, ends in (("qkv", 4096, (4096, 8192, 12288)),
                          ("o", 4096, (4096,)),
                          ("gateup", 4096, (11008, 22016)),
                          ("down", 11008, (4096,))):
        S, N = len(ends), ends[-1]
        x = torch.randn(B, K, generator=g).to(torch.bfloat16).to(DEV)
        a = (torch.randn(SLOTS, S * R, K, generator=g) * 0.02) \
            .to(torch.bfloat16).to(DEV)
        b = (torch.randn(SLOTS, N, R, generator=g) * 0.02) \
            .to(torch.bfloat16).to(DEV)
        y = torch.randn(B, N, generator=g).to(torch.bfloat16).to(DEV)
        t = ops.lora_shrink(x, a, idx8, segments=S)
        li = idx8.long()
        seg = torch.zeros(N, dtype=torch.long, device=DEV)
        for e in ends[:-1]:
            seg += (torch.arange(N, device=DEV) >= e).long()

        def torch_shrink():
            return torch.bmm(a[li], x.unsqueeze(2)).squeeze(2)

        def torch_expand():
            # per segment: gather the rows' B, one bmm, scaled add
            lo = 0
            tb = t.to(torch.bfloat16)
            for s, hi in enumerate(ends):
                y[:, lo:hi].add_(torch.bmm(
                    b[li, lo:hi], tb[:, s * R:(s + 1) * R].unsqueeze(2))
                    .squeeze(2), alpha=2.0)
                lo = hi

        ext = ops.ext()
        res[name] = rounds({
            "lora_shrink": lambda: ext.lora_shrink(x, a, idx8, S),
            "torch_gather_bmm_shrink": torch_shrink,
            "lora_expand_": lambda: ext.lora_expand_(y, t, b, sc, idx8,
                                                     list(ends)),
            "torch_gather_bmm_expand": torch_expand}, 200)
        print(name, res[name], flush=True)
    return res


def bench_step():
    model = fuse_for_inference(build_model("llama2-7b", dtype=torch.bfloat16,
                                           device=DEV).eval())
    pool = AdapterPool(model, SLOTS, R)
    g = torch.Generator(device=DEV).manual_seed(1)
    for sites in pool.sites:
        for site in sites.values():
            site.a.normal_(0, 0.02, generator=g)
            site.b.normal_(0, 0.02, generator=g)
    pool.scales.fill_(2.0)
    pool.names = [f"a{i}" for i in range(SLOTS)]
    bs = ops.BLOCK_SIZE
    per_seq = CTX // bs + 1
    nblocks = B * per_seq + 1
    caches = model.alloc_caches(nblocks, DEV)
    gd = GraphedDecoder(model, caches, B, per_seq, nblocks - 1, DEV)
    gd.enable_lora(pool)

    def args(n):
        rows = [list(range(i * per_seq, (i + 1) * per_seq)) for i in range(n)]
        return ([7] * n, [CTX] * n,
                [r[CTX // bs] * bs + CTX % bs for r in rows], rows,
                [CTX + 1] * n, [0] * n)

    a32, a4 = args(B), args(4)
    variants = {
        "base_b32": lambda: gd.decode(*a32),
        "lora_b32_all_rows_none": lambda: gd.decode(
            *a32, adapter_slots=[-1] * B),
        "lora_b32_one_adapter": lambda: gd.decode(
            *a32, adapter_slots=[0] * B),
        "lora_b32_eight_adapters": lambda: gd.decode(
            *a32, adapter_slots=[m % SLOTS for m in range(B)]),
        "base_b4": lambda: gd.decode(*a4)}
    res = rounds(variants, 20)
    res["eight_merged_models_8x_base_b4_us"] = round(
        8 * res["base_b4"]["median_us"], 1)
    print(res, flush=True)
    return res


def main():
    res = {"sites": bench_sites()}
    if not sites_only:
        res["step"] = bench_step()
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


main()
