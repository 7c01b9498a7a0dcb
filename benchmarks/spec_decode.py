"""Speculative decoding: what a verify step costs and what it buys.

  kernel  ops.paged_verify (attention_verify.hip) against the baseline
          already in the tree, ops.paged_prefill_batch on the same rows,
          and against T calls of ops.paged_decode. llama2-7b geometry
          (32/32 heads, Dh 128, plain V) and llama2-70b geometry (64/8,
          Dh 128, transposed V); B 1/8/32, T 5, context 512/2048.
  step    llama2-7b shapes (random weights), hipGraph replays: the verify
          step at T = 5 against the decode step at B 1/8/32, context 512.
          r = verify / decode; a verify step pays for itself once it
          accepts r - 1 drafts on average.
  engine  tokens/s of Engine(speculative=4) against Engine(batch_sampler=
          True) at B = 8, 64 new tokens: a prompt that repeats itself with
          the n-gram drafter, the same with a drafter replaying the
          non-speculative run (every draft right), and random tokens with a
          drafter that is always wrong (pure overhead).

Times are device events around back-to-back launches / replays, rounds of
the variants interleaved in one process; median and min over the rounds.

    python benchmarks/spec_decode.py [OUT.json] [--kernel-only]
"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1]))
from runbooks_amd import ops  # noqa: E402
from runbooks_amd.models import build_model  # noqa: E402
from runbooks_amd.models.transformer import fuse_for_inference  # noqa: E402
from runbooks_amd.serve import Engine  # noqa: E402
from runbooks_amd.serve.graph import GraphedDecoder  # noqa: E402

DEV = "cuda:0"
BS = ops.BLOCK_SIZE
T = 5
kernel_only = "--kernel-only" in sys.argv
_pos = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = _pos[0] if _pos else "spec_decode.json"


def timed(fn, n):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def rounds(variants, n, reps=7):
    for fn in variants.values():
        timed(fn, 3)
    got = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            got[k].append(timed(fn, n))
    return {k: {"median_us": round(statistics.median(v), 2),
                "min_us": round(min(v), 2)} for k, v in got.items()}


def bench_kernel():
    res = {}
    g = torch.Generator().manual_seed(0)
    for geo, Hq, Hkv, vt in (("llama2-7b", 32, 32, False),
                             ("llama2-70b", 64, 8, True)):
        for B in (1, 8, 32):
            for ctx in (512, 2048):
                S = ctx + T
                nb = (S + BS - 1) // BS
                kc, vc = ops.alloc_kv_cache(B * nb + 1, Hkv, 128, DEV,
                                            v_transposed=vt)
                kc.copy_(torch.randn(kc.shape, generator=g).to(kc.dtype))
                vc.copy_(torch.randn(vc.shape, generator=g).to(vc.dtype))
                perm = torch.randperm(B * nb, generator=g).to(torch.int32)
                table = perm.view(B, nb).to(DEV)
                q = torch.randn(B, T, Hq, 128, generator=g) \
                    .to(torch.bfloat16).to(DEV)
                qp = q.view(B * T, Hq, 128)
                sl = torch.full((B,), S, dtype=torch.int32, device=DEV)
                ql = torch.full((B,), T, dtype=torch.int32, device=DEV)
                plan = ops.paged_prefill_plan([T] * B, [ctx] * B, DEV)
                qd = [q[:, t].contiguous() for t in range(T)]
                sd = [torch.full((B,), ctx + t + 1, dtype=torch.int32,
                                 device=DEV) for t in range(T)]
                ns_d = ops.attention._auto_nsplit(B, Hkv, sl, mfma=vt)
                ns_v = ops.attention.verify_auto_nsplit(
                    B, Hkv, (Hq // Hkv) * T, nb)

                def decodes():
                    for t in range(T):
                        ops.paged_decode(qd[t], kc, vc, table, sd[t],
                                         nsplit=ns_d)

                key = f"{geo}_B{B}_ctx{ctx}"
                res[key] = rounds({
                    "paged_verify": lambda: ops.paged_verify(
                        q, kc, vc, table, sl, ql, nsplit=ns_v),
                    "paged_prefill_batch": lambda: ops.paged_prefill_batch(
                        qp, kc, vc, table, plan),
                    f"{T}x_paged_decode": decodes}, 20)
                res[key]["verify_nsplit"] = ns_v
                print(key, res[key], flush=True)
                del kc, vc
    return res


def bench_step(model):
    res = {}
    ctx = 512
    per_seq = (ctx + T) // BS + 2
    for B in (1, 8, 32):
        nblocks = B * per_seq + 1
        caches = model.alloc_caches(nblocks, DEV)
        gd = GraphedDecoder(model, caches, B, per_seq, nblocks - 1, DEV)
        gd.enable_verify(T)
        rows = [list(range(i * per_seq, (i + 1) * per_seq)) for i in range(B)]
        dec = ([7] * B, [ctx] * B,
               [r[ctx // BS] * BS + ctx % BS for r in rows], rows,
               [ctx + 1] * B, [0] * B)
        pos = list(range(ctx, ctx + T))
        ver = ([[7] * T] * B, [pos] * B,
               [[r[p // BS] * BS + p % BS for p in pos] for r in rows], rows,
               [ctx + T] * B)
        r = rounds({"decode": lambda: gd.decode(*dec),
                    "verify_T5": lambda: gd.verify(*ver)}, 20)
        ratio = r["verify_T5"]["median_us"] / r["decode"]["median_us"]
        r["ratio"] = round(ratio, 3)
        r["break_even_accepted_per_step"] = round(ratio - 1, 3)
        res[f"B{B}"] = r
        print(f"step B={B}", r, flush=True)
        del gd, caches
    return res


class _Replay:
    def __init__(self, by_prompt, wrong=False):
        self.by_prompt, self.wrong = by_prompt, wrong

    def propose(self, req, k):
        n = len(req.output_ids)
        d = self.by_prompt[tuple(req.prompt_ids)][n:n + k]
        return [(t + 1) % 32000 for t in d] if self.wrong else d


def bench_engine():
    g = torch.Generator().manual_seed(2)
    Bq, new = 8, 64
    sets = {
        "repeating": [(torch.randint(1, 32000, (16,), generator=g).tolist())
                      * 8 for _ in range(Bq)],
        "random": [torch.randint(1, 32000, (128,), generator=g).tolist()
                   for _ in range(Bq)]}

    def run(prompts, **kw):
        # a fresh model per engine: each engine fuses and registers its own
        model = build_model("llama2-7b", dtype=torch.bfloat16,
                            device=DEV).eval()
        eng = Engine(model, device=DEV, kv_blocks=512, max_batch=Bq, **kw)
        eng.max_prefills_per_step = Bq
        best = None
        for _ in range(3):                      # first pass captures graphs
            reqs = [eng.submit(p, max_new_tokens=new) for p in prompts]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while eng.has_work():
                eng.step()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        st = {k: v for k, v in eng.stats.items() if k.startswith("spec")}
        del eng, model
        torch.cuda.empty_cache()
        return reqs, {"tokens_per_s": round(Bq * new / best, 1), **st}

    res = {}
    for name, prompts in sets.items():
        reqs, base = run(prompts, batch_sampler=True)
        rec = {tuple(p): r.output_ids for p, r in zip(prompts, reqs)}
        res[name] = {"no_speculation": base}
        cases = {"ngram": {}, "replay_all_right": {"drafter": _Replay(rec)}} \
            if name == "repeating" else \
            {"always_wrong": {"drafter": _Replay(rec, wrong=True)}}
        for cname, kw in cases.items():
            res[name][cname] = run(prompts, speculative=4, **kw)[1]
        print(name, res[name], flush=True)
    return res


def main():
    res = {"kernel": bench_kernel()}
    if not kernel_only:
        model = fuse_for_inference(build_model(
            "llama2-7b", dtype=torch.bfloat16, device=DEV).eval())
        res["step"] = bench_step(model)
        del model
        torch.cuda.empty_cache()
        res["engine"] = bench_engine()
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


main()
