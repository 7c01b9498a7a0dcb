#!/usr/bin/env python3
"""What prefilling from the paged cache buys a serving engine (llama2-7b,
random weights, one GPU).

    python benchmarks/prefix_ttft.py [--rounds 2] [--out FILE.json]
                                     [--experiments prefix,chunk,burst]

Three experiments, each run in alternating fresh child processes so neither
setting inherits a warm allocator, graph or library state from the other:

* prefix: requests share a 1024-token prefix and add 64 tokens of their
  own. Request 1 fills the prefix cache; the admission step() of requests
  2..9 is timed with prefill_from_cache off and on (max_new_tokens=1, so
  the step is the prefill alone).
* chunk: 8 sequences are decoding when a 4096-token prompt arrives; the
  largest single step() time until its first token is reported for
  prefill_chunk 0 and 512, next to the plain decode step time. An untimed
  4096-token prompt runs first so library warm-up is not in the figure.
* burst: eight requests arrive together and the time until all eight have
  their first token is reported, with prefill_batch 0 (eight forwards in
  one step, max_prefills_per_step=8) and 8 (one packed forward). "shared":
  after one request has filled a 1024-token prefix, each of the eight adds
  64 own tokens (prefill_from_cache on in both settings). "cold": eight
  unrelated 256-token prompts. An untimed burst of each kind runs first.

Times are host clocks around step(), which ends in a device sync.
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODEL = "llama2-7b"
PREFIX, UNIQUE, LONG, CHUNK = 1024, 64, 4096, 512


def _timed_step(eng, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def child_prefix(from_cache: bool) -> dict:
    import torch

    from runbooks_amd.serve import Engine
    eng = Engine(MODEL, kv_blocks=3072, seed=1, prefix_cache=True,
                 prefill_from_cache=from_cache, prefill_chunk=0)
    g = torch.Generator().manual_seed(0)
    vocab = eng.cfg.vocab_size
    shared = torch.randint(1, vocab, (PREFIX,), generator=g).tolist()
    ms = []
    for i in range(9):
        tail = torch.randint(1, vocab, (UNIQUE,), generator=g).tolist()
        req = eng.submit(shared + tail, max_new_tokens=1)
        ms.append(_timed_step(eng, torch))
        assert req.finished and len(req.output_ids) == 1
    return {"prefill_from_cache": from_cache, "fill_ms": round(ms[0], 2),
            "admit_ms": [round(x, 2) for x in ms[1:]],
            "admit_ms_median": round(statistics.median(ms[1:]), 2),
            "prefill_tokens": eng.stats["prefill_tokens"],
            "prefix_skipped_tokens": eng.stats["prefix_skipped_tokens"]}


def child_chunk(chunk: int) -> dict:
    import torch

    from runbooks_amd.serve import Engine
    eng = Engine(MODEL, kv_blocks=3072, seed=1, prefix_cache=False,
                 prefill_from_cache=False, prefill_chunk=chunk)
    g = torch.Generator().manual_seed(0)
    vocab = eng.cfg.vocab_size
    running = [eng.submit(torch.randint(1, vocab, (64,), generator=g).tolist(),
                          max_new_tokens=2000) for _ in range(8)]
    while len(eng.running) < 8:
        eng.step()
    decode = [_timed_step(eng, torch) for _ in range(20)][5:]
    worst = None
    for timed in (False, True):     # the first long prompt only warms up
        long = eng.submit(torch.randint(1, vocab, (LONG,),
                                        generator=g).tolist(),
                          max_new_tokens=1)
        steps = []
        while not long.finished:
            n0 = [len(r.output_ids) for r in running]
            steps.append(_timed_step(eng, torch))
            assert all(len(r.output_ids) == n + 1
                       for r, n in zip(running, n0)), "decode starved"
        if timed:
            worst = steps
    return {"prefill_chunk": chunk,
            "decode_step_ms_median": round(statistics.median(decode), 2),
            "steps_to_first_token": len(worst),
            "worst_step_ms": round(max(worst), 2),
            "total_ms": round(sum(worst), 2)}


BURST, COLD, REPEATS = 8, 256, 3


def child_burst(batch: int) -> dict:
    import torch

    from runbooks_amd.serve import Engine
    eng = Engine(MODEL, kv_blocks=3072, seed=1, prefix_cache=True,
                 prefill_from_cache=True, prefill_chunk=0,
                 prefill_batch=batch)
    eng.max_prefills_per_step = BURST
    g = torch.Generator().manual_seed(0)
    vocab = eng.cfg.vocab_size

    def rand(n):
        return torch.randint(1, vocab, (n,), generator=g).tolist()

    def burst(prompts):
        reqs = [eng.submit(p, max_new_tokens=1) for p in prompts]
        ms, steps = 0.0, 0
        while not all(r.finished for r in reqs):
            ms += _timed_step(eng, torch)
            steps += 1
        assert all(len(r.output_ids) == 1 for r in reqs)
        return ms, steps

    shared_ms, cold_ms, steps = [], [], set()
    for i in range(REPEATS + 1):            # the first of each only warms up
        shared = rand(PREFIX)
        fill = eng.submit(shared + rand(UNIQUE), max_new_tokens=1)
        while not fill.finished:
            eng.step()
        skipped0 = eng.stats["prefix_skipped_tokens"]
        ms_s, n_s = burst([shared + rand(UNIQUE) for _ in range(BURST)])
        assert eng.stats["prefix_skipped_tokens"] - skipped0 == BURST * PREFIX
        ms_c, n_c = burst([rand(COLD) for _ in range(BURST)])
        eng.flush_prefix_cache()
        if i:
            shared_ms.append(ms_s)
            cold_ms.append(ms_c)
            steps.update((n_s, n_c))
    assert steps == {1}, steps              # every burst is one step()
    assert eng.stats["prefill_batches"] == (2 * (REPEATS + 1) if batch > 1
                                            else 0)
    return {"prefill_batch": batch,
            "shared_ms": [round(x, 2) for x in shared_ms],
            "shared_ms_median": round(statistics.median(shared_ms), 2),
            "cold_ms": [round(x, 2) for x in cold_ms],
            "cold_ms_median": round(statistics.median(cold_ms), 2)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--out", default=None)
    p.add_argument("--experiments", default="prefix,chunk,burst")
    p.add_argument("--child", choices=["prefix", "chunk", "burst"],
                   default=None)
    p.add_argument("--value", type=int, default=0)
    args = p.parse_args()
    if args.child == "prefix":
        print("RESULT " + json.dumps(child_prefix(bool(args.value))))
        return
    if args.child == "chunk":
        print("RESULT " + json.dumps(child_chunk(args.value)))
        return

    if args.child == "burst":
        print("RESULT " + json.dumps(child_burst(args.value)))
        return

    def run(kind, value):
        r = subprocess.run([sys.executable, os.path.abspath(__file__),
                            "--child", kind, "--value", str(value)],
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"{kind} child (value {value}) failed: "
                             f"exit {r.returncode}")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        print(f"{kind} {value}: done", file=sys.stderr, flush=True)
        return json.loads(line[-1][len("RESULT "):])

    res = {"model": MODEL, "prefix_tokens": PREFIX, "unique_tokens": UNIQUE,
           "long_prompt": LONG, "burst_requests": BURST,
           "cold_tokens": COLD, "prefix": [], "chunk": [], "burst": []}
    todo = args.experiments.split(",")
    for kind, values in (("prefix", (0, 1)), ("chunk", (0, CHUNK)),
                         ("burst", (0, BURST))):
        if kind not in todo:
            continue
        for _ in range(args.rounds):
            for v in values:
                res[kind].append(run(kind, v))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
