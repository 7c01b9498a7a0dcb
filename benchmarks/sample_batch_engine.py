"""Wall time per Engine._sample_batch call (download included), the
sort-based / row-by-row path against the batched sampler
(batch_sampler=True), 32 x 32000 bf16 logits:
  (a) every row temperature 0.8, top_p 0.9
  (b) as (a), one row with a seed and a presence penalty
  (c) as (b), logprobs = 5 on every row

    python benchmarks/sample_batch_engine.py [OUT.json]
    rocprofv3 --kernel-trace --stats -- \
        python benchmarks/sample_batch_engine.py --profile-new
"""
import json
import sys
import time

import torch

sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1]))
from runbooks_amd.models import build_model  # noqa: E402
from runbooks_amd.serve import Engine  # noqa: E402
from runbooks_amd.serve.engine import Request  # noqa: E402

DEV = "cuda:0"
B, V = 32, 32000
profile_new = "--profile-new" in sys.argv
_pos = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = _pos[0] if _pos else "sample_batch_engine.json"


def reqs_for(case):
    g = torch.Generator().manual_seed(1)
    out = []
    for i in range(B):
        prompt = torch.randint(0, V, (200,), generator=g).tolist()
        r = Request(i, prompt, temperature=0.8, top_p=0.9)
        r.output_ids = torch.randint(0, V, (56,), generator=g).tolist()
        if case in "bc" and i == 7:
            r.seed = 1234
            r.presence_penalty = 0.5
        if case == "c":
            r.logprobs = 5
        out.append(r)
    return out


def main():
    model = build_model("smoke-llama", dtype=torch.bfloat16)
    old = Engine(model, device=DEV, kv_blocks=64, batch_sampler=False)
    new = Engine(model, device=DEV, kv_blocks=64, batch_sampler=True)
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(B, V, generator=g) * 4).to(torch.bfloat16).to(DEV)
    res = {}
    for case in "abc":
        reqs = reqs_for(case)

        def run(eng, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                eng._sample_batch(logits, reqs)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / n * 1e6
            for r in reqs:
                r.logprob_data.clear()
            return dt

        if profile_new:
            run(new, 10)
            run(new, 100)
            continue
        run(old, 10), run(new, 10)
        rounds = [(run(old, 100), run(new, 100)) for _ in range(5)]
        res[case] = {"old_us": [round(o, 1) for o, _ in rounds],
                     "new_us": [round(n, 1) for _, n in rounds]}
        print(case, res[case], flush=True)
    if not profile_new:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


main()
