"""Sliding-window prefill: what the windowed flash-forward instantiation
costs and saves at mistral-7b geometry (Hq 32, Hkv 8, Dh 128, B 1).

ops.flash_prefill with window = 0 and window = 4096 on the same tensors at
S = 4096 (the window covers every key: both calls run the unwindowed
kernel) and S = 8192 (a 256-row workgroup stages at most 70 of up to 128 KV
tiles; from tile counts alone, 0.75x the time). With --baseline-ext PATH
the flash_prefill of a second build of the extension (the parent commit's
_hip*.so) is timed in the same rounds as "baseline".

Times are device events around N back-to-back launches; the variants take
turns within each of REPS rounds in one process, after a warm-up of each.
Reported per variant: median, min and max over the rounds (us); the spread
to judge a difference by is max - min. Outputs are compared first: rows
below 4096 see the same keys with and without the window and must be
bit-identical, as must the baseline's output and window = 0.

    python benchmarks/window_prefill.py [OUT.json] [--baseline-ext PATH]
"""
import importlib.machinery
import importlib.util
import json
import math
import statistics
import sys

import torch

sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1]))
from runbooks_amd import ops  # noqa: E402

DEV = "cuda:0"
HQ, HKV, DH, W = 32, 8, 128, 4096
REPS, N = 9, 20


def load_ext(path):
    """A second build of the extension under another module name."""
    loader = importlib.machinery.ExtensionFileLoader("rb_baseline._hip", path)
    mod = importlib.util.module_from_spec(
        importlib.util.spec_from_loader("rb_baseline._hip", loader))
    loader.exec_module(mod)
    return mod


def timed(fn, n):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def rounds(variants):
    for fn in variants.values():
        timed(fn, 5)
    got = {k: [] for k in variants}
    for _ in range(REPS):
        for k, fn in variants.items():
            got[k].append(timed(fn, N))
    return {k: {"median_us": round(statistics.median(v), 1),
                "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
            for k, v in got.items()}


def main():
    args = sys.argv[1:]
    base = None
    if "--baseline-ext" in args:
        i = args.index("--baseline-ext")
        base = load_ext(args[i + 1])
        del args[i:i + 2]
    out_path = args[0] if args else "window_prefill.json"
    assert ops.has_hip(), "needs the gfx950 extension and a GPU"
    res = {}
    for S in (4096, 8192):
        torch.manual_seed(S)
        q, k, v = (torch.randn(1, S, h, DH, dtype=torch.bfloat16, device=DEV)
                   for h in (HQ, HKV, HKV))
        variants = {"window0": lambda: ops.flash_prefill(q, k, v),
                    f"window{W}": lambda: ops.flash_prefill(q, k, v, window=W)}
        o0, ow = (fn() for fn in variants.values())
        assert torch.equal(o0[:, :W], ow[:, :W]), "rows below W changed"
        assert S == W or not torch.equal(o0, ow), "the window had no effect"
        if base is not None:
            variants["baseline"] = lambda: base.flash_prefill(
                q, k, v, 1.0 / math.sqrt(DH))
            assert torch.equal(variants["baseline"](), o0), "window0 != baseline"
        res[f"S{S}"] = r = rounds(variants)
        for name, t in r.items():
            print(f"S={S:5d} {name:11s} median {t['median_us']:8.1f} us  "
                  f"min {t['min_us']:8.1f}  max {t['max_us']:8.1f}  "
                  f"x window0 {t['median_us'] / r['window0']['median_us']:.3f}",
                  flush=True)
    with open(out_path, "w") as f:
        json.dump({"geometry": {"Hq": HQ, "Hkv": HKV, "Dh": DH, "window": W},
                   "reps": REPS, "launches_per_timing": N, "results": res},
                  f, indent=2)


if __name__ == "__main__":
    main()
