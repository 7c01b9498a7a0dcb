"""gfx950 kernels of csrc/lora_serve.hip and the adapter decode path on
the GPU: numerics against fp64, the exact guarantees (untouched / zero
rows, batch independence, run-to-run identity), the model against the
CPU fp32 apply_lora reference, and the engine under graphs."""
import pytest
import torch

from runbooks_amd import ops
from runbooks_amd.models import build_model
from runbooks_amd.models.transformer import fuse_for_inference
from runbooks_amd.serve import Engine
from runbooks_amd.serve.lora import AdapterPool, LoraBatch
from runbooks_amd.train.lora import apply_lora, lora_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOTS = 4


def _idx(M, kind):
    """int32 [M] over 4 slots mixing -1, repeats and all-different."""
    if kind == "mixed":
        vals = [(-1 if m % 3 == 1 else (m * 7 + 1) % SLOTS) for m in range(M)]
    elif kind == "same":
        vals = [2] * M
    else:                       # as different as 4 slots allow
        vals = [m % SLOTS for m in range(M)]
    return torch.tensor(vals, dtype=torch.int32)


def _bf16(shape, g, std=1.0):
    return (torch.randn(shape, generator=g) * std).to(torch.bfloat16)


# ---------------------------------------------------------------------------
# lora_shrink
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("S,R", [(1, 16), (3, 16), (2, 16), (1, 64)])
@pytest.mark.parametrize("K", [256, 4096, 11008])
def test_lora_shrink(K, S, R):
    """K = 256 is less than one wave's 512-element stride, 11008 is ragged
    against it. Bound: bf16 products are exact in fp32 and K * 2^-24 *
    sum|x a| covers an fp32 summation in any order."""
    g = torch.Generator().manual_seed(K + 10 * S + R)
    a = _bf16((SLOTS, S * R, K), g)
    a_d = a.to(DEV)
    x33 = _bf16((33, K), g)
    outs = {}
    for M in (1, 5, 33):
        for kind in ("mixed", "same", "diff"):
            idx = _idx(M, kind)
            x = x33[:M].contiguous()
            t = ops.lora_shrink(x.to(DEV), a_d, idx.to(DEV), segments=S,
                                idx_cpu=idx)
            t2 = ops.lora_shrink(x.to(DEV), a_d, idx.to(DEV), segments=S)
            assert t.dtype == torch.float32 and t.shape == (M, S * R)
            assert torch.equal(t, t2), "run-to-run"
            t = t.cpu()
            live = idx >= 0
            assert (t[~live] == 0).all()
            ag = a[idx.clamp_min(0).long()].double()
            ref = torch.einsum("mk,mjk->mj", x.double(), ag)
            mag = torch.einsum("mk,mjk->mj", x.double().abs(), ag.abs())
            err = (t.double() - ref).abs()[live]
            bound = (K * 2.0 ** -24 * mag)[live]
            print(f"shrink K={K} S={S} R={R} M={M} {kind}: max err "
                  f"{err.max().item() if err.numel() else 0:.3e}, min "
                  f"slack {(bound - err).min().item() if err.numel() else 0:.3e}")
            assert (err <= bound).all()
            outs[(M, kind)] = (t, idx)
    # row m of the M = 33 batch == the M = 1 call on that row, bit for bit
    t33, idx33 = outs[(33, "mixed")]
    for m in (0, 2, 17, 32):
        one = ops.lora_shrink(x33[m:m + 1].contiguous().to(DEV), a_d,
                              idx33[m:m + 1].to(DEV), segments=S).cpu()
        assert torch.equal(one[0], t33[m]), m


# ---------------------------------------------------------------------------
# lora_expand_
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,seg_ends,R", [
    (256, (256,), 16), (512, (256, 384, 512), 16),
    (22016, (11008, 22016), 16), (4096, (4096,), 16), (4096, (4096,), 64)])
def test_lora_expand(N, seg_ends, R):
    """Bound: one bf16 ulp for the final rounding (2^-8 |ref|) plus fp32
    accumulation of R + 1 terms with margin (2^-20 of the magnitudes)."""
    S = len(seg_ends)
    g = torch.Generator().manual_seed(N + R + S)
    b = _bf16((SLOTS, N, R), g)
    b_d = b.to(DEV)
    sc = torch.rand(SLOTS, generator=g) * 2 + 0.25
    y33 = _bf16((33, N), g)
    t33 = torch.randn(33, S * R, generator=g)
    seg = torch.zeros(N, dtype=torch.long)
    for e in seg_ends[:-1]:
        seg += (torch.arange(N) >= e).long()
    outs = {}
    for M in (1, 5, 33):
        for kind in ("mixed", "same", "diff"):
            idx = _idx(M, kind)
            y0, t = y33[:M].contiguous(), t33[:M].contiguous()
            y = ops.lora_expand_(y0.to(DEV), t.to(DEV), b_d, sc.to(DEV),
                                 idx.to(DEV), seg_ends, idx_cpu=idx)
            y2 = ops.lora_expand_(y0.to(DEV), t.to(DEV), b_d, sc.to(DEV),
                                  idx.to(DEV), seg_ends)
            assert torch.equal(y, y2), "run-to-run"
            y = y.cpu()
            live = idx >= 0
            # the pattern in rows without an adapter is bit-untouched
            assert torch.equal(y[~live].view(torch.int16),
                               y0[~live].view(torch.int16))
            slot = idx.clamp_min(0).long()
            tj = t.double().view(M, S, R)[:, seg]               # [M, N, R]
            prod = tj * b[slot].double()
            s = sc[slot].double()[:, None]
            ref = y0.double() + s * prod.sum(-1)
            bound = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * (
                y0.double().abs() + s.abs() * prod.abs().sum(-1))
            err = (y.double() - ref).abs()[live]
            print(f"expand N={N} R={R} M={M} {kind}: max err "
                  f"{err.max().item() if err.numel() else 0:.3e}")
            assert (err <= bound[live]).all()
            outs[(M, kind)] = (y, idx)
    y_all, idx33 = outs[(33, "mixed")]
    for m in (0, 2, 17, 32):
        one = ops.lora_expand_(y33[m:m + 1].contiguous().to(DEV),
                               t33[m:m + 1].contiguous().to(DEV), b_d,
                               sc.to(DEV), idx33[m:m + 1].to(DEV),
                               seg_ends).cpu()
        assert torch.equal(one[0].view(torch.int16),
                           y_all[m].view(torch.int16)), m


# ---------------------------------------------------------------------------
# model and engine
# ---------------------------------------------------------------------------
SEED = 3
PROMPT = [5, 9, 2, 7, 11]
TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj",
           "down_proj")


@pytest.fixture(scope="module")
def base():
    """bf16 smoke-llama on the GPU, fused, and its exact values in fp32."""
    m = build_model("smoke-llama", dtype=torch.bfloat16, device=DEV,
                    seed=SEED)
    weights = {k: v.float().cpu() for k, v in m.state_dict().items()}
    return fuse_for_inference(m).eval(), weights


@pytest.fixture(scope="module")
def adapters():
    """Two random adapters whose values are exact in bf16."""
    ref = build_model("smoke-llama", dtype=torch.float32, seed=SEED)
    apply_lora(ref, r=16, alpha=32, targets=TARGETS)
    out = {}
    for name, seed in (("A", 101), ("B", 202)):
        g = torch.Generator().manual_seed(seed)
        out[name] = {k: (torch.randn(v.shape, generator=g) * 0.05)
                     .to(torch.bfloat16).float()
                     for k, v in lora_state_dict(ref).items()}
    return out


@pytest.fixture(scope="module")
def references(base, adapters):
    """name -> stacked [prefill, decode] logits of the CPU fp32 apply_lora
    model that shares the GPU model's exact bf16 values."""
    _, weights = base
    out = {}
    S = len(PROMPT)
    for name in ("none", "A", "B"):
        ref = build_model("smoke-llama", dtype=torch.float32, seed=SEED)
        ref.load_state_dict(weights)
        if name != "none":
            apply_lora(ref, r=16, alpha=32)
            ref.load_state_dict(adapters[name], strict=False)
        ref.eval()
        caches = ref.alloc_caches(4, "cpu")
        with torch.no_grad():
            lp = ref.prefill(torch.tensor([PROMPT]),
                             torch.arange(S, dtype=torch.int32), caches,
                             torch.arange(S, dtype=torch.int32))
            ld = ref.decode(torch.tensor([3]),
                            torch.tensor([S], dtype=torch.int32), caches,
                            torch.tensor([S], dtype=torch.int32),
                            torch.tensor([[0]], dtype=torch.int32),
                            torch.tensor([S + 1], dtype=torch.int32))
        out[name] = torch.cat([lp, ld]).float()
    return out


def _rel(got, ref):
    return (got - ref).abs().max().item() / ref.abs().max().item()


def test_references_are_separated(references):
    """The three references differ pairwise by >= 10x the 3e-2 tolerance
    the GPU logits are held to: a path that ignored idx cannot pass."""
    names = list(references)
    for i in range(3):
        for j in range(i + 1, 3):
            a, b = references[names[i]], references[names[j]]
            sep = (a - b).abs().max().item() / max(a.abs().max().item(),
                                                   b.abs().max().item())
            print(f"separation {names[i]}/{names[j]}: {sep:.3f}")
            assert sep >= 10 * 3e-2, (names[i], names[j], sep)


def test_model_decode_eager_matches_cpu_reference(base, adapters,
                                                  references):
    m, _ = base
    pool = AdapterPool(m, max_loras=2, rank=16)
    pool.load_state("A", adapters["A"], alpha=32)
    pool.load_state("B", adapters["B"], alpha=32)
    rows = [-1, pool.slot_of("A"), pool.slot_of("B")]
    S, bs = len(PROMPT), ops.BLOCK_SIZE
    caches = m.alloc_caches(8, DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    lp = m.prefill(
        torch.tensor([PROMPT] * 3, device=DEV),
        torch.arange(S, **i32).repeat(3), caches,
        torch.cat([torch.arange(S, **i32) + b * bs for b in range(3)]),
        lora=LoraBatch(pool, rows))
    ld = m.decode(
        torch.full((3,), 3, dtype=torch.long, device=DEV),
        torch.full((3,), S, **i32), caches,
        torch.tensor([b * bs + S for b in range(3)], **i32),
        torch.arange(3, **i32).view(3, 1), torch.full((3,), S + 1, **i32),
        lora=LoraBatch(pool, rows))
    torch.cuda.synchronize()
    for i, name in enumerate(("none", "A", "B")):
        got = torch.stack([lp[i], ld[i]]).float().cpu()
        err = _rel(got, references[name])
        print(f"eager row {name}: rel err {err:.4f}")
        assert err < 3e-2, (name, err)


def _lora_engine(m, adapters, max_loras=2, max_batch=4):
    eng = Engine(m, device=DEV, kv_blocks=128, seed=11, max_batch=max_batch,
                 max_loras=max_loras, prefix_cache=False)
    if max_loras:
        for name, state in adapters.items():
            eng.lora_pool.load_state(name, state, alpha=32)
    return eng


def test_model_decode_graphed_matches_cpu_reference(base, adapters,
                                                    references):
    """The same three rows through an Engine with graphs: prefill each
    request, then capture the logits of the first (graphed) decode step."""
    m, _ = base
    eng = _lora_engine(m, adapters)
    assert eng.use_graphs
    seen = {}
    orig = eng._sample_batch

    def spy(logits, reqs):
        if len(reqs) == 3 and "ld" not in seen:
            seen["ld"] = logits.float().cpu().clone()
        return orig(logits, reqs)

    eng._sample_batch = spy
    eng.max_prefills_per_step = 3
    first = []
    orig_first = eng._sample_first

    def spy_first(req, logits):
        first.append(logits[0].float().cpu().clone())
        orig_first(req, logits)
        return 3                # the reference's decode input token

    eng._sample_first = spy_first
    for a in (None, "A", "B"):
        eng.submit(list(PROMPT), max_new_tokens=2, adapter=a)
    eng.step()
    torch.cuda.synchronize()
    assert (4, "lora") in eng._graphed.graphs
    for i, name in enumerate(("none", "A", "B")):
        got = torch.stack([first[i], seen["ld"][i]])
        err = _rel(got, references[name])
        print(f"graphed row {name}: rel err {err:.4f}")
        assert err < 3e-2, (name, err)


def test_engine_mixed_requests_under_graphs(base, adapters):
    """6 requests over {none, A, B}, max_batch 4, greedy, 8 tokens:
    padding rows, bucket changes and adapter-free steps all occur. The
    adapter-free requests must produce the tokens a max_loras=0 engine
    produces for the same requests at the same batch positions, where
    only the graph family differs; their logits are compared at 3e-2 as
    well, step by step. (In a batch with an adapter row the adapter-free
    rows also take the plain-GEMM sites, so SwiGLU and the residual norm
    see bf16-rounded inputs where the fused epilogues keep fp32; on this
    model that moves no greedy token.)"""
    m, _ = base
    names = [None, "A", None, "B", "A", None]
    # one admission per step: the first step decodes request 0 alone, an
    # adapter-free step on the adapter-free graph family
    budgets = [8] * 6
    prompts = [[1 + i, 2, 3 + i, 4] for i in range(6)]

    def run(max_loras):
        eng = _lora_engine(m, adapters, max_loras=max_loras)
        rec = {}
        orig = eng._sample_batch

        def spy(logits, reqs):
            for i, r in enumerate(reqs):
                rec.setdefault(r.request_id, []).append(
                    logits[i].float().cpu().clone())
            return orig(logits, reqs)

        eng._sample_batch = spy
        reqs = [eng.submit(p, max_new_tokens=n,
                           adapter=a if max_loras else None)
                for p, n, a in zip(prompts, budgets, names)]
        while not all(r.finished for r in reqs):
            eng.step()
        return eng, [r.output_ids for r in reqs], \
            [rec[r.request_id] for r in reqs]

    eng, got, got_l = run(2)
    plain, want, want_l = run(0)
    V = eng.cfg.vocab_size
    for out, n in zip(got, budgets):
        assert len(out) == n and all(0 <= t < V for t in out)
    assert eng.stats["lora_decode_steps"] > 0
    assert eng.stats["lora_decode_steps"] < eng.stats["steps"]
    assert {k for k in eng._graphed.graphs if isinstance(k, tuple)}
    assert {k for k in eng._graphed.graphs if isinstance(k, int)}
    assert "lora_rows" not in plain.stats
    for i, a in enumerate(names):
        if a is not None:
            continue
        assert got[i] == want[i], (i, got[i], want[i])
        compared = 0
        for k, (lg, lw) in enumerate(zip(got_l[i], want_l[i])):
            if got[i][:k + 1] != want[i][:k + 1]:
                break
            err = _rel(lg, lw)
            assert err < 3e-2, (i, k, err)
            compared += 1
        assert compared >= 1
    assert any(got[i] != want[i] for i, a in enumerate(names) if a)
